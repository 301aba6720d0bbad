"""Shared parity criterion of the layer-level oracle tests, WITH its bookkeeping: an entry passes when it is within
tolerance of the fp32 oracle (the reference's own arithmetic), or -- the escape clause -- as close to the fp64 oracle as the fp32 oracle
itself is (x4): max / min / |.| routings flip between fp32 evaluations where two messages tie or a residual sits on zero, in the
reference as much as here.  Every call REPORTS the achieved maximum error and how many entries needed the escape clause (pytest -rA
shows the lines) -- apart from the entries on which the fp32 oracle itself left its fp64 evaluation by more than the tolerance, which
are reported as the oracle's flips -- and asserts that they are at most 0.5 % of the tensor: a regression from 3e-6 to 1.9e-5, or a kernel that leans on
the clause, no longer passes silently.  The LOCAL clause is capped too (1 % of the tensor by default).  Only tensors whose true value is
numerically ZERO everywhere -- the fp64 oracle's largest entry is at most 1e-6 of the upstream (cotangent) scale: the gradient of a bias
in front of a BatchNorm -- are exempt from the fractions: both evaluations return rounding noise there, entry by entry unrelated
(the round-5 exemption, "fp64 value <= 1e3 x the fp32 oracle's worst error", let any tensor with one max / min
routing flip through).  ``max_escape_fraction = 0`` is what the BASELINE-config tests pass: no entry may need the tensor-wide clause;
lists with ``std`` (ill-conditioned in the reference's own fp32 arithmetic, profiles/NOTES.md) name their looser caps explicitly.

``check_reduced`` is the second comparator, for tensors that are SUMS OVER THE BATCH'S ROWS (parameter gradients) at sizes where the fp32
oracle's own near-sequential sum is 1e-3 (relative) off its fp64 evaluation: there ``check``'s x4 band is a 0.5 - 2 % band, wide enough for
a kernel that loses a slab of partial sums.  It judges the kernels against the fp64 oracle and allows the reference's own fp32 error on
that tensor, x1."""
import collections
import os

import torch

REPORT = []
MAX_ESCAPE_FRACTION = 0.005
MAX_LOCAL_FRACTION = 0.01
ZERO_TENSOR = 1e-6          # max|fp64 value| <= ZERO_TENSOR x upstream scale: a numerically zero tensor
REPORT_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity_report.txt")


def _to_report_file(line):
    """Every comparison's line also goes to gpurun_out/parity_report.txt (merged back from the GPU box): the achieved errors and the number
    of entries that needed the fp64 clause are on record whatever pytest's verbosity was."""
    try:
        os.makedirs(os.path.dirname(REPORT_FILE), exist_ok=True)
        with open(REPORT_FILE, "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def note(line):
    """A line of a test's own (a measured ratio next to its assertion) into the same report as the comparators' lines."""
    REPORT.append(line)
    print(line)
    _to_report_file(line)


def check(ours, r32, r64, name, rtol, atol, abs_scale=None, exempt_noise=True, max_escape_fraction=None, max_local_fraction=None,
          upstream_scale=1.0):
    """``|ours - r32| <= atol * scale + rtol * |r64|`` per entry (scale = max(1, max|r64|) unless given), or the fp64 clause.
    ``upstream_scale``: the size of the cotangent the tensor's gradient was pulled back from (1 for the suite's unit-variance cotangents);
    a tensor is "numerically zero" -- exempt from the clause caps -- when max|fp64 value| <= 1e-6 of it.
    Returns the three counts of its line: ``Counts(local, escaped, oracle_fp32_flips)``."""
    a, r32, r64 = ours.detach().cpu().double(), r32.detach().cpu().double(), r64.detach().cpu().double()
    scale = abs_scale if abs_scale is not None else max(1.0, float(r64.abs().max()) if r64.numel() else 1.0)
    tol = atol * scale + rtol * r64.abs()
    ref_err = float((r32 - r64).abs().max()) if r64.numel() else 0.0
    ok_ref = (a - r32).abs() <= tol
    # the fp64 clause, LOCAL first: an entry may sit as far from the fp64 oracle as the fp32 oracle's OWN error at that entry (x4) -- where
    # the reference's arithmetic itself is unsure.  Only what that does not cover falls back on the tensor-wide bound (the kernel's max /
    # min / |.| routing flipped on an entry where the oracle's did not): those entries are the counted, capped ones.
    ok_local = (a - r64).abs() <= tol + 4 * (r32 - r64).abs()
    ok_f64 = (a - r64).abs() <= tol + 4 * ref_err
    bad = ~(ok_ref | ok_local | ok_f64)
    # entries where the fp32 ORACLE itself is off its fp64 evaluation by more than the tolerance (a max / min / |.| routing that flipped
    # in the reference's own arithmetic: CPU thread count and summation order move them) are the oracle's, not ours: counted apart
    oracle_flip = (r32 - r64).abs() > tol
    flips = int((~ok_ref & (ok_local | ok_f64) & oracle_flip).sum())
    local = int((~ok_ref & ok_local & ~oracle_flip).sum())
    escaped = int((~ok_ref & ~ok_local & ok_f64 & ~oracle_flip).sum())
    n = a.numel()
    err32 = float((a - r32).abs().max()) if n else 0.0
    err64 = float((a - r64).abs().max()) if n else 0.0
    line = (f"PARITY {name}: n={n} max|ours-fp32 oracle|={err32:.3e} max|ours-fp64 oracle|={err64:.3e} oracle's own fp32 error={ref_err:.3e} "
            f"scale={scale:.3g} local_clause={local} escaped={escaped} ({100.0 * escaped / max(n, 1):.3f} %) oracle_fp32_flips={flips}")
    REPORT.append(line)
    print(line)
    _to_report_file(line)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {n} entries off ({line})"
    noise = exempt_noise and float(r64.abs().max() if n else 0.0) <= ZERO_TENSOR * max(float(upstream_scale), 1e-30)
    if not noise:
        if max_escape_fraction is None:
            allowed = max(1, int(MAX_ESCAPE_FRACTION * n))
        else:
            allowed = int(max_escape_fraction * n)
        assert escaped <= allowed, f"{name}: {escaped} of {n} entries needed the fp64 clause (allowed {allowed}): {line}"
        cap = MAX_LOCAL_FRACTION if max_local_fraction is None else max_local_fraction
        allowed_local = max(1, int(cap * n))
        assert local <= allowed_local, f"{name}: {local} of {n} entries needed the local fp64 clause (allowed {allowed_local}): {line}"
    return Counts(local, escaped, flips)


def numerically_zero(r64, upstream_scale=1.0):
    """``check``'s definition: the fp64 oracle's largest entry is at most 1e-6 of the upstream (cotangent) scale."""
    return r64.numel() == 0 or float(r64.detach().abs().max()) <= ZERO_TENSOR * max(float(upstream_scale), 1e-30)


Counts = collections.namedtuple("Counts", "local escaped oracle_fp32_flips")
Reduced = collections.namedtuple("Reduced", "e_ours e_ref l_ours l_ref")
FLOOR_L2 = 2e-5


def check_reduced(ours, r32, r64, name, rtol=1e-4, atol=2e-5, margin=1.0, upstream_scale=1.0):
    """A row-reduced tensor (a parameter gradient: every entry a sum over the batch's rows) against the FP64 oracle, the allowance being the
    reference's own fp32 error on this tensor, measured in this call:

        E_ref = max|r32 - r64|,  L_ref = ||r32 - r64||_2 / ||r64||_2
        max|ours - r64| <= margin * max(E_ref, floor)   and   ||ours - r64||_2 / ||r64||_2 <= margin * max(L_ref, FLOOR_L2)

    ``floor`` is the suite's tolerance ``atol * scale + rtol * |r64|`` at the worst entry (scale = max(1, max|r64|), as in ``check``); the
    floors only matter where the fp32 oracle is (nearly) exact.  ``margin`` is 1: the library's reductions are hierarchical (fp32 tiles,
    per-workgroup slots, fp64 finalize) and have to sit inside the error of the reference's near-sequential fp32 sum; 2 is the only other
    value a caller may pass, on a named tensor with the cause written next to the call.  A numerically zero tensor (``check``'s definition:
    max|r64| <= 1e-6 of the upstream scale) has no meaningful ratio: it goes to ``check`` with its existing exemption and bound.
    The line (pytest -rA and the report file, as ``check``'s) carries E_ours, E_ref, their ratio, L_ours, L_ref."""
    assert margin in (1.0, 2.0), "check_reduced: the margin is 1; 2 on a named tensor with its cause written down, nothing else"
    a, b32, b64 = ours.detach().cpu().double(), r32.detach().cpu().double(), r64.detach().cpu().double()
    n = a.numel()
    if numerically_zero(b64, upstream_scale):
        check(ours, r32, r64, name + " [numerically zero: check's bound]", rtol=rtol, atol=atol, upstream_scale=upstream_scale)
        return None
    assert a.shape == b64.shape == b32.shape, f"{name}: shapes {tuple(a.shape)} / {tuple(b32.shape)} / {tuple(b64.shape)}"
    scale = max(1.0, float(b64.abs().max()))
    err = (a - b64).abs().flatten()
    worst = int(err.argmax())
    e_ours, e_ref = float(err[worst]), float((b32 - b64).abs().max())
    floor = atol * scale + rtol * float(b64.flatten()[worst].abs())
    norm = float(b64.norm())
    l_ours, l_ref = float((a - b64).norm()) / norm, float((b32 - b64).norm()) / norm
    line = (f"PARITY-REDUCED {name}: n={n} E_ours={e_ours:.3e} E_ref={e_ref:.3e} E_ours/E_ref={e_ours / max(e_ref, 1e-300):.3f} "
            f"L_ours={l_ours:.3e} L_ref={l_ref:.3e} L_ours/L_ref={l_ours / max(l_ref, 1e-300):.3f} scale={scale:.3g} floor={floor:.3e} margin=x{margin:g}")
    note(line)
    assert bool(torch.isfinite(a).all()), f"{name}: not finite ({line})"
    assert e_ours <= margin * max(e_ref, floor), f"{name}: worst entry further from the fp64 oracle than the fp32 oracle's worst ({line})"
    assert l_ours <= margin * max(l_ref, FLOOR_L2), f"{name}: L2 error above the fp32 oracle's own ({line})"
    return Reduced(e_ours, e_ref, l_ours, l_ref)
