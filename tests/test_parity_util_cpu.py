"""tests/parity_util.py's comparator for row-reduced tensors (``check_reduced``) on synthetic tensors, no GPU: what it accepts and
what it has to reject, and what ``check`` returns."""
import pytest
import torch

import parity_util
from parity_util import check, check_reduced


@pytest.fixture(autouse=True)
def _no_report_file(monkeypatch):
    monkeypatch.setattr(parity_util, "_to_report_file", lambda line: None)


def _gradient_like(rows=300, cols=48, rel=1e-3, seed=0):
    """a weight gradient of scale ~1e3 and an 'fp32 oracle' that is ``rel`` (relative, per entry) off it, as at 275 k rows"""
    gen = torch.Generator().manual_seed(seed)
    r64 = 300.0 * torch.randn(rows, cols, generator=gen, dtype=torch.float64)
    r32 = (r64 * (1 + rel * torch.randn(rows, cols, generator=gen, dtype=torch.float64))).float()
    return r32, r64


def test_check_reduced_accepts_the_fp32_oracle_itself_and_reports_ratio_one():
    r32, r64 = _gradient_like()
    res = check_reduced(r32, r32, r64, "r32 itself")
    assert res.e_ours == res.e_ref > 0 and res.l_ours == res.l_ref > 0
    assert "E_ours/E_ref=1.000" in parity_util.REPORT[-1]
    better = r64 + 0.25 * (r32.double() - r64)          # a hierarchical sum: inside the sequential sum's error
    assert check_reduced(better.float(), r32, r64, "a quarter of the error").e_ours < res.e_ref


def test_check_reduced_rejects_one_and_a_half_times_the_oracles_error():
    r32, r64 = _gradient_like()
    worse = r64 + 1.5 * (r32.double() - r64)
    with pytest.raises(AssertionError):
        check_reduced(worse, r32, r64, "x1.5")
    check_reduced(worse, r32, r64, "x1.5 under the named x2 widening", margin=2.0)
    with pytest.raises(AssertionError):
        check_reduced(worse, r32, r64, "no other margin", margin=4.0)
    # ... which check's x4 band lets through: the reason for the second comparator
    check(worse, r32, r64, "x1.5 through check", rtol=1e-4, atol=2e-5)


def test_check_reduced_rejects_one_column_scaled_by_two_percent():
    r32, r64 = _gradient_like()
    a = r32.clone()
    a[:, 7] *= 1 + 2e-2
    with pytest.raises(AssertionError):
        check_reduced(a, r32, r64, "one column x 1.02")


def test_check_reduced_l2_clause_catches_what_the_worst_entry_hides():
    """every entry moved by 0.9 x the oracle's WORST error: the max clause holds, the L2 clause does not"""
    r32, r64 = _gradient_like()
    e_ref = float((r32.double() - r64).abs().max())
    a = r64 + 0.9 * e_ref * torch.sign(torch.randn(r64.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64))
    with pytest.raises(AssertionError, match="L2"):
        check_reduced(a, r32, r64, "uniformly at the worst entry's error")


def test_check_reduced_accepts_a_numerically_zero_tensor_through_checks_bound():
    """the gradient of a bias in front of a BatchNorm: fp64 value ~1e-13, both fp32 evaluations rounding noise, entry by entry unrelated"""
    gen = torch.Generator().manual_seed(1)
    r64 = 1e-13 * torch.randn(70, generator=gen, dtype=torch.float64)
    r32 = 9e-4 * torch.randn(70, generator=gen)
    ours = 9e-4 * torch.randn(70, generator=gen)
    assert check_reduced(ours, r32, r64, "zero tensor") is None
    assert check_reduced(torch.zeros(70), r32, r64, "exact zeros") is None
    with pytest.raises(AssertionError):
        check_reduced(ours + 0.5, r32, r64, "not noise")


def test_check_reduced_floors_hold_where_the_fp32_oracle_is_exact():
    _, r64 = _gradient_like()
    r32 = r64.float()                                       # (rounded once: error 6e-8 relative, below the floors)
    a = r64 * (1 + 1e-5)
    res = check_reduced(a, r32, r64, "inside the floors")
    assert res.e_ours > res.e_ref and res.l_ours > res.l_ref
    with pytest.raises(AssertionError):
        check_reduced(r64 * (1 + 5e-4), r32, r64, "outside the floors")


def test_check_returns_its_three_counts():
    gen = torch.Generator().manual_seed(2)
    r64 = torch.randn(1000, generator=gen, dtype=torch.float64)
    r32 = r64.float().clone()
    r32[:3] += 1.0                                          # three routing flips of the oracle's own
    a = r64.float().clone()
    a[:3] += 1.0                                            # ... which we share
    a[10] += 3e-4                                           # one entry of ours on the tensor-wide clause (tol 1.2e-4 + 4 x 1.0)
    counts = check(a, r32, r64, "counts", rtol=1e-4, atol=2e-5)
    assert counts == (0, 1, 0) and counts.escaped == 1
    a[1] -= 1.0                                             # the oracle flipped here, we did not
    counts = check(a, r32, r64, "counts", rtol=1e-4, atol=2e-5)
    assert (counts.local, counts.escaped, counts.oracle_fp32_flips) == (0, 1, 1)
