"""The eigenvector augmentations without a GPU (csrc/dgn_eig_augment.hip, dgn_amd.EigAugment): the numpy Philox of tests/eig_augment_ref.py
against the Random123 known answers, the fp64 restatement of the two training loops against the reference's own recorded runs
(tests/golden/g20_eig_augment.npz: uniforms in, ``ndata['eig']`` as the model saw it out), and every argument check that needs no device."""
import os

import numpy as np
import pytest
import torch

import eig_augment_ref as R


@pytest.fixture(scope="module")
def lib():
    from dgn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# Random123's kat_vectors for philox4x32_10: counter, key -> output
_KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def test_philox_known_answers():
    for counter, key, want in _KAT:
        got = R.philox4x32_10(np.array(counter, dtype=np.uint32), np.array(key, dtype=np.uint32))
        assert got.dtype == np.uint32 and got.tolist() == list(want), [hex(v) for v in got]
    # vectorised over the counters, one key: row by row the same numbers
    counters = np.array([k[0] for k in _KAT], dtype=np.uint32)
    many = R.philox4x32_10(counters, np.array(_KAT[2][1], dtype=np.uint32))
    for row, c in zip(many, counters):
        assert row.tolist() == R.philox4x32_10(c, np.array(_KAT[2][1], dtype=np.uint32)).tolist()


def test_kernel_draws_layout():
    """Counter (lo32 i, hi32 i, lo32 calls, hi32 calls), key (lo32 key, hi32 key); u from the top 24 bits of r[0], the signs from r[1]."""
    key, calls = (0x299f31d0 << 32) | 0xa4093822, (0x03707344 << 32) | 0x13198a2e
    u, plus = R.kernel_draws(3, key, calls)
    for i in range(3):
        r = R.philox4x32_10(np.array([i, 0, 0x13198a2e, 0x03707344], dtype=np.uint32), np.array([0xa4093822, 0x299f31d0], dtype=np.uint32))
        assert u[i] == float(int(r[0]) >> 8) / 2 ** 24 and 0 <= u[i] < 1
        assert [bool((int(r[1]) >> j) & 1) for j in range(32)] == plus[i].tolist()
    assert np.float32(u).astype(np.float64).tolist() == u.tolist()                  # 24 bits: exact in fp32
    assert not np.array_equal(R.kernel_draws(3, key, calls + 1)[0], u)


@pytest.mark.parametrize("case", ["molecules_flip", "superpixels_rot30", "superpixels_flip", "superpixels_rot30_flip"])
def test_restatement_reproduces_the_reference_loops(golden, case):
    """The restatement, fed the uniforms the reference's loop drew, gives the eig its model saw: bit for bit where only signs change,
    within 1e-6 max|eig| where the rotation's fp32 arithmetic rounds (the signs of the flipped column exact there too)."""
    g = golden("g20_eig_augment")
    assert case in g["cases"].tolist()
    eig, seen = g[f"{case}/eig_in"], g[f"{case}/eig_seen"]
    aug, flip = float(g[f"{case}/augmentation"]), bool(g[f"{case}/flip"])
    draws = [g[f"{case}/u{j}"] for j in range(int(g[f"{case}/n_draws"]))]
    assert eig.shape == (40, 6) and eig.dtype == np.float32 and (eig == 0).sum() == 10
    if case == "molecules_flip":
        (u,) = draws
        out, _ = R.augment(eig, 0.0, None, range(6), u >= 0.5)
    else:
        rot = aug > 1e-7
        assert len(draws) == int(rot) + int(flip)
        out, _ = R.augment(eig, aug if rot else 0.0, draws[0] if rot else None, [2] if flip else [], (draws[-1] >= 0.5)[:, None] if flip else None)
    assert not np.array_equal(seen, eig)
    if aug <= 1e-7:
        assert R.same_bits(out, seen)                                               # -0.0 included
        assert np.signbit(seen[eig == 0]).any()
    else:
        tol = 1e-6 * np.abs(eig).max()
        assert np.abs(out - seen).max() <= tol
        big = np.abs(out) > tol                                                     # (below the tolerance a sign is rounding's)
        assert big[:, 1:3].sum() >= 70 and np.array_equal(np.signbit(out[big]), np.signbit(seen[big]))
        untouched = [0, 3, 4, 5]
        assert R.same_bits(out[:, untouched], seen[:, untouched])


def test_restatement_zero_sign_and_untouched_columns():
    eig = np.array([[0.0, 1.0, -2.0], [-0.0, 0.0, 3.0]], dtype=np.float32)
    out, safe = R.augment(eig, 0.0, None, [0, 2], np.array([[False, True], [False, False]]))
    assert R.same_bits(out, np.array([[-0.0, 1.0, -2.0], [0.0, 0.0, -3.0]], dtype=np.float32)) and safe.tolist() == [1.0, 1.0]
    out, safe = R.augment(eig, 180.0, np.array([0.75, 0.5]), [], None)               # +90 degrees: (x1, x2) -> (x2, -x1); 0 degrees: unchanged
    np.testing.assert_allclose(out, [[0.0, -2.0, -1.0], [-0.0, 0.0, 3.0]], atol=1e-15)
    np.testing.assert_allclose(safe, [0.0, 1.0], atol=1e-30)


def test_eig_augment_argument_checks_need_no_device():
    from dgn_amd import EigAugment, _lib
    from dgn_amd.eig import _flip_mask
    assert _flip_mask(None) == 0 and _flip_mask("all") == 0xFFFFFFFF and _flip_mask(2) == 4 and _flip_mask([0, 5, 31]) == 1 | 32 | 1 << 31
    assert _flip_mask(()) == 0 and _flip_mask(range(6)) == 63
    for bad, exc in ((dict(flip=True), TypeError), (dict(flip=32), ValueError), (dict(flip=-1), ValueError), (dict(flip="column 2"), ValueError),
                     (dict(flip=[1.5]), TypeError), (dict(flip=[0, 40]), ValueError), (dict(rotate_deg=float("nan")), ValueError),
                     (dict(rotate_deg=float("inf")), ValueError), (dict(seed=-1), ValueError), (dict(seed=2 ** 63), ValueError),
                     (dict(seed=1.5), ValueError)):
        with pytest.raises(exc, match="EigAugment"):
            EigAugment(device="cuda:0", **bad)
    with pytest.raises(_lib.DgnError, match="CUDA"):
        EigAugment(device="cpu")
    with pytest.raises(TypeError):
        EigAugment.superpixels(30, True, flip=2)                                    # the preset owns the column


def test_ops_eig_augment_refuses_cpu_tensors():
    from dgn_amd import _lib, ops
    with pytest.raises(_lib.DgnError, match="CUDA"):
        ops.eig_augment(torch.zeros(4, 6), torch.zeros(4, dtype=torch.int64), 0.0, 63)


def test_c_abi_validates_before_any_device_work(lib):
    from dgn_amd import _lib
    err = lambda: lib.dgn_last_error().decode()
    a = 1 << 12                                                                    # dummy aligned pointer, never dereferenced
    call = lambda n, K, eig, ld_in, out, ld_out, deg, mask, state: lib.dgn_eig_augment(n, K, eig, ld_in, out, ld_out, deg, mask, state, None)
    assert call(0, 6, None, 6, None, 6, 0.0, 63, None) == _lib.DGN_OK                # no rows: nothing launched, state untouched
    assert call(0, 6, None, 6, None, 6, 30.0, -1, None) == _lib.DGN_OK               # (a mask with bit 31 set is a negative int32)
    assert call(-1, 6, a, 6, a, 6, 0.0, 63, a) == _lib.DGN_ERR_INVALID and "n_rows" in err()
    assert call(10, 0, a, 6, a, 6, 0.0, 63, a) == _lib.DGN_ERR_INVALID and "1 <= K <= 32" in err()
    assert call(10, 33, a, 33, a, 33, 0.0, 63, a) == _lib.DGN_ERR_INVALID and "1 <= K <= 32" in err()
    assert call(10, 2, a, 2, a, 2, 15.0, 0, a) == _lib.DGN_ERR_INVALID and "K >= 3" in err()
    assert call(0, 2, None, 2, None, 2, 15.0, 0, None) == _lib.DGN_ERR_INVALID       # (an error even without rows)
    assert call(10, 6, a, 5, a, 6, 0.0, 63, a) == _lib.DGN_ERR_INVALID and "strides" in err()
    assert call(10, 6, a, 6, a, 5, 0.0, 63, a) == _lib.DGN_ERR_INVALID and "strides" in err()
    assert call(10, 6, a, 6, a, 6, float("nan"), 63, a) == _lib.DGN_ERR_INVALID and "finite" in err()
    assert call(10, 6, None, 6, a, 6, 0.0, 63, a) == _lib.DGN_ERR_INVALID and "null" in err()
    assert call(10, 6, a, 6, a, 6, 0.0, 63, None) == _lib.DGN_ERR_INVALID and "null" in err()
    assert call(10, 6, a, 8, a, 6, 0.0, 63, a) == _lib.DGN_ERR_INVALID and "in place" in err()
    assert _lib.ABI_VERSION >= 38 and "dgn_eig_augment" in _lib.EXPORTS
