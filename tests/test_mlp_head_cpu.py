"""The fused MLPReadout head (csrc/dgn_mlp_head.hip) without a GPU: the domain that ``dgn_mlp_head_supported`` reports, the workspace size,
the argument checks that run before any device work, and the Python side on CPU tensors (``MLPReadout`` keeps torch's route there,
``ops.mlp_head`` refuses).  Needs the built library, like tests/test_abi.py."""
import ctypes as C
import os

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from dgn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _i32(values):
    return (C.c_int32 * len(values))(*values)


SHIPPED = [(45, 22, 11, 1), (47, 23, 11, 2), (70, 35, 17, 1), (70, 70, 70, 128)]      # ZINC, PATTERN, HIV, PCBA


def _weights(dims):
    return sum(a * b for a, b in zip(dims[:-1], dims[1:]))


def test_supported_over_the_edges_of_the_domain(lib):
    sup = lambda dims: lib.dgn_mlp_head_supported(len(dims) - 1, _i32(dims))
    for dims in SHIPPED:
        assert sup(dims) == 1, dims
    assert sup((7, 1)) == 1 and sup((1, 1)) == 1 and sup((5, 3, 2)) == 1 and sup((128, 64, 32, 32)) == 1
    assert sup((0, 4)) == 0 and sup((4, 0)) == 0 and sup((4, 0, 4)) == 0           # width 0
    assert sup((128, 128)) == 1 and sup((129, 4)) == 0 and sup((4, 129)) == 0       # width 128 / 129
    assert sup((4,)) == 0                                                          # no Linear
    assert sup((4, 4, 4, 4, 4)) == 1 and sup((4, 4, 4, 4, 4, 4)) == 0               # four / five Linears
    assert lib.dgn_mlp_head_supported(3, None) == 0


def test_one_float_over_the_weight_limit_is_rejected(lib):
    sup = lambda dims: lib.dgn_mlp_head_supported(len(dims) - 1, _i32(dims))
    for at in ((128, 128, 32), (32, 128, 128), (1, 128, 128, 31), (128, 62, 128, 18, 128), (100, 100, 100, 4, 20)):
        assert _weights(at) == 20480 and sup(at) == 1, at
    one_more = (1, 1, 128, 128, 31)                                                # 1 + 128 + 16 384 + 3 968
    assert _weights(one_more) == 20481 and sup(one_more) == 0
    assert _weights((128, 128, 32, 1)) == 20512 and sup((128, 128, 32, 1)) == 0


def test_workspace_bytes(lib):
    wsb = lambda n, dims: lib.dgn_mlp_head_backward_workspace_bytes(n, len(dims) - 1, _i32(dims))
    for dims in SHIPPED:
        assert wsb(1000, dims) > 0 and wsb(0, dims) > 0, dims
    assert wsb(1000, (129, 4)) == 0 and wsb(1000, (4,)) == 0 and wsb(-1, SHIPPED[0]) == 0 and wsb(2 ** 31, SHIPPED[0]) == 0
    # one slot of sum_l d_l (d_{l-1} + 1) floats per workgroup, a workgroup per 32-row tile up to 256
    items = 23 * 48 + 11 * 24 + 2 * 12
    assert wsb(1, SHIPPED[1]) == items * 4 and wsb(33, SHIPPED[1]) == 2 * items * 4 and wsb(15361, SHIPPED[1]) == 256 * items * 4
    assert wsb(2 ** 31 - 1, SHIPPED[1]) == 256 * items * 4


def test_argument_checks_run_before_any_device_work(lib):
    from dgn_amd import _lib
    err = lambda: lib.dgn_last_error().decode()
    vp = C.c_void_p
    a = 1 << 12                                                                    # dummy pointer, never dereferenced
    dims = _i32((47, 23, 11, 2))
    ptrs, nulls = (vp * 3)(a, a, a), (vp * 3)(a, None, a)
    fwd, bwd = lib.dgn_mlp_head_forward, lib.dgn_mlp_head_backward
    assert fwd(0, 3, dims, None, 47, ptrs, ptrs, None, 2, None) == 0               # no row: nothing to do
    assert fwd(10, 3, _i32((47, 23, 11, 129)), a, 47, ptrs, ptrs, a, 129, None) == -1 and "dgn_mlp_head_supported" in err()
    assert fwd(10, 3, dims, a, 46, ptrs, ptrs, a, 2, None) == -1 and "row stride" in err()
    assert fwd(10, 3, dims, a, 47, ptrs, ptrs, a, 1, None) == -1 and "row stride" in err()
    assert fwd(10, 3, dims, None, 47, ptrs, ptrs, a, 2, None) == -1 and "null" in err()
    assert fwd(10, 3, dims, a, 47, nulls, ptrs, a, 2, None) == -1 and "null weight / bias 1" in err()
    assert fwd(10, 3, dims, a, 47, None, ptrs, a, 2, None) == -1 and "null" in err()
    assert fwd(2 ** 31, 3, dims, a, 47, ptrs, ptrs, a, 2, None) == -1 and "int32" in err()
    need = lib.dgn_mlp_head_backward_workspace_bytes(10, 3, dims)
    assert bwd(10, 3, dims, a, 47, ptrs, ptrs, a, 2, None, 47, ptrs, ptrs, a, need - 1, None) == -1 and "workspace" in err()
    assert bwd(10, 3, dims, a, 47, ptrs, ptrs, a, 2, None, 47, ptrs, ptrs, a + 2, need, None) == -1 and "workspace" in err()
    assert bwd(10, 3, dims, a, 47, ptrs, ptrs, a, 2, None, 47, ptrs, ptrs, None, need, None) == -1 and "workspace" in err()
    assert bwd(10, 3, dims, a, 47, ptrs, ptrs, a, 2, a, 46, ptrs, ptrs, a, need, None) == -1 and "row stride" in err()
    assert bwd(10, 3, dims, a, 47, ptrs, ptrs, a, 1, None, 47, ptrs, ptrs, a, need, None) == -1 and "row stride" in err()
    assert bwd(10, 3, dims, a, 47, ptrs, ptrs, None, 2, None, 47, ptrs, ptrs, a, need, None) == -1 and "null" in err()
    assert bwd(10, 3, dims, a, 47, ptrs, ptrs, a, 2, None, 47, nulls, ptrs, a, need, None) == -1 and "gradient 1" in err()
    assert bwd(10, 3, dims, a, 47, ptrs, ptrs, a, 2, None, 47, None, ptrs, a, need, None) == -1 and "null" in err()
    assert "dgn_mlp_head_forward" in _lib.EXPORTS


def test_python_side_on_cpu_tensors():
    import dgn_amd
    from dgn_amd import ops
    from dgn_amd.nets import MLPReadout
    assert ops.FUSED_MLP_HEAD is (os.environ.get("DGN_FUSED_MLP_HEAD", "1") != "0") and dgn_amd.mlp_head is ops.mlp_head
    torch.manual_seed(0)
    m = MLPReadout(47, 2)
    x = torch.randn(65, 47, requires_grad=True)
    ws = [fc.weight for fc in m.FC_layers]
    assert not ops.mlp_head_supported(x, ws)                                       # CPU tensors: torch's route
    y = m(x)
    ref = x
    for fc in m.FC_layers[:-1]:
        ref = torch.relu(torch.nn.functional.linear(ref, fc.weight, fc.bias))
    ref = torch.nn.functional.linear(ref, m.FC_layers[-1].weight, m.FC_layers[-1].bias)
    assert torch.equal(y, ref)
    y.sum().backward()
    assert x.grad is not None and all(fc.weight.grad is not None for fc in m.FC_layers)
    with pytest.raises(dgn_amd._lib.DgnError):
        ops.mlp_head(x, ws, [fc.bias for fc in m.FC_layers])
