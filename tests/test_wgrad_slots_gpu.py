"""The slot loop of the weight-gradient finalize kernels at its boundaries, through the C ABI on the GPU.

Every weight-gradient family leaves one partial block per workgroup in a workspace slot and a finalize kernel adds the slots in a fixed
order.  The shared slot sum has three code paths -- pairs of sixteen slots, the odd remainder, fewer than sixteen slots -- so every
entry point runs at 1, 15, 16, 17, 31, 32 and 33 slots, plus one ragged case whose last 16-row strip is partly filled.  The row counts
come from each family's plan ("strips of 16 rows, at most a multiple of the CU count"); each test asserts the slot count it meant to
reach where the library lets it be read back.  Inputs are integers from {-2 .. 2}: every partial sum is an integer far below 2^24,
exact in fp32 in any order, so the results must EQUAL the fp64 product, and two calls must give identical bytes."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

SLOTS = (1, 15, 16, 17, 31, 32, 33)


def _ints(gen, *shape):
    return torch.randint(-2, 3, shape, device="cuda", generator=gen).float()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _twice(call, *outs):
    """Run ``call`` twice into NaN-filled outputs: the first results, after asserting the second are the same bytes."""
    res = []
    for _ in range(2):
        for o in outs:
            o.fill_(float("nan"))
        call()
        res.append([o.clone() for o in outs])
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    return res[0]


# dgn_linear_wgrad (wgrad_groups) and dgn_linear_bd_wgrad (bd_wgrad_groups): four waves of one strip each per workgroup,
# groups = ceil(strips / 4) while that is below the CU count
LIN_ROWS = [(64, 1),       # 4 strips    -> 1 slot
            (960, 15),     # 60 strips   -> 15 slots
            (1024, 16),    # 64 strips   -> 16 slots
            (1088, 17),    # 68 strips   -> 17 slots
            (1984, 31),    # 124 strips  -> 31 slots
            (2048, 32),    # 128 strips  -> 32 slots
            (2112, 33),    # 132 strips  -> 33 slots
            (1045, 17)]    # 66 strips   -> 17 slots; the last strip has 5 rows, the last workgroup two waves without a strip


@pytest.mark.parametrize("k,n", [(6, 10), (70, 70)])
@pytest.mark.parametrize("M,slots", LIN_ROWS)
def test_linear_wgrad_slot_counts(M, slots, k, n):
    from dgn_amd import _lib
    lib = _lib.load()
    gen = torch.Generator(device="cuda").manual_seed(M + k)
    g, x = _ints(gen, M, n), _ints(gen, M, k)
    nb = lib.dgn_linear_wgrad_workspace_bytes(M, k, n, 1)
    assert nb == slots * ((n + 15) // 16 * 16) * ((k + 15) // 16 * 16) * 4             # one padded block per slot
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dw, db = torch.empty(n, k, device="cuda"), torch.empty(n, device="cuda")
    st = _lib.stream_ptr(x.device)
    dw, db = _twice(lambda: _lib.check(lib.dgn_linear_wgrad(M, k, n, 1, g.data_ptr(), n, 0, x.data_ptr(), k, 0, dw.data_ptr(), k, 0, db.data_ptr(), 0,
                                                            ws.data_ptr(), nb, st), "dgn_linear_wgrad"), dw, db)
    assert torch.equal(dw.double(), g.double().t() @ x.double())
    assert torch.equal(db.double(), g.double().sum(0))


@pytest.mark.parametrize("M,slots", LIN_ROWS)
def test_linear_bd_wgrad_slot_counts(M, slots):
    from dgn_amd import _lib
    lib = _lib.load()
    T, fi = 5, 14
    Fm = T * fi
    assert lib.dgn_linear_bd_supported(T, fi)
    gen = torch.Generator(device="cuda").manual_seed(M)
    g, x = _ints(gen, M, 2 * Fm), _ints(gen, M, Fm)
    nb = lib.dgn_linear_bd_wgrad_workspace_bytes(M, T, fi)
    assert nb == slots * 2 * T * 256 * 4                                               # 2 T tiles of 16 x 16 per slot
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dw, db = torch.empty(2 * Fm, Fm, device="cuda"), torch.empty(2 * Fm, device="cuda")
    st = _lib.stream_ptr(x.device)
    dw, db = _twice(lambda: _lib.check(lib.dgn_linear_bd_wgrad(M, T, fi, g.data_ptr(), x.data_ptr(), dw.data_ptr(), Fm, db.data_ptr(), ws.data_ptr(), nb, st),
                                       "dgn_linear_bd_wgrad"), dw, db)
    # the towers' diagonal blocks of g^T x, zero elsewhere: row j Fm + t fi + a against the columns t fi .. t fi + fi - 1
    tower_r = (torch.arange(2 * Fm, device="cuda") % Fm) // fi
    tower_c = torch.arange(Fm, device="cuda") // fi
    ref = (g.double().t() @ x.double()) * (tower_r[:, None] == tower_c[None, :])
    assert torch.equal(dw.double(), ref)
    assert torch.equal(db.double(), g.double().sum(0))


# dgn_gemm_wgrad, strip kernel (wgrad_plan) and tile kernel (tile_wgrad_plan; one block of tiles at these widths): the strips are dealt
# round-robin to min(strips, CU count) workgroups
GEMM_ROWS = [(16, 1),      # 1 strip     -> 1 slot
             (240, 15),    # 15 strips   -> 15 slots
             (256, 16),    # 16 strips   -> 16 slots
             (272, 17),    # 17 strips   -> 17 slots
             (496, 31),    # 31 strips   -> 31 slots
             (512, 32),    # 32 strips   -> 32 slots
             (528, 33),    # 33 strips   -> 33 slots
             (263, 17)]    # 17 strips   -> 17 slots; the last strip has 7 rows


@pytest.mark.parametrize("tile", [0, 1])        # option tile_wgrad: 0 the strip kernel, 1 the tile kernel
@pytest.mark.parametrize("k,n", [(7, 5), (75, 75)])
@pytest.mark.parametrize("M,slots", GEMM_ROWS)
def test_gemm_wgrad_slot_counts(monkeypatch, M, slots, k, n, tile):
    from dgn_amd import _lib
    lib = _lib.load()
    assert min((M + 15) // 16, _cus()) == slots
    monkeypatch.setattr(_lib.options, "tile_wgrad", tile)
    gen = torch.Generator(device="cuda").manual_seed(M + k)
    g, x = _ints(gen, M, n), _ints(gen, M, k)
    nb = lib.dgn_gemm_wgrad_workspace_bytes(M, k, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dw, db = torch.empty(n, k, device="cuda"), torch.empty(n, device="cuda")
    st = _lib.stream_ptr(x.device)
    dw, db = _twice(lambda: _lib.check(lib.dgn_gemm_wgrad(M, k, n, g.data_ptr(), n, x.data_ptr(), k, dw.data_ptr(), k, db.data_ptr(), ws.data_ptr(), nb, st),
                                       "dgn_gemm_wgrad"), dw, db)
    assert torch.equal(dw.double(), g.double().t() @ x.double())
    assert torch.equal(db.double(), g.double().sum(0))


# dgn_dc_wgrad (dc::wgrad_plan): one workgroup per unit of 64 virtual rows while the units are fewer than the CUs; in-degree classes 1
# and 2, each padded to whole units.  (units of class 1, nodes of class 1, units of class 2, nodes of class 2)
DC_NODES = [((1, 64, 0, 0), 1),
            ((7, 448, 8, 512), 15),
            ((8, 512, 8, 512), 16),
            ((8, 512, 9, 576), 17),
            ((15, 960, 16, 1024), 31),
            ((16, 1024, 16, 1024), 32),
            ((16, 1024, 17, 1088), 33),
            ((8, 490, 9, 547), 17)]     # class 1 ends with 42 rows of a unit, class 2 with 35: strips of 16, 16, 3 rows and an empty one


@pytest.mark.parametrize("nodes,slots", DC_NODES)
def test_dc_wgrad_slot_counts(nodes, slots):
    import dgn_amd
    from dgn_amd import _lib
    lib = _lib.load()
    k, n, S = 46, 45, 2
    _, n1, _, n2 = nodes
    N = n1 + n2
    cpu = torch.Generator().manual_seed(N)
    deg = torch.cat([torch.ones(n1, dtype=torch.long), torch.full((n2,), 2, dtype=torch.long)])[torch.randperm(N, generator=cpu)]
    dst = torch.repeat_interleave(torch.arange(N), deg)
    src = torch.randint(0, N, (dst.numel(),), generator=cpu)
    graph = dgn_amd.DGNGraph(src.cuda(), dst.cuda(), N)
    dc = graph.degree_classes()
    assert dc["n_units"] == slots == nodes[0] + nodes[2] and slots <= _cus()
    gen = torch.Generator(device="cuda").manual_seed(N)
    g, x = _ints(gen, N, n), _ints(gen, N, k)
    scale = torch.randint(1, 3, (32, S), device="cuda", generator=gen).float()
    s = _lib.DgnDegreeClasses(n_units=dc["n_units"], vperm=dc["vperm"].data_ptr(), unit_class=dc["unit_class"].data_ptr(),
                              present=dc["present"].data_ptr(), scale=scale.data_ptr())
    nb = lib.dgn_dc_wgrad_workspace_bytes(dc["n_units"], k, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    out = torch.empty(S * n, k, device="cuda")
    st = _lib.stream_ptr(x.device)
    out, = _twice(lambda: _lib.check(lib.dgn_dc_wgrad(C.byref(s), S, k, n, g.data_ptr(), n, x.data_ptr(), k, out.data_ptr(), k, None, ws.data_ptr(), nb, st),
                                     "dgn_dc_wgrad"), out)
    sc = scale.double()[deg.cuda()]                                                    # [N, S]
    ref = torch.cat([(g.double() * sc[:, j:j + 1]).t() @ x.double() for j in range(S)], 0)
    assert torch.equal(out.double(), ref)
