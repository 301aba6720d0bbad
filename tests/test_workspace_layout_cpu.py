"""Every ``*_workspace_bytes`` / ``*_aux_bytes`` query of the multi-part workspaces, pinned without a GPU.

The host code of an entry point with a scratch buffer states its layout once (csrc/dgn_common.hpp: ``WsLayout``) and the exported query,
the size check and the carve read that one struct.  The numbers below are what the queries returned BEFORE the layouts had one
definition each (recorded from the previous library over this very grid): a layout function that moves a span or changes a total
shows up here.  The queries are host arithmetic over host structs -- the device pointers in them are never followed, so any non-null
address stands in -- and ``n_cus()`` answers 256 without a device, which is also the MI355X's count: the table holds on both machines.

``dgn_graph_build_workspace_bytes`` is the exception: its last span is what the hipCUB primitives ask for, which changes with the
device the library sees (measured: 512 bytes for an empty graph without a device, 1 024 on the MI355X).  It is checked against its own
layout, and against totals recorded on either kind of machine (``test_graph_build_blocks``).  Needs the built library, like
tests/test_abi.py."""
import ctypes as C
import os

import pytest

PTR = 0x1000      # a device address that is never followed


@pytest.fixture(scope="module")
def lib():
    from dgn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _graph(n_nodes, n_edges, hubs=0, chunks=0, csc=False):
    from dgn_amd import _lib
    g = _lib.DgnGraph()
    g.n_nodes, g.n_edges, g.indptr, g.src = n_nodes, n_edges, PTR, PTR
    if hubs:
        g.n_hub, g.n_chunks, g.hub_rows, g.hub_chunk_ptr, g.chunk_hub, g.hub_threshold, g.hub_chunk = hubs, chunks, PTR, PTR, PTR, 64, 32
    if csc:
        g.csc_ptr, g.csc_pos = PTR, PTR
    return g


def _spec(ops, chs, n_ch, towers=1, scalers=1):
    from dgn_amd import _lib
    s = _lib.DgnAggSpec()
    s.n_agg, s.n_ch, s.n_scalers, s.n_towers, s.avg_log, s.eps = len(ops), n_ch, scalers, towers, 1.0, 1e-5
    for i, (op, ch) in enumerate(zip(ops, chs)):
        s.agg_op[i], s.agg_ch[i] = op, ch
    return s


# aggregator lists: ZINC towers / complex (mean max min dir1-av dir1-dx [+ the h_in block]), the simple layer's (mean dir1-dx-no-abs), plain
MEAN, MAX, MIN, AV, DX, DXN, X_IN = 0, 2, 3, 6, 8, 9, 10
LISTS = {"zinc": ((MEAN, MAX, MIN, AV, DX), (0, 0, 0, 0, 0), 1), "zinc_h": ((MEAN, MAX, MIN, AV, DX, X_IN), (0, 0, 0, 0, 0, 0), 1),
         "c1": ((MEAN, DXN), (0, 0), 1), "c1_h": ((MEAN, DXN, X_IN), (0, 0, 0), 1), "plain": ((MEAN, MAX), (0, 0), 0),
         "two_ch": ((MEAN, DX, AV), (0, 0, 1), 2), "c3": ((MEAN, DX, DX), (0, 0, 1), 2)}
# graphs: n_nodes of 0, 1, 37 and above 131 072; hub rows present and absent; the transposed view present and absent; no edges
GRAPHS = {"n0": (0, 0, 0, 0, True), "n1": (1, 0, 0, 0, True), "n37": (37, 80, 0, 0, False), "n37_csc": (37, 80, 0, 0, True),
          "mol": (300, 640, 0, 0, True), "dense": (300, 2400, 0, 0, True), "hub": (300, 1200, 2, 5, True), "hub_nocsc": (300, 1200, 3, 7, False),
          "big": (140000, 300000, 0, 0, True), "big_hub": (140000, 600000, 4, 9, True)}


def _agg(lib):
    from dgn_amd import _lib
    out = {}
    for gn, ga in GRAPHS.items():
        g = _graph(*ga)
        out[f"edge_weights/{gn}"] = lib.dgn_edge_weights_workspace_bytes(C.byref(g), 2)
        for ln in ("zinc", "plain", "two_ch"):
            ops, chs, n_ch = LISTS[ln]
            for towers, F in ((1, 6), (1, 70), (1, 76), (5, 70)):
                s = _spec(ops, chs, n_ch, towers)
                key = f"{gn}/{ln}/T{towers}/F{F}"
                out[f"agg_fwd/{key}"] = lib.dgn_agg_workspace_bytes(C.byref(g), C.byref(s), F)
                for det in (0, 1):
                    out[f"agg_bwd/{key}/det{det}"] = lib.dgn_agg_backward_workspace_bytes(C.byref(g), C.byref(s), F, det)
        for ln in ("zinc", "c1", "plain", "two_ch", "c3"):
            ops, chs, n_ch = LISTS[ln]
            s = _spec(ops, chs, n_ch)
            for F, odd in ((70, 0), (76, 75), (7, 0)):
                m = _lib.DgnMsg()
                m.F, m.x_src, m.ld_src, m.x_in, m.ld_in, m.f_valid = F, PTR, F, PTR, F, odd
                out[f"agg_aux/{gn}/{ln}/F{F}/odd{odd}"] = lib.dgn_agg_aux_bytes(C.byref(g), C.byref(s), C.byref(m))
    for F, K in ((0, 4), (70, 0), (70, 4), (7, 3), (64, 5), (2048, 4)):
        out[f"edge_table/F{F}/K{K}"] = lib.dgn_agg_edge_table_workspace_bytes(F, K)
    return out


def _tails(lib):
    out = {}
    for n in (0, 1, 37, 4097, 131073, 300000):
        for F in (1, 70, 75, 256, 1024, 1025):
            out[f"bn_tail/n{n}/F{F}"] = lib.dgn_bn_tail_workspace_bytes(n, F)
    for units in (0, 1, 15, 257, 816, 5000):
        for k, n in ((280, 70), (350, 70), (304, 76), (96, 90), (2048, 128), (280, 130)):
            out[f"dc_wgrad/u{units}/k{k}/n{n}"] = lib.dgn_dc_wgrad_workspace_bytes(units, k, n)
    return out


def _towers(lib):
    from dgn_amd import _lib
    out = {}
    for gn in ("n0", "n1", "n37_csc", "mol", "hub", "hub_nocsc", "big"):
        g = _graph(*GRAPHS[gn])
        # (the last two: widths outside the towers kernels, every query 0)
        for T, fi, fo, S, ln in ((5, 14, 14, 3, "zinc_h"), (1, 14, 14, 3, "zinc_h"), (1, 18, 30, 1, "c1_h"), (2, 15, 14, 3, "zinc_h"), (5, 14, 10, 1, "c1_h"),
                                 (5, 14, 14, 2, "zinc"), (5, 16, 16, 3, "zinc_h"), (1, 70, 70, 3, "zinc_h")):
            ops, chs, n_ch = LISTS[ln]
            s = _spec(ops, chs, n_ch, T)
            L = _lib.DgnTowersLayer()
            L.graph, L.spec, L.n_towers, L.f_in, L.f_out, L.n_scalers = C.pointer(g), C.pointer(s), T, fi, fo, S
            key = f"{gn}/T{T}x{fi}-{fo}/S{S}/{ln}"
            out[f"towers_fwd/{key}"] = lib.dgn_towers_layer_forward_workspace_bytes(C.byref(L))
            out[f"towers_bwd/{key}"] = lib.dgn_towers_layer_backward_workspace_bytes(C.byref(L))
            out[f"towers_aux/{key}"] = lib.dgn_towers_layer_agg_aux_bytes(C.byref(L))
    return out


def _dense(lib):
    from dgn_amd import _lib
    out = {}
    for gn in ("n0", "n1", "n37_csc", "mol", "dense", "hub", "big"):
        g = _graph(*GRAPHS[gn])
        dc = _lib.DgnDegreeClasses()
        dc.n_units, dc.vperm, dc.unit_class, dc.present, dc.scale = (GRAPHS[gn][0] + 63) // 64 + 15, PTR, PTR, PTR, PTR
        for typ, f_in, f_out, S, ln in ((0, 75, 75, 3, "c1"), (0, 70, 70, 1, "c1"), (1, 70, 70, 3, "zinc_h"), (1, 65, 65, 3, "zinc_h"), (0, 45, 45, 2, "zinc"),
                                        (1, 47, 47, 1, "c1_h"), (0, 300, 200, 3, "c1")):
            ops, chs, n_ch = LISTS[ln]
            s = _spec(ops, chs, n_ch)
            for with_dc in (0, 1):
                L = _lib.DgnDenseLayer()
                L.graph, L.spec, L.type, L.f_in, L.f_out, L.n_scalers = C.pointer(g), C.pointer(s), typ, f_in, f_out, S
                L.n_agg = len(ops) - typ
                L.id_slot = 0
                if with_dc:
                    L.dc = C.pointer(dc)
                key = f"{gn}/type{typ}/{f_in}-{f_out}/S{S}/{ln}/dc{with_dc}"
                out[f"dense_fwd/{key}"] = lib.dgn_dense_layer_forward_workspace_bytes(C.byref(L))
                out[f"dense_bwd/{key}"] = lib.dgn_dense_layer_backward_workspace_bytes(C.byref(L))
                out[f"dense_aux/{key}"] = lib.dgn_dense_layer_agg_aux_bytes(C.byref(L))
    return out


def _block(lib):
    from dgn_amd import _lib
    out = {}
    ch = (_lib.DgnChannel * 2)()
    for N, n_blocks in ((0, 0), (1, 1), (37, 2), (3000, 128), (4097, 128), (8193, 300), (140000, 6000)):
        g = _graph(N, 2 * N, csc=True)
        t = _lib.DgnBlockTable()
        t.n_blocks, t.max_rows, t.max_edges, t.desc = n_blocks, 38, 90, PTR
        for typ, T, fi, fo, S, ln in ((0, 1, 75, 75, 3, "c1"), (1, 1, 70, 70, 3, "zinc"), (2, 5, 14, 14, 3, "zinc"), (2, 2, 9, 10, 1, "two_ch"), (0, 1, 70, 70, 1, "plain")):
            ops, chs, n_ch = LISTS[ln]
            s = _spec(ops, chs, n_ch, 1, S)
            L = _lib.DgnBlockLayer()
            L.graph, L.blocks, L.spec, L.channels, L.eig = C.pointer(g), C.pointer(t), C.pointer(s), ch, PTR
            L.type, L.n_towers, L.f_in, L.f_out = typ, T, fi, fo
            key = f"N{N}/type{typ}/T{T}x{fi}-{fo}/S{S}/{ln}"
            out[f"block_fwd/{key}"] = lib.dgn_block_layer_forward_workspace_bytes(C.byref(L))
            out[f"block_bwd/{key}"] = lib.dgn_block_layer_backward_workspace_bytes(C.byref(L))
    return out


FAMILIES = {"agg": _agg, "tails": _tails, "towers": _towers, "dense": _dense, "block": _block}


def record(lib):
    """{family: [bytes of every case, in the grid's order]} of this library (what EXPECTED was written from)"""
    return {name: list(fn(lib).values()) for name, fn in FAMILIES.items()}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_queries_return_the_recorded_bytes(lib, family):
    got, want = FAMILIES[family](lib), EXPECTED[family]
    assert len(got) == len(want)
    wrong = {k: (v, w) for (k, v), w in zip(got.items(), want) if v != w}
    assert not wrong, f"{len(wrong)} of {len(want)} queries changed (got, recorded), e.g. {dict(list(wrong.items())[:5])}"
    # every branch of the family is in the grid: some queries answer 0 (no workspace / unsupported), some do not
    assert any(w == 0 for w in want) and any(w > 0 for w in want)


def test_graph_build_blocks(lib):
    """four int32 arrays per edge (+ 1), four per node (+ 2), a byte per edge (+ 1), each rounded up to 256 bytes, then the primitives'
    storage, which depends on max(n_nodes + 2, n_edges) + 1 alone: two graphs with the same maximum differ by their named blocks"""
    up = lambda x: (x + 255) & ~255
    named = lambda n, e: 4 * up(4 * (e + 1)) + 4 * up(4 * (n + 2)) + up(e + 1)
    q = lib.dgn_graph_build_workspace_bytes
    for e, nodes in ((300, (0, 1, 37, 298)), (1200, (300, 1198, 5)), (0, (0,)), (300000, (140000, 299998, 1))):
        cub = {q(n, e) - named(n, e) for n in nodes}
        assert len(cub) == 1 and min(cub) > 0, (e, nodes, cub)
    # the node side decides the maximum: n_edges below n_nodes + 2
    assert q(140000, 20) - named(140000, 20) == q(140000, 139000) - named(140000, 139000) > 0
    # the primitives' share: what hipCUB asks for rounded up to 256, + 256 -- so a multiple of 256, and never less than 256
    for n, e in BUILD_RECORDED[False]:
        assert (q(n, e) - named(n, e)) % 256 == 0 and q(n, e) - named(n, e) >= 256, (n, e)
    # ... and the totals as recorded from the previous library: hipCUB sizes its storage by the device it sees, so there is one
    # set for a machine without a device and one for the MI355X
    import torch
    assert {k: q(*k) for k in BUILD_RECORDED[False]} == BUILD_RECORDED[torch.cuda.is_available()]


BUILD_RECORDED = {False: {(0, 0): 2816, (37, 20): 2816, (300, 1200): 26112, (140000, 20): 2242048, (140000, 300000): 7341312},
                  True: {(0, 0): 3328, (37, 20): 3328, (300, 1200): 35840, (140000, 20): 3362304, (140000, 300000): 9742592}}


# the recorded table: per family, the bytes of every case in the order its function above walks the grid
EXPECTED = {
    "agg": [
        0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 512, 512,
        0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 512, 512, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        0, 0, 0, 0, 0, 2816, 3072, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2816, 3072, 0, 0, 0, 0, 2048, 0, 0, 22528, 0, 0, 24320, 0, 0, 22528, 0, 0, 2048,
        0, 0, 22528, 0, 0, 24320, 0, 0, 22528, 0, 0, 2048, 0, 0, 22528, 0, 0, 24320, 0, 0, 22528, 2816, 3072, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2816,
        3072, 0, 0, 0, 0, 15360, 0, 0, 179200, 0, 0, 194560, 0, 0, 179200, 0, 0, 15360, 0, 0, 179200, 0, 0, 194560, 0, 0, 179200, 0, 0, 15360, 0,
        0, 179200, 0, 0, 194560, 0, 0, 179200, 21248, 23040, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 21248, 23040, 0, 0, 0, 0, 57600, 0, 0, 672000, 0, 0,
        729600, 0, 0, 672000, 0, 0, 57600, 0, 0, 672000, 0, 0, 729600, 0, 0, 672000, 0, 0, 57600, 0, 0, 672000, 0, 0, 729600, 0, 0, 672000, 0, 0,
        0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 21248, 23040, 2304, 768, 1792, 1792, 30720, 16128, 16128, 352256, 17408, 17408, 382208, 16128, 16128, 352256,
        1536, 1536, 30464, 12288, 12288, 348416, 13312, 13312, 378112, 12288, 12288, 348416, 2048, 2048, 30976, 19968, 19968, 356096, 21760, 21760,
        386560, 19968, 19968, 356096, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1024, 2560, 2560, 2560, 23040, 23040, 23040, 24832, 24832,
        24832, 23040, 23040, 23040, 1792, 1792, 1792, 17152, 17152, 17152, 18688, 18688, 18688, 17152, 17152, 17152, 2816, 2816, 2816, 28416,
        28416, 28416, 30976, 30976, 30976, 28416, 28416, 28416, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7200000, 0, 0, 84000000, 0,
        0, 91200000, 0, 0, 84000000, 0, 0, 7200000, 0, 0, 84000000, 0, 0, 91200000, 0, 0, 84000000, 0, 0, 7200000, 0, 0, 84000000, 0, 0, 91200000,
        0, 0, 84000000, 9800192, 10640128, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 9800192, 10640128, 0, 1280, 2816, 2816, 14402816, 29440, 29440, 168029440,
        32000, 32000, 182432000, 29440, 29440, 168029440, 2560, 2560, 14402560, 22528, 22528, 168022528, 24320, 24320, 182424320, 22528, 22528,
        168022528, 3584, 3584, 14403584, 36864, 36864, 168036864, 39936, 39936, 182439936, 36864, 36864, 168036864, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        0, 0, 0, 0, 0, 0, 0, 573440, 43008, 655360, 16777216,
    ],
    "tails": [
        0, 0, 0, 0, 0, 0, 24, 1680, 1800, 6144, 24576, 0, 24, 2800, 3000, 22528, 90112, 0, 56, 192080, 205800, 2103296, 8413184, 0, 1048, 2294320,
        2458200, 8390656, 33562624, 0, 2360, 2294320, 2458200, 8390656, 33562624, 0, 0, 0, 0, 0, 0, 0, 3041540, 3717380, 3210500, 1216772,
        34603268, 0, 4331836, 5294396, 4572476, 1732924, 49283388, 0, 14838532, 18135812, 15662852, 5935876, 63963508, 0, 21750832, 26584112,
        22959152, 8700976, 67109248, 0, 25990376, 31765736, 27434216, 10396904, 67109248, 0,
    ],
    "towers": [
        9175040, 21504, 0, 1835008, 1536, 0, 3932160, 4352, 0, 3670016, 4096, 0, 6553600, 11008, 0, 9175040, 21248, 0, 0, 0, 0, 0, 0, 0, 9175040,
        192768, 512, 1835008, 25856, 256, 3932160, 25600, 0, 3670016, 56576, 256, 6553600, 93952, 0, 9175040, 151296, 512, 0, 0, 0, 0, 0, 0,
        9175040, 346880, 2816, 1835008, 56832, 768, 3932160, 62720, 0, 3670016, 122112, 1280, 6553600, 208384, 0, 9175040, 295424, 2816, 0, 0, 0,
        0, 0, 0, 9175040, 2131456, 21248, 1835008, 365824, 4352, 3932160, 406784, 0, 3670016, 792320, 9216, 6553600, 1357568, 0, 9175040, 1842432,
        21248, 0, 0, 0, 0, 0, 0, 9191168, 2304512, 0, 1838592, 400896, 0, 3936768, 451840, 0, 3677184, 866816, 0, 6569728, 1530624, 0, 9191168,
        2015488, 0, 0, 0, 0, 0, 0, 0, 9198080, 1975296, 0, 1840128, 335104, 0, 3938304, 366848, 0, 3680256, 725760, 0, 6576640, 1201408, 0,
        9198080, 1686272, 0, 0, 0, 0, 0, 0, 0, 9175040, 630793472, 9800192, 1835008, 130064384, 1960192, 3932160, 153230592, 0, 3670016, 267873792,
        4200192, 6553600, 466211328, 0, 9175040, 587415296, 9800192, 0, 0, 0, 0, 0, 0,
    ],
    "dense": [
        2457600, 137728, 0, 1238528, 2544640, 0, 2293760, 40192, 0, 2293760, 40192, 0, 2293760, 393984, 0, 1155840, 6891776, 0, 2129920, 345600, 0,
        1073408, 6362112, 0, 1474560, 83456, 0, 743168, 2249728, 0, 1540096, 46592, 0, 1540096, 46592, 0, 6553600, 1441792, 0, 6553600, 1441792, 0,
        2458624, 306432, 0, 1238528, 2600704, 0, 2294272, 105728, 0, 2294272, 105728, 0, 2294784, 802304, 512, 1155840, 7036928, 512, 2130944,
        753920, 512, 1073408, 6497024, 512, 1475072, 185088, 256, 743168, 2299136, 256, 1540352, 91136, 0, 1540352, 91136, 0, 6556160, 3260416, 0,
        6556160, 3260416, 0, 2491136, 724736, 0, 1238528, 2691328, 0, 2304256, 292352, 0, 2304256, 292352, 0, 2324992, 1759488, 2816, 1155840,
        7191296, 2816, 2158848, 1701888, 2816, 1073408, 6642176, 2816, 1488128, 449536, 2048, 743168, 2366976, 2048, 1547264, 243968, 0, 1547264,
        243968, 0, 6642432, 7198464, 0, 6642432, 7198464, 0, 2727680, 4008704, 0, 1238528, 3558656, 0, 2377984, 1741568, 0, 2377984, 1741568, 0,
        2545920, 9310976, 21248, 1155840, 8873216, 21248, 2364160, 9185024, 19968, 1073408, 8214784, 19968, 1582592, 2516736, 13824, 743168,
        3045632, 13824, 1596672, 1415936, 0, 1596672, 1415936, 0, 7273728, 38462208, 0, 7273728, 38462208, 0, 2727680, 4543744, 0, 1238528,
        4093696, 0, 2377984, 2234368, 0, 2377984, 2234368, 0, 2545920, 9803776, 0, 1155840, 9366016, 0, 2364160, 9649664, 0, 1073408, 8679424, 0,
        1582592, 2840576, 0, 743168, 3369472, 0, 1596672, 1753856, 0, 1596672, 1753856, 0, 7273728, 40574208, 0, 7273728, 40574208, 0, 2745088,
        4196352, 0, 1255936, 3746304, 0, 2394112, 1914624, 0, 2394112, 1914624, 0, 2562048, 9484032, 0, 1171968, 9046272, 0, 2379520, 9348352, 0,
        1088768, 8378112, 0, 1593344, 2630656, 0, 753920, 3159552, 0, 1607680, 1534464, 0, 1607680, 1534464, 0, 7341312, 39201792, 0, 7341312,
        39201792, 0, 128458496, 390033664, 0, 2458368, 362274304, 0, 41494528, 259436800, 0, 41494528, 259436800, 0, 119894528, 699622400, 9800192,
        2294528, 635155712, 9800192, 111330816, 649613568, 9240064, 2130688, 596466176, 9240064, 51875072, 287252992, 6440192, 1475072, 274852608,
        6440192, 27860736, 284538112, 0, 27860736, 284538112, 0, 342555392, 1260212992, 0, 342555392, 1260212992, 0,
    ],
    "block": [
        0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1280, 137216, 1280, 355328, 1280, 92928, 512, 6912, 1280, 41472, 2560, 285952, 2304, 720896, 2304, 216064,
        768, 17920, 2304, 93184, 153600, 18444288, 143360, 46280960, 143360, 13891840, 40960, 1170176, 143360, 6104320, 153600, 18702592, 143360,
        46522112, 143360, 12960000, 40960, 1140224, 143360, 6345472, 360192, 43203072, 336128, 108446976, 336128, 26339584, 96000, 2212352, 336128,
        14283008, 7200000, 856425984, 6720000, 2161810688, 6720000, 511868160, 1920000, 41544192, 6720000, 278530816,
    ],
}
