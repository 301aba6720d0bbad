"""CPU-side checks of the drop-in boundary: the C-ABI library builds/loads and exports every symbol
include/dgn_hip.h declares (no compute without a GPU), the ctypes structs match the header's layout,
and the product path refuses to run without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from dgn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_header_symbols_are_exported(lib):
    from dgn_amd import _lib
    header = open(os.path.join(ROOT, "include", "dgn_hip.h")).read()
    declared = set(re.findall(r"\b(dgn_[a-z_]+)\s*\(", header))
    assert declared == set(_lib.EXPORTS)
    for sym in declared:
        assert getattr(lib, sym) is not None
    assert lib.dgn_abi_version() == _lib.ABI_VERSION
    # no function is left on ctypes' defaults: argtypes are set, as many as the prototype has parameters by this test's own regex
    protos = dict(re.findall(r"\b(dgn_[a-z_]+)\s*\(([^()]*)\)\s*;", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))
    assert list(protos) == list(_lib.EXPORTS)                       # header order
    for sym, params in protos.items():
        argtypes = getattr(lib, sym).argtypes
        assert argtypes is not None and len(argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), sym


def test_struct_layouts_match_header(lib):
    from dgn_amd import _lib
    # every struct the binding derived against the sizeof the LIBRARY was compiled with (dgn_sizeof; 0 for a struct the header has and
    # dgn_sizeof forgot), then a few sizes spelled out for LP64
    header = open(os.path.join(ROOT, "include", "dgn_hip.h")).read()
    structs = {name: t for name, t in vars(_lib).items() if isinstance(t, type) and issubclass(t, C.Structure)}
    assert set(structs) == set(re.findall(r"typedef\s+struct\s+(\w+)", header)) and len(structs) >= 15
    for name, t in structs.items():
        assert C.sizeof(t) == lib.dgn_sizeof(name.encode()) > 0, name
    assert lib.dgn_sizeof(b"NoSuchStruct") == 0
    assert C.sizeof(_lib.DgnChannel) == 16
    assert C.sizeof(_lib.DgnGraph) == 8 * 9 + 4 * 2 + 8 * 2 + 8 + 8 + 8 + 8 + 8 + 8 * 5       # (+ max_in_degree padded, n_src, row_base, blk_cut, blk_gap padded; gblk_desc, n_gblk, gblk_rows padded, csc_order, dst_csr)
    assert C.sizeof(_lib.DgnAggSpec) == 4 * (1 + 16 + 16 + 1 + 1 + 4 + 1 + 1 + 1 + 1 + 1) + 8
    assert C.sizeof(_lib.DgnMsg) == 8 * 9 + 8 + 8                               # (+ edge_type, n_edge_types padded)
    assert C.sizeof(_lib.DgnMsgGrad) == 8 * 8 + 8                                # (+ accumulate, padded)
    assert f"#define DGN_MAX_AGG {_lib.DGN_MAX_AGG}" in header
    assert f"#define DGN_MAX_CH {_lib.DGN_MAX_CH}" in header
    assert f"#define DGN_MAX_SCALERS {_lib.DGN_MAX_SCALERS}" in header


_MINI = """
/* a comment with a prototype inside: int dgn_not_real(int x); */
#ifndef MINI_H
#define MINI_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define DGN_N 3   /* array length */
enum { DGN_A = 0, DGN_B = -2 };
enum {
    DGN_C = 7    /* the last enumerator has no comma */
};
typedef struct DgnInner { int32_t a, b, c[DGN_N]; float x, y; } DgnInner;
typedef struct DgnOuter {
    const DgnInner* inner;      /* a struct pointer */
    const float* const* tables; float* out; int64_t ld;   /* several fields on one line */
    uint64_t offset; size_t bytes; unsigned char* mask; int64_t pad[2];
} DgnOuter;
const char* dgn_text(void);
size_t dgn_bytes(const DgnOuter* o, uint64_t offset,
                 const float* const* tables, const char* name, double* val, int k, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* MINI_H */
"""


def test_header_parser_reads_every_construct_of_the_header():
    from dgn_amd import _cabi
    h = _cabi.parse(_MINI)
    assert h.constants == {"DGN_N": 3, "DGN_A": 0, "DGN_B": -2, "DGN_C": 7}
    inner, outer = h.structs["DgnInner"], h.structs["DgnOuter"]
    assert list(h.structs) == ["DgnInner", "DgnOuter"] and issubclass(outer, C.Structure)
    assert inner._fields_ == [("a", C.c_int32), ("b", C.c_int32), ("c", C.c_int32 * 3), ("x", C.c_float), ("y", C.c_float)]      # multi-declarator, #define-sized array
    assert outer._fields_ == [("inner", C.POINTER(inner)), ("tables", C.POINTER(C.c_void_p)), ("out", C.c_void_p), ("ld", C.c_int64),
                              ("offset", C.c_uint64), ("bytes", C.c_size_t), ("mask", C.c_void_p), ("pad", C.c_int64 * 2)]
    assert C.sizeof(inner) == 28 and C.sizeof(outer) == 8 * 9
    assert list(h.prototypes) == ["dgn_text", "dgn_bytes"]                                      # the one inside the comment is no declaration
    assert h.prototypes["dgn_text"] == (C.c_char_p, [])
    assert h.prototypes["dgn_bytes"] == (C.c_size_t, [C.POINTER(outer), C.c_uint64, C.POINTER(C.c_void_p), C.c_char_p, C.c_void_p, C.c_int, C.c_void_p])


@pytest.mark.parametrize("text", [
    "int dgn_f(int128_t x);",                                            # unknown type
    "typedef struct DgnS { bool flag; } DgnS;",                          # ... in a field
    "long dgn_f(void);",                                                 # ... as the result
    "int dgn_f(const DgnNowhere* p);",                                   # pointer to an undeclared struct
    "typedef struct DgnS { const DgnNowhere* p; } DgnS;",
    "int dgn_f(DgnS s);\ntypedef struct DgnS { int a; } DgnS;",          # ... declared only later; and by value
    "int dgn_global;",                                                   # stray declarations
    "struct DgnS;",
    "typedef int32_t dgn_index;",
    "static inline int dgn_f(int x) { return x; }",
    "#define DGN_F(x) (x)",
    "#define DGN_HALF 0.5",
    "#include <stdio.h>",
    "// a C++ comment",
    "}",
    "enum { DGN_A, DGN_B };",                                            # enumerators without values
    "typedef struct DgnS { int a; } DgnT;",                              # two names
    "typedef struct DgnS { int a[DGN_UNKNOWN]; } DgnS;",                 # array length that is no #define
    "typedef struct DgnS { float *a, *b; } DgnS;",                       # pointer declarators sharing a type
    "typedef struct DgnS { int a : 3; } DgnS;",                          # bit field
    "int dgn_f(int32_t);",                                               # parameter without a name
    "int dgn_f(int32_t dims[4]);",                                       # array parameter
    "int dgn_f(float*** p);",
    "int dgn_f(int x)",                                                  # no semicolon
])
def test_header_parser_raises_on_what_it_does_not_understand(text):
    from dgn_amd import _cabi
    with pytest.raises(ValueError, match="dgn_hip.h"):
        _cabi.parse("#define DGN_N 3\n" + text + "\nint dgn_after(void);\n")


def test_missing_header_is_an_error():
    from dgn_amd import _lib
    missing = os.path.join(ROOT, "include", "no_such_header.h")
    with pytest.raises(_lib.DgnError, match="no_such_header.h"):
        _lib.read_abi(missing)


def test_argument_validation_without_gpu(lib):
    """Validation errors are reported before anything touches the device."""
    from dgn_amd import _lib
    g = _lib.DgnGraph()
    g.n_nodes, g.n_edges = 4, 0
    spec = _lib.DgnAggSpec()
    spec.n_agg = 0
    msg = _lib.DgnMsg()
    rc = lib.dgn_agg_forward(C.byref(g), C.byref(spec), C.byref(msg), None, 0, None, None, 0, None, 0, None)
    assert rc == -1 and b"null CSR" in lib.dgn_last_error()
    assert lib.dgn_agg_workspace_bytes(C.byref(g), C.byref(spec), 8) == 0
    rc = lib.dgn_edge_weights(C.byref(g), None, None, None, 4, 1, None, None, 0, None, 0, None)
    assert rc == -1


def test_edge_weight_route_switches_are_library_options(lib):
    """ew_big_min / ew_separate / ew_no_flat8 (DGN_EW_BIG_MIN, DGN_EW_SEPARATE, DGN_EW_NO_FLAT8) sit in the option table: read per call of
    dgn_edge_weights, so a test can flip them (tests/test_edge_weights_gpu.py does) and gets the defaults back."""
    from dgn_amd import _lib
    for name, env, default in (("ew_big_min", "DGN_EW_BIG_MIN", 1 << 19), ("ew_separate", "DGN_EW_SEPARATE", 0), ("ew_no_flat8", "DGN_EW_NO_FLAT8", 0)):
        if env in os.environ:
            continue                                            # (the caller's environment chose a route: its value is the process's default)
        assert lib.dgn_get_option(name.encode()) == default, name
        assert lib.dgn_set_option(name.encode(), 7) == 0 and getattr(_lib.options, name) == 7
        setattr(_lib.options, name, default)
        assert lib.dgn_get_option(name.encode()) == default
    assert lib.dgn_get_option(b"ew_no_such_switch") == -2 ** 63 and lib.dgn_set_option(b"ew_no_such_switch", 1) == -1


def test_plan_and_registry():
    import dgn_amd
    from dgn_amd import spec
    assert len(dgn_amd.AGGREGATOR_NAMES) == 24 and len(dgn_amd.SCALER_NAMES) == 3
    plan = dgn_amd.make_plan("mean max dir1-dx dir1-av dir1-dx-balanced".split(), ["amplification"])
    assert plan.applied_scalers == (spec.SCALE_IDENTITY,)          # lone scaler is not applied
    assert plan.n_channels == 2 and plan.launches[0].chs == [0, 0, 0, 0, 1]
    many = dgn_amd.make_plan(list(dgn_amd.AGGREGATOR_NAMES), ["identity", "attenuation"])
    assert sum(len(l.ops) for l in many.launches) == 24
    assert all(len(l.channels) <= 4 and len(l.ops) <= 16 for l in many.launches)
    assert dgn_amd.AGGREGATORS["dir2-smooth"].name == "dir2-smooth"
    with pytest.raises(KeyError):
        dgn_amd.AGGREGATORS["dir4-dx"]
    with pytest.raises(KeyError):
        dgn_amd.SCALERS["linear"]


def test_state_dict_layout_matches_reference(golden):
    """Same keys and shapes as the reference layers' state_dict (fixtures hold the reference's)."""
    import dgn_amd
    g = golden("g4_layers")
    for name in g["cases"].tolist():
        meta = g[f"{name}/meta"].tolist()
        layer = dgn_amd.DGNLayer(in_dim=int(meta[1]), out_dim=int(meta[2]), dropout=0.0, graph_norm=True, batch_norm=True,
                                 aggregators=meta[3], scalers=meta[4], avg_d={"log": torch.tensor(float(meta[5]))},
                                 type_net=meta[0], residual=True, towers=int(meta[6]), divide_input=bool(int(meta[7])),
                                 edge_features=bool(int(meta[8])), edge_dim=int(meta[9]), pretrans_layers=int(meta[10]),
                                 posttrans_layers=int(meta[11])).model
        ref = {k[len(name) + 5:]: g[k].shape for k in g.files if k.startswith(f"{name}/sd::")}
        mine = {k: tuple(v.shape) for k, v in layer.state_dict().items()}
        assert mine == {k: tuple(v) for k, v in ref.items()}, name


def test_fresh_init_matches_reference_under_seed(golden):
    """FCLayer init (xavier_uniform gain 1/in_size, zero bias; layers.py:94-99) under the same seed."""
    import dgn_amd
    g = golden("g4_layers")
    name = "simple_fresh_init"
    torch.manual_seed(0)
    layer = dgn_amd.DGNLayer(10, 10, 0.0, True, True, "mean dir1-dx", "identity", {"log": torch.tensor(1.1)}, "simple", True).model
    for k, v in layer.state_dict().items():
        assert torch.equal(v, torch.from_numpy(g[f"{name}/sd::{k}"])), k


def test_no_cpu_fallback():
    import dgn_amd
    from dgn_amd.ops import directional_aggregate
    src = torch.tensor([0, 1])
    with pytest.raises((dgn_amd._lib.DgnError, RuntimeError, AssertionError)):
        g = dgn_amd.DGNGraph(src, src.flip(0), 2, eig=torch.randn(2, 2))
        directional_aggregate(g, dgn_amd.make_plan(["mean"], ["identity"]), 1.0, x_src=torch.randn(2, 4))


def test_argument_validation_runs_before_any_device_work(lib):
    """Maximum sizes and malformed arguments are rejected by the host-side checks with an error code and a message
    (no kernel is launched, so this runs without a GPU): int32 CSR range, widths over the kernels' limits, nulls."""
    from dgn_amd import _lib
    err = lambda: lib.dgn_last_error().decode()
    g = _lib.DgnGraph()
    g.n_nodes, g.n_edges = 2 ** 31, 10                      # beyond the int32 CSR range
    spec, msg = _lib.DgnAggSpec(), _lib.DgnMsg()
    spec.n_agg, spec.n_scalers, spec.n_towers, spec.eps = 1, 1, 1, 1e-8
    msg.F, msg.x_src, msg.ld_src = 4, 1, 4                  # (a non-null dummy pointer: never dereferenced)
    rc = lib.dgn_agg_forward(C.byref(g), C.byref(spec), C.byref(msg), None, 0, None, None, 0, None, 0, None)
    assert rc == -1 and "int32" in err()
    g.n_nodes = 10
    rc = lib.dgn_agg_forward(C.byref(g), C.byref(spec), C.byref(msg), None, 0, None, None, 0, None, 0, None)
    assert rc == -1 and "null CSR" in err()
    g.indptr = g.src = 1                                    # (dummies again)
    spec.n_agg = 99                                         # more aggregators than one launch takes
    rc = lib.dgn_agg_forward(C.byref(g), C.byref(spec), C.byref(msg), None, 0, None, None, 0, None, 0, None)
    assert rc == -1 and "n_agg" in err()
    assert lib.dgn_bn_tail_forward(5, 2000, None, 2000, None, None, None, None, 0.1, 1e-5, 1, 0, None, None, None, None, None, 0, None, None) == -1
    assert "F <= 1024" in err()
    assert lib.dgn_scale_combine_forward(5, 1, 3, 4, None, None, None, None, None, 0, None) == -1      # S = 3 without a scale table
    assert lib.dgn_scale_combine_backward(5, 600, 1, 8, None, 0, None, None, None, None, None, 0, None, None) == -1
    assert "4096" in err()
    assert lib.dgn_bn_tail_workspace_bytes(0, 8) == 0 and lib.dgn_bn_tail_workspace_bytes(1000, 8) > 0
    assert lib.dgn_scale_combine_backward_workspace_bytes(1000, 5, 14) > 0


def test_message_of_x_dst_alone_is_refused_before_any_launch(lib):
    """m_j = x_dst[i] for every slot j is no message (and the gather loops read their one gathered term unconditionally): the forward and
    the backward return DGN_ERR_INVALID from the host-side checks -- nothing launched, `out` and the sinks left as they were.  Host memory
    stands in for the device's: nothing may read or write it."""
    import numpy as np
    from dgn_amd import _lib
    err = lambda: lib.dgn_last_error().decode()
    N, F_ = 3, 4
    indptr, src = np.array([0, 1, 2, 3], dtype=np.int32), np.array([1, 2, 0], dtype=np.int32)
    x = np.arange(N * F_, dtype=np.float32).reshape(N, F_)
    out, g_out = np.full((N, F_), 7.0, dtype=np.float32), np.ones((N, F_), dtype=np.float32)
    sinks = [np.full((N, F_), 9.0, dtype=np.float32) for _ in range(3)]
    ptr = lambda a: a.ctypes.data
    g = _lib.DgnGraph()
    g.n_nodes, g.n_edges, g.indptr, g.src = N, 3, ptr(indptr), ptr(src)
    spec = _lib.DgnAggSpec()
    spec.n_agg, spec.n_scalers, spec.n_towers, spec.eps = 1, 1, 1, 1e-8            # mean | identity
    msg = _lib.DgnMsg()
    msg.F, msg.x_dst, msg.ld_dst, msg.x_in, msg.ld_in = F_, ptr(x), F_, ptr(x), F_
    gr = _lib.DgnMsgGrad()
    gr.g_src, gr.ld_src, gr.g_dst, gr.ld_dst, gr.g_in, gr.ld_in = ptr(sinks[0]), F_, ptr(sinks[1]), F_, ptr(sinks[2]), F_
    args = (C.byref(g), C.byref(spec), C.byref(msg), None, 0, None)
    for accumulate in (0, 1):
        gr.accumulate = accumulate
        for rc in (lib.dgn_agg_forward(*args, ptr(out), F_, None, 0, None),
                   lib.dgn_agg_forward_aux(*args, ptr(out), F_, None, None, 0, None),
                   lib.dgn_agg_backward(*args, ptr(g_out), F_, C.byref(gr), None, 0, None),
                   lib.dgn_agg_backward_aux(*args, ptr(g_out), F_, None, C.byref(gr), None, 0, None)):
            assert rc == _lib.DGN_ERR_INVALID and "gathered term" in err(), (rc, err())
    g.n_nodes, g.n_edges = 0, 0                                                    # ... also where there is nothing to do
    assert lib.dgn_agg_forward(*args, ptr(out), F_, None, 0, None) == _lib.DGN_ERR_INVALID
    assert lib.dgn_agg_backward(*args, ptr(g_out), F_, C.byref(gr), None, 0, None) == _lib.DGN_ERR_INVALID
    assert (out == 7.0).all() and all((s == 9.0).all() for s in sinks)
    msg.x_dst = None                                                               # (no term at all: the same refusal)
    assert lib.dgn_agg_forward(*args, ptr(out), F_, None, 0, None) == _lib.DGN_ERR_INVALID and "gathered term" in err()


def test_linear_entry_points_validate_before_any_device_work(lib):
    """dgn_linear_*: width limits, dense-row and alignment requirements, workspace size -- all host-side checks."""
    err = lambda: lib.dgn_last_error().decode()
    assert lib.dgn_linear_supported(70, 140, 0) == 1 and lib.dgn_linear_supported(70, 140, 1) == 1
    assert lib.dgn_linear_supported(71, 140, 0) == 0 and lib.dgn_linear_supported(70, 162, 0) == 0      # odd / too wide
    assert lib.dgn_linear_supported(160, 160, 0) == 1 and lib.dgn_linear_supported(160, 160, 1) == 0    # 100 tiles > 45
    a = 1 << 12                                                                                        # dummy aligned pointer, never dereferenced
    assert lib.dgn_linear_forward(10, 71, 140, 1, a, 71, 0, a, 71, 0, 0, None, 0, a, 140, 0, None) == -1 and "even" in err()
    assert lib.dgn_linear_forward(10, 70, 140, 1, a, 72, 0, a, 70, 0, 0, None, 0, a, 140, 0, None) == -1 and "dense rows" in err()
    assert lib.dgn_linear_forward(10, 70, 140, 1, a + 4, 70, 0, a, 70, 0, 0, None, 0, a, 140, 0, None) == -1
    assert lib.dgn_linear_forward(10, 70, 140, 1, None, 70, 0, a, 70, 0, 0, None, 0, a, 140, 0, None) == -1 and "null" in err()
    assert lib.dgn_linear_forward(0, 70, 140, 1, None, 70, 0, None, 70, 0, 0, None, 0, None, 140, 0, None) == 0      # no rows: nothing to do
    need = lib.dgn_linear_wgrad_workspace_bytes(1000, 70, 140, 1)
    assert need > 0 and lib.dgn_linear_wgrad_workspace_bytes(1000, 70, 141, 1) == 0
    assert lib.dgn_linear_wgrad(1000, 70, 140, 1, a, 140, 0, a, 70, 0, a, 70, 0, None, 0, a, need - 1, None) == -1 and "workspace" in err()
    assert lib.dgn_linear_wgrad(1000, 64, 140, 1, a, 140, 0, a, 64, 0, a, 64, 0, a, 0, a, need, None) == -1 and "bias gradient" in err()
    assert lib.dgn_linear_combine_forward(10, 84, 5, 4, 14, a, 0, a, 84, 0, a, None, None, a, 70, None) == -1 and "3 scalers" in err()
    assert lib.dgn_linear_combine_forward(10, 84, 5, 3, 14, a, 0, a, 84, 0, None, None, None, a, 70, None) == -1       # 3 scalers need the table
    assert lib.dgn_linear_combine_backward_input(10, 5, 3, 13, 84, a, 0, a, a, 84, 0, a, 0, None) == -1 and "even f_out" in err()
    assert lib.dgn_linear_combine_backward_weight(10, 5, 3, 14, 84, a, 0, a, a, 0, a, 84, 0, None, 0, None) == -1 and "workspace" in err()
