"""``dgn_eig_mid`` (one packed-storage Jacobi workgroup per graph of 65 to 192 nodes) on the GPU: the dense per-graph oracle at the limits of
both width classes and on the degenerate cases, chaining after ``dgn_eig_small``, ``batch_eig``'s routes, a foreign edge, bit-reproducibility
across batch compositions and log slots, and HIP-graph capture.  Tolerances as tests/test_eig_small_gpu.py: 1e-10 on fp64 eigenvalues, 5e-5
on the residuals of the fp32 columns, 2e-5 on cluster projectors (clusters by the 1e-6 rule), 1 <= status < 30."""
import numpy as np
import pytest
import torch

import eig_mid_model as M

pytestmark = pytest.mark.gpu

K = 6
NAMES = [name for name, _ in M.mid_graphs()]
_ORACLE = {}


def _cat(graphs):
    """list of (src, dst, n) -> (src, dst, sizes) of the batch (torch int64, global ids)"""
    srcs, dsts, sizes, off = [], [], [], 0
    for s, d, n in graphs:
        srcs.append(np.asarray(s, dtype=np.int64) + off)
        dsts.append(np.asarray(d, dtype=np.int64) + off)
        sizes.append(int(n))
        off += int(n)
    return torch.from_numpy(np.concatenate(srcs)), torch.from_numpy(np.concatenate(dsts)), sizes


def _offsets(sizes, dev="cuda"):
    off = torch.zeros(len(sizes) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.as_tensor(sizes, dtype=torch.int64), 0)
    return off.to(dev)


def _graph(src, dst, sizes):
    import dgn_amd
    return dgn_amd.DGNGraph(src.cuda(), dst.cuda(), int(sum(sizes)))


def _solve_mid(src, dst, sizes, k=K, norm="none", ids=None, **kw):
    """laplacian_eig_mid on a fresh DGNGraph -> (vec, values, status) on the host"""
    import dgn_amd
    if ids is not None:
        kw["graph_ids"] = torch.as_tensor(ids, dtype=torch.int32, device="cuda")
    vec, val, st = dgn_amd.laplacian_eig_mid(_graph(src, dst, sizes), _offsets(sizes), k, norm, **kw)
    torch.cuda.synchronize()
    return vec.cpu(), val.cpu(), st.cpu()


def _clusters(w, kk, n, tol=1e-6):
    """index ranges [j, e) of (near-)equal eigenvalues among the first kk that lie wholly inside the first kk columns"""
    j = 0
    while j < kk:
        e = j + 1
        while e < n and abs(w[e] - w[j]) < tol:
            e += 1
        if e <= kk:
            yield j, e
        j = e


def _oracle(key, src, dst, sizes, k, norm):
    """the dense oracle of a batch, computed once per (batch, norm); checks the precondition of the cluster rule on the way"""
    from oracle import eig_oracle
    if (key, norm) not in _ORACLE:
        ref = eig_oracle.eigvecs(src.numpy(), dst.numpy(), sizes, k, norm)
        for n, (w, _) in zip(sizes, ref):
            M.assert_unambiguous_clusters(w, min(k, n - 1))
        _ORACLE[(key, norm)] = ref
    return _ORACLE[(key, norm)]


def _check_against_oracle(key, vec, val, st, src, dst, sizes, norm, k=K):
    from oracle import eig_oracle
    ref = _oracle(key, src, dst, sizes, k, norm)
    vec, val, off = vec.double().numpy(), val.numpy(), 0
    s_np, d_np = src.numpy(), dst.numpy()
    for g, (n, (w, v)) in enumerate(zip(sizes, ref)):
        blk, kk = vec[off:off + n], min(k, n)
        assert np.all(blk[:, kk:] == 0) and np.all(np.isnan(val[g, kk:])), g           # fewer nodes than k: zero columns, NaN values
        np.testing.assert_allclose(val[g, :kk], w[:kk], rtol=0, atol=1e-10, err_msg=f"graph {g}")
        for j, e in _clusters(w, kk, n):
            np.testing.assert_allclose(blk[:, j:e] @ blk[:, j:e].T, v[:, j:e] @ v[:, j:e].T, atol=2e-5, err_msg=f"graph {g}")
        m = (d_np >= off) & (d_np < off + n)
        L = eig_oracle.graph_laplacian(s_np[m] - off, d_np[m] - off, n, norm)
        for c in range(kk):
            np.testing.assert_allclose(L @ blk[:, c], w[c] * blk[:, c], atol=5e-5, err_msg=f"graph {g} column {c}")
        off += n
    if st is not None:
        assert int(st.min()) >= 1 and int(st.max()) < 30, st.tolist()


@pytest.fixture(scope="module")
def graphs():
    return dict(M.mid_graphs())


@pytest.fixture(scope="module")
def mid_batch(graphs):
    return _cat([graphs[name] for name in NAMES])


@pytest.mark.parametrize("norm", ["none", "sym"])
def test_class_limits_and_degenerate_graphs_vs_oracle(mid_batch, norm):
    src, dst, sizes = mid_batch
    assert sizes == [65, 127, 128, 129, 191, 192, 129, 138, 107, 192, 80, 70, 66]
    _oracle("mid", src, dst, sizes, K, norm)                              # (the precondition, before the GPU is called)
    vec, val, st = _solve_mid(src, dst, sizes, K, norm)
    print(f"eig_mid sweeps ({norm}): {dict(zip(NAMES, st.tolist()))}, histogram {torch.bincount(st.clamp(min=0).long()).tolist()}")
    _check_against_oracle("mid", vec, val, st, src, dst, sizes, norm)
    g = NAMES.index("edgeless70")                                         # nothing to rotate: one sweep, K unit vectors in column order
    off = sum(sizes[:g])
    assert int(st[g]) == 1 and torch.equal(vec[off:off + 70], torch.eye(70, K))


def test_walk(graphs):
    src, dst, sizes = _cat([graphs["sbm129"]])
    _oracle("sbm129", src, dst, sizes, K, "walk")
    vec, val, st = _solve_mid(src, dst, sizes, K, "walk")
    _check_against_oracle("sbm129", vec, val, st, src, dst, sizes, "walk")
    np.testing.assert_allclose(vec.double().norm(dim=0).numpy(), 1.0, atol=1e-6)


def test_widest_replay_block(graphs):
    """k = 32 on the 65-node graph: the [m][k] block of the replay at its widest, two items per thread."""
    src, dst, sizes = _cat([graphs["sbm65"]])
    _oracle("sbm65", src, dst, sizes, 32, "none")
    vec, val, st = _solve_mid(src, dst, sizes, 32, "none")
    _check_against_oracle("sbm65", vec, val, st, src, dst, sizes, "none", k=32)


@pytest.fixture(scope="module")
def chain_batch(graphs):
    from dgn_amd import synth
    mols = M.split(synth.molecule_batch(12, seed=7, laplacian_eig=False))
    big = M.split(synth.sbm_batch(1, seed=4, n_lo=193, n_hi=193))[0]
    mids = [graphs[name] for name in NAMES]
    order = mols[:5] + mids[:6] + [big] + mols[5:] + mids[6:]              # graph 11 has 193 nodes
    return _cat(order), _cat(mols)


def test_chaining_after_the_small_kernel(chain_batch):
    import dgn_amd
    (src, dst, sizes), (m_src, m_dst, m_sizes) = chain_batch
    assert sizes[11] == 193 and max(sizes[:5] + sizes[12:19]) <= 64
    _oracle("chain", src, dst, sizes, K, "none")
    graph, off = _graph(src, dst, sizes), _offsets(sizes)
    N, G = sum(sizes), len(sizes)
    vec = torch.full((N, K), 7.0, dtype=torch.float32, device="cuda")
    val = torch.full((G, K), 3.0, dtype=torch.float64, device="cuda")
    st = torch.zeros(G, dtype=torch.int32, device="cuda")
    dgn_amd.laplacian_eig_small(graph, off, K, "none", out=vec, values=val, status=st)
    dgn_amd.laplacian_eig_mid(graph, off, K, "none", out=vec, values=val, status=st)
    torch.cuda.synchronize()
    vec, val, st, o = vec.cpu(), val.cpu(), st.cpu(), off.cpu().tolist()
    assert int(st[11]) == -1 and bool((vec[o[11]:o[12]] == 7.0).all()) and bool((val[11] == 3.0).all())
    rest = [g for g in range(G) if g != 11]
    assert int(st[rest].min()) >= 1 and int(st[rest].max()) < 30
    # the small graphs: the bits of a laplacian_eig_small run on them alone
    a_vec, a_val, _ = dgn_amd.laplacian_eig_small(_graph(m_src, m_dst, m_sizes), _offsets(m_sizes), K, "none")
    a_vec, a_val, a_off = a_vec.cpu(), a_val.cpu(), _offsets(m_sizes, "cpu").tolist()
    for i, g in enumerate(list(range(5)) + list(range(12, 19))):
        assert torch.equal(vec[o[g]:o[g + 1]], a_vec[a_off[i]:a_off[i + 1]]) and torch.equal(val[g].view(torch.int64), a_val[i].view(torch.int64)), g
    # batch_eig: check=True solves all of them (the 193-node graph through the bucketed eigh) ...
    eig, values = dgn_amd.batch_eig(graph, sizes, K, "none")
    _check_against_oracle("chain", eig.cpu(), values.cpu(), None, src, dst, sizes, "none")
    keep = torch.ones(N, dtype=torch.bool)
    keep[o[11]:o[12]] = False
    assert torch.equal(eig.cpu()[keep], vec[keep]) and torch.equal(values.cpu()[rest].view(torch.int64), val[rest].view(torch.int64))
    # ... check=False alone leaves everything above 64 nodes zero, as before; with mid=True only the 193-node graph
    raw_vec, raw_val = dgn_amd.batch_eig(graph, sizes, K, "none", check=False)
    filled_vec, filled_val = dgn_amd.batch_eig(graph, sizes, K, "none", check=False, mid=True)
    raw_vec, raw_val, filled_vec, filled_val = raw_vec.cpu(), raw_val.cpu(), filled_vec.cpu(), filled_val.cpu()
    for g, n in enumerate(sizes):
        rows = slice(o[g], o[g + 1])
        if n > 64:
            assert bool((raw_vec[rows] == 0).all()) and bool(torch.isnan(raw_val[g]).all()), g
        else:
            assert torch.equal(raw_vec[rows], vec[rows]), g
        if n > 192:
            assert bool((filled_vec[rows] == 0).all()) and bool(torch.isnan(filled_val[g]).all()), g
        else:
            assert torch.equal(filled_vec[rows], vec[rows]) and torch.equal(filled_val[g].view(torch.int64), val[g].view(torch.int64)), g


def test_foreign_edge_into_a_mid_graph(graphs):
    import dgn_amd
    from dgn_amd import synth
    mols = M.split(synth.molecule_batch(2, seed=9, laplacian_eig=False))
    p = np.arange(100)
    path = (np.concatenate([p[:-1], p[1:]]), np.concatenate([p[1:], p[:-1]]), 100)
    src, dst, sizes = _cat([mols[0], graphs["sbm65"], path, mols[1]])
    off = _offsets(sizes, "cpu").tolist()
    src = torch.cat([src, torch.tensor([0])])                              # an edge from node 0 (graph 0) into the path graph
    dst = torch.cat([dst, torch.tensor([off[2] + 50])])
    graph, N = _graph(src, dst, sizes), sum(sizes)
    vec = torch.full((N, K), 7.0, dtype=torch.float32, device="cuda")
    val = torch.full((4, K), 3.0, dtype=torch.float64, device="cuda")
    st = torch.zeros(4, dtype=torch.int32, device="cuda")
    dgn_amd.laplacian_eig_small(graph, _offsets(sizes), K, "sym", out=vec, values=val, status=st)
    dgn_amd.laplacian_eig_mid(graph, _offsets(sizes), K, "sym", out=vec, values=val, status=st)
    torch.cuda.synchronize()
    st = st.cpu().tolist()
    assert st[2] == -2 and min(st[0], st[1], st[3]) >= 1
    assert bool((vec[off[2]:off[3]] == 7.0).all()) and bool((val[2] == 3.0).all())      # nothing of the graph is written
    clean = _solve_mid(*_cat([graphs["sbm65"]]), K, "sym")
    assert torch.equal(vec[off[1]:off[2]].cpu(), clean[0]) and torch.equal(val[1].cpu().view(torch.int64), clean[1][0].view(torch.int64))
    with pytest.raises(dgn_amd._lib.DgnError, match="graph 2"):
        dgn_amd.batch_eig(graph, sizes, K, "sym")


def _rows(vec, val, sizes):
    """per graph: (its rows of vec, its row of val as raw bits -- NaN slots compare equal)"""
    off, out = 0, []
    for g, n in enumerate(sizes):
        out.append((vec[off:off + n], val[g].view(torch.int64)))
        off += n
    return out


@pytest.mark.parametrize("norm", ["none", "sym"])
def test_bit_reproducible_across_batches_and_log_slots(graphs, norm):
    from dgn_amd import synth
    mine = [graphs["sbm65"], graphs["knn2"], graphs["sbm129"]]            # both classes
    others = M.split(synth.molecule_batch(4, seed=5, laplacian_eig=False)) + [graphs["rings2x40"], graphs["knn1"], graphs["loop66"]]
    alone = _rows(*_solve_mid(*_cat(mine), K, norm)[:2], [n for _, _, n in mine])
    assert all(bool(r[0].abs().sum() > 0) for r in alone)
    perm = [2, 0, 1]
    got = _rows(*_solve_mid(*_cat([mine[i] for i in perm]), K, norm)[:2], [mine[i][2] for i in perm])
    for pos, i in enumerate(perm):
        assert torch.equal(got[pos][0], alone[i][0]) and torch.equal(got[pos][1], alone[i][1]), (pos, i)
    mixed = [others[0], mine[0], others[4], others[1], mine[1], others[5], others[2], others[6], mine[2], others[3]]
    where = [1, 4, 8]
    batch, sizes = _cat(mixed), [n for _, _, n in mixed]
    for ids in (None, [8, 4, 1], [5, 1, 7, 8, 2, 4]):                       # log slot = graph index, or the place in the list
        vec, val, st = _solve_mid(*batch, K, norm, ids=ids)
        got = _rows(vec, val, sizes)
        for i, pos in enumerate(where):
            assert torch.equal(got[pos][0], alone[i][0]) and torch.equal(got[pos][1], alone[i][1]), (ids, pos)
        solved = [g for g, n in enumerate(sizes) if n > 64 and (ids is None or g in ids)]
        assert [g for g in range(len(sizes)) if st[g] != 0] == solved


def test_capture_and_replay(graphs):
    """One capture of laplacian_eig_small + laplacian_eig_mid over a padded graph with a preallocated workspace serves every batch that
    fits: replay == the eager calls on that batch."""
    import dgn_amd
    from dgn_amd import _lib, synth
    dev = torch.device("cuda")
    mols = M.split(synth.molecule_batch(8, seed=1, laplacian_eig=False))
    batches = [_cat(mols[:5] + [graphs["loop66"], graphs["knn2"]]), _cat([graphs["sbm129"]] + mols[5:])]
    n_cap, e_cap, g_cap = 400, 12000, 8
    graph = dgn_amd.DGNGraph.padded(n_cap, e_cap, dev)
    off = torch.zeros(g_cap + 1, dtype=torch.int64, device=dev)
    out = torch.zeros(n_cap, K, dtype=torch.float32, device=dev)
    val = torch.zeros(g_cap, K, dtype=torch.float64, device=dev)
    st = torch.zeros(g_cap, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().dgn_eig_mid_workspace_bytes(g_cap, 30), dtype=torch.uint8, device=dev)

    def load(b):
        src, dst, sizes = b
        assert sum(sizes) <= n_cap and src.numel() <= e_cap and len(sizes) <= g_cap
        graph.rebuild(src, dst, sum(sizes))
        off.copy_(_offsets(sizes + [0] * (g_cap - len(sizes))))           # unused graph slots are empty: offset = the batch's node count
        out.zero_()

    def both(**kw):
        r = dgn_amd.laplacian_eig_small(graph, off, K, "sym", **{k: v for k, v in kw.items() if k != "workspace"})
        return dgn_amd.laplacian_eig_mid(graph, off, K, "sym", out=r[0], values=r[1], status=r[2], workspace=kw.get("workspace"))

    load(batches[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                          # warm-up outside the capture
        both(out=out, values=val, status=st, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        both(out=out, values=val, status=st, workspace=ws)
    for b in batches:
        load(b)
        cg.replay()
        torch.cuda.synchronize()
        got = (out.clone(), val.clone(), st.clone())
        want = both()
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int64), want[1].view(torch.int64)) and torch.equal(got[2], want[2])
        n_g = len(b[2])
        assert int(got[2][:n_g].min()) >= 1 and int(got[2][:n_g].max()) < 30 and bool(got[0][:sum(b[2])].abs().sum() > 0)
        for g, n in enumerate(b[2]):                                       # every graph's rows are filled, the mid ones included
            o = sum(b[2][:g])
            assert bool(got[0][o:o + n].abs().sum() > 0), g
    graph.check_deferred()
