"""``dgn_eig_small`` (one Jacobi workgroup per graph) on the GPU: the reference's fixtures, the dense per-graph oracle at the width-class
boundaries, directed graphs, bit-reproducibility across batch compositions, oversize graphs and foreign edges, and HIP-graph capture.
Tolerances: 5e-5 on fp32 eigenvector columns (residuals, subspaces) and 2e-5 on projectors as in test_eig_hip.py; 1e-10 on fp64 eigenvalues."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 6


def _split(b):
    """a synth batch -> list of per-graph (src, dst, n) with local node ids (numpy)"""
    src, dst, out, off = b["src"].numpy(), b["dst"].numpy(), [], 0
    for n in b["sizes"].tolist():
        m = (dst >= off) & (dst < off + n)
        out.append((src[m] - off, dst[m] - off, int(n)))
        off += n
    return out


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


def _solve(src, dst, sizes, k=K, norm="none", **kw):
    """laplacian_eig_small on a fresh DGNGraph -> (vec, values, status) on the host"""
    import dgn_amd
    graph = dgn_amd.DGNGraph(src.cuda(), dst.cuda(), int(sum(sizes)))
    vec, val, st = dgn_amd.laplacian_eig_small(graph, _offsets(sizes), k, norm, **kw)
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


def _check_against_oracle(vec, val, st, src, dst, sizes, norm, k=K):
    from oracle import eig_oracle
    ref = eig_oracle.eigvecs(src.numpy(), dst.numpy(), sizes, k, norm)
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
    assert int(st.min()) >= 1 and int(st.max()) < 30, st.tolist()


def _fixture_batch(g):
    graphs = [(g[f"g{i}/src"], g[f"g{i}/dst"], int(g[f"g{i}/n"])) for i in range(int(g["n_graphs"]))]
    return _cat(graphs)


@pytest.mark.parametrize("norm", ["none", "sym", "walk"])
def test_g9_fixture(golden, norm):
    """Every column is an eigenvector of the L the reference's get_eig built (data/molecules.py:100-116), with its sorted eigenvalue; same
    subspaces as the columns it stored; eigenvalues against numpy's on that L (non-symmetric for 'walk')."""
    g = golden("g9_laplacian")
    k = int(g["pos_enc_dim"])
    src, dst, sizes = _fixture_batch(g)
    vec, val, st = _solve(src, dst, sizes, k, norm)
    vec, off = vec.double().numpy(), 0
    for i, n in enumerate(sizes):
        L, ref, blk = g[f"g{i}/{norm}/L"], g[f"g{i}/{norm}/eig"].astype(np.float64), vec[off:off + n]
        w = np.sort(np.linalg.eigvals(L).real)
        np.testing.assert_allclose(val[i].numpy(), w[:k], rtol=0, atol=1e-10)
        for c in range(k):
            np.testing.assert_allclose(L @ blk[:, c], w[c] * blk[:, c], atol=5e-5)
        for j, e in _clusters(w, k, n):
            coef, *_ = np.linalg.lstsq(blk[:, j:e], ref[:, j:e], rcond=None)
            np.testing.assert_allclose(blk[:, j:e] @ coef, ref[:, j:e], atol=5e-5)
        off += n
    assert int(st.min()) >= 1 and int(st.max()) < 30


def test_g14_positional_encoding(golden):
    """positional_encoding against what the reference's routine stored (data/molecules.py:18-32), by subspace."""
    import dgn_amd
    g = golden("g14_pos_enc")
    p = int(g["pos_enc_dim"])
    src, dst, sizes = _fixture_batch(g)
    graph = dgn_amd.DGNGraph(src.cuda(), dst.cuda(), sum(sizes))
    pe = dgn_amd.positional_encoding(graph, sizes, p)
    assert pe.shape == (sum(sizes), p) and pe.dtype == torch.float32
    pe, off = pe.cpu().double().numpy(), 0
    for i, n in enumerate(sizes):
        w, ref, blk = g[f"g{i}/eigval"], g[f"g{i}/pos_enc"].astype(np.float64), pe[off:off + n]
        for j, e in _clusters(w, p + 1, n):
            if j == 0:                                                   # column 0 (the null vector) is not part of pos_enc
                assert e == 1
                continue
            coef, *_ = np.linalg.lstsq(blk[:, j - 1:e - 1], ref[:, j - 1:e - 1], rcond=None)
            np.testing.assert_allclose(blk[:, j - 1:e - 1] @ coef, ref[:, j - 1:e - 1], atol=5e-5)
        off += n


@pytest.fixture(scope="module")
def boundary_batch():
    from dgn_amd import synth
    graphs = _split(synth.molecule_batch(40, seed=7, laplacian_eig=False))
    graphs.append(([], [], 1))                                            # one node, no edge
    graphs.append(([0, 1], [1, 0], 2))                                    # two nodes, one bond
    for i, n in enumerate((31, 32, 33, 63, 64)):                         # both sides of each width class's limit, dense
        graphs += _split(synth.sbm_batch(1, seed=20 + i, n_lo=n, n_hi=n))
    graphs.append(([], [], 4))                                            # no edges at all (fewer nodes than k)
    path = np.arange(6)
    graphs.append((np.concatenate([path[:-1], path[1:], [2]]), np.concatenate([path[1:], path[:-1], [2]]), 7))   # a self-loop, an isolated node
    return _cat(graphs)


@pytest.mark.parametrize("norm", ["none", "sym"])
def test_class_boundaries_vs_oracle(boundary_batch, norm):
    src, dst, sizes = boundary_batch
    assert sizes[40:] == [1, 2, 31, 32, 33, 63, 64, 4, 7]
    vec, val, st = _solve(src, dst, sizes, K, norm)
    print(f"eig_small sweeps ({norm}): max {int(st.max())}, histogram {torch.bincount(st.long()).tolist()}")
    _check_against_oracle(vec, val, st, src, dst, sizes, norm)


@pytest.mark.parametrize("norm", ["none", "sym"])
def test_directed_graphs(norm):
    """k-nearest-neighbour graphs (directed, in-degree 0 possible): the symmetrised adjacency (A + A^T) / 2, as the oracle defines it."""
    from dgn_amd import synth
    b = synth.knn_batch(6, seed=5, n_lo=30, n_hi=64)
    sizes = b["sizes"].tolist()
    vec, val, st = _solve(b["src"], b["dst"], sizes, K, norm)
    _check_against_oracle(vec, val, st, b["src"], b["dst"], sizes, norm)


def _rows(vec, val, sizes):
    """per graph: (its rows of vec, its row of val as raw bits -- NaN slots compare equal)"""
    off, out = 0, []
    for g, n in enumerate(sizes):
        out.append((vec[off:off + n], val[g].view(torch.int64)))
        off += n
    return out


@pytest.mark.parametrize("norm", ["none", "sym"])
def test_bit_reproducible_across_batches(norm):
    from dgn_amd import synth
    mine = _split(synth.molecule_batch(20, seed=3, laplacian_eig=False))
    others = _split(synth.molecule_batch(40, seed=5, laplacian_eig=False)) + _split(synth.sbm_batch(10, seed=6, n_lo=33, n_hi=64))
    alone = _rows(*_solve(*_cat(mine), K, norm)[:2], [n for _, _, n in mine])
    perm = np.random.default_rng(0).permutation(20).tolist()
    shuffled = [mine[i] for i in perm]
    got = _rows(*_solve(*_cat(shuffled), K, norm)[:2], [n for _, _, n in shuffled])
    for pos, i in enumerate(perm):
        assert torch.equal(got[pos][0], alone[i][0]) and torch.equal(got[pos][1], alone[i][1]), (pos, i)
    mixed, where = [], []
    for i in range(50):
        mixed.append(others[i])
        if i % 2 == 0 and i // 2 < 20:
            where.append(len(mixed))
            mixed.append(mine[i // 2])
    got = _rows(*_solve(*_cat(mixed), K, norm)[:2], [n for _, _, n in mixed])
    for i, pos in enumerate(where):
        assert torch.equal(got[pos][0], alone[i][0]) and torch.equal(got[pos][1], alone[i][1]), (pos, i)


def test_oversize_and_foreign_edges():
    import dgn_amd
    from dgn_amd import synth
    from oracle import eig_oracle
    base = _split(synth.molecule_batch(12, seed=9, laplacian_eig=False))
    big = _split(synth.sbm_batch(1, seed=4, n_lo=65, n_hi=65))[0]
    path = np.arange(10)
    clean = (np.concatenate([path[:-1], path[1:]]), np.concatenate([path[1:], path[:-1]]), 10)
    graphs = base[:3] + [big] + base[3:6] + [clean] + base[6:]            # the 65-node graph is graph 3, the path graph 7
    src, dst, sizes = _cat(graphs)
    off = _offsets(sizes, "cpu").tolist()
    src_bad = torch.cat([src, torch.tensor([0])])                          # an edge from node 0 (graph 0) into the path graph
    dst_bad = torch.cat([dst, torch.tensor([off[7] + 4])])
    N = sum(sizes)
    pre_vec = torch.full((N, K), 7.0, dtype=torch.float32, device="cuda")
    pre_val = torch.full((len(sizes), K), 3.0, dtype=torch.float64, device="cuda")
    vec, val, st = _solve(src_bad, dst_bad, sizes, K, "none", out=pre_vec, values=pre_val)
    assert st[3] == -1 and st[7] == -2 and int(st[[0, 1, 2, 4, 5, 6] + list(range(8, 14))].min()) >= 1
    got = _rows(vec, val, sizes)
    for g in (3, 7):                                                       # nothing of theirs is written
        assert bool((got[g][0] == 7.0).all()) and bool((val[g] == 3.0).all())
    rest = base
    want = _rows(*_solve(*_cat(rest), K, "none")[:2], [n for _, _, n in rest])
    for i, g in enumerate([0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13]):
        assert torch.equal(got[g][0], want[i][0]) and torch.equal(got[g][1], want[i][1]), g

    bad_graph = dgn_amd.DGNGraph(src_bad.cuda(), dst_bad.cuda(), N)
    with pytest.raises(dgn_amd._lib.DgnError, match="graph 7"):
        dgn_amd.batch_eig(bad_graph, sizes, K, "none")
    # without the foreign edge the 65-node graph goes through the bucketed eigh; check=False leaves its rows zero
    graph = dgn_amd.DGNGraph(src.cuda(), dst.cuda(), N)
    raw_vec, raw_val = dgn_amd.batch_eig(graph, sizes, K, "none", check=False)
    assert bool((raw_vec[off[3]:off[4]] == 0).all()) and bool(torch.isnan(raw_val[3]).all())
    eig, values = dgn_amd.batch_eig(graph, sizes, K, "none")
    eig, values = eig.cpu().double().numpy(), values.cpu().numpy()
    w, v = eig_oracle.eigvecs(src.numpy(), dst.numpy(), sizes, K, "none")[3]
    blk = eig[off[3]:off[4]]
    np.testing.assert_allclose(values[3], w[:K], rtol=0, atol=1e-10)
    L = eig_oracle.graph_laplacian(big[0], big[1], 65, "none")
    for c in range(K):
        np.testing.assert_allclose(L @ blk[:, c], w[c] * blk[:, c], atol=5e-5)
    for j, e in _clusters(w, K, 65):
        np.testing.assert_allclose(blk[:, j:e] @ blk[:, j:e].T, v[:, j:e] @ v[:, j:e].T, atol=2e-5)
    others = [g for g in range(14) if g != 3]
    for g in others:                                                       # the fallback touches no other graph's rows
        assert torch.equal(torch.from_numpy(eig[off[g]:off[g + 1]]).float(), raw_vec[off[g]:off[g + 1]].cpu())


def test_capture_and_replay():
    """One capture of laplacian_eig_small over a padded graph serves every batch that fits: replay == the eager call on that batch."""
    import dgn_amd
    from dgn_amd import synth
    dev = torch.device("cuda")
    batches = [synth.molecule_batch(10, seed=1, laplacian_eig=False), synth.molecule_batch(7, seed=2, laplacian_eig=False)]
    n_cap, e_cap, g_cap = 400, 1000, 10
    graph = dgn_amd.DGNGraph.padded(n_cap, e_cap, dev)
    off = torch.zeros(g_cap + 1, dtype=torch.int64, device=dev)
    out = torch.zeros(n_cap, K, dtype=torch.float32, device=dev)
    val = torch.zeros(g_cap, K, dtype=torch.float64, device=dev)
    st = torch.zeros(g_cap, dtype=torch.int32, device=dev)

    def load(b):
        sizes = b["sizes"].tolist()
        graph.rebuild(b["src"], b["dst"], int(b["num_nodes"]))
        o = _offsets(sizes + [0] * (g_cap - len(sizes)))                   # unused graph slots are empty: offset = the batch's node count
        off.copy_(o)
        out.zero_()

    load(batches[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                          # warm-up outside the capture
        dgn_amd.laplacian_eig_small(graph, off, K, "sym", out=out, values=val, status=st)
    torch.cuda.current_stream().wait_stream(side)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        dgn_amd.laplacian_eig_small(graph, off, K, "sym", out=out, values=val, status=st)
    for b in batches:
        load(b)
        cg.replay()
        torch.cuda.synchronize()
        got = (out.clone(), val.clone(), st.clone())
        want = dgn_amd.laplacian_eig_small(graph, off, K, "sym")
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int64), want[1].view(torch.int64)) and torch.equal(got[2], want[2])
        n_g = b["sizes"].numel()
        assert int(got[2][:n_g].min()) >= 1 and bool(got[0][:int(b["num_nodes"])].abs().sum() > 0)
    graph.check_deferred()
