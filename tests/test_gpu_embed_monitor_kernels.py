"""``functional.embedding_monitor`` (``spcl_embed_monitor``, csrc/embed_monitor.hip) on the device against the float64
restatement of tests/_embed_monitor_oracle.py.  Neighbour identities are never compared with the oracle's (top-k gaps of
clustered rows go down to 1e-8): every check is the tie-independent one of ``O.check`` with tol = (d + 8) 2^-24."""
import numpy as np
import pytest
import torch

from tests import _embed_monitor_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _F():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    return F_hip


def _rows(N, d, seed, clusters=6, spread=0.35):
    """seeded clustered rows of uneven length, three label kinds (cluster, its parity, wide values up to 65535) and the
    two-view pair layout (row i <-> i + N // 2; the middle row of an odd N has none)"""
    g = np.random.default_rng(seed)
    centres = g.standard_normal((clusters, d))
    which = g.integers(0, clusters, N)
    z = centres[which] + spread * g.standard_normal((N, d))
    M = N // 2
    z[M:2 * M] = z[:M] + 0.1 * g.standard_normal((M, d))  # the other view lies near its slice
    which[M:2 * M] = which[:M]
    z *= g.uniform(0.5, 3.0, (N, 1))
    labels = np.stack([which, which % 2, g.integers(0, 65536, N)]).astype(np.int64)
    pair = np.full(N, -1, dtype=np.int64)
    pair[:M] = np.arange(M) + M
    pair[M:2 * M] = np.arange(M)
    return z.astype(np.float32), labels, pair


def _call(z, labels, pair, k, exclude_pair):
    F_hip = _F()
    zt = torch.from_numpy(z).to(DEV)
    lt = None if labels is None else torch.from_numpy(labels).to(DEV)
    pt = None if pair is None else torch.from_numpy(pair).to(DEV)
    return F_hip.embedding_monitor(zt, lt, pt, k=k, exclude_pair=exclude_pair)


def _np(res):
    return {name: getattr(res, name).cpu().numpy() for name in res._fields}


@pytest.mark.parametrize("d", [1, 3, 20, 64, 130, 256])
@pytest.mark.parametrize("N", [2, 3, 63, 64, 65, 130, 258])
def test_shape_sweep(N, d):
    z, labels, pair = _rows(N, d, seed=1000 * N + d)
    ref = O.similarity(z)
    none = np.full(N, -1, dtype=np.int64)
    for k in (1, 5, 32):
        for L in (0, 1, 3):
            for pr, excl in ((pair, True), (pair, False), (none, True)):
                lab = labels[:L] if L else None
                got = _np(_call(z, lab, pr, k, excl))
                O.check(got, z, lab, pr, k, excl, ref=ref)


def test_multi_block_sweep():
    N, d, k = 1026, 128, 20
    z, labels, pair = _rows(N, d, seed=7, clusters=12)
    got = _np(_call(z, labels, pair, k, True))
    O.check(got, z, labels, pair, k, True)


def test_pair_argument_may_be_absent():
    z, labels, _ = _rows(65, 20, seed=3)
    a = _np(_call(z, labels, None, 5, True))
    b = _np(_call(z, labels, np.full(65, -1, dtype=np.int64), 5, True))
    O.check(a, z, labels, None, 5, True)
    for name in a:
        assert np.array_equal(a[name], b[name], equal_nan=True), name


def test_duplicate_rows_are_listed_together_with_equal_bits():
    N, d, k = 130, 130, 5
    g = np.random.default_rng(11)
    # row i = centre + 5 e_i + a little noise: s(i, centre) = 0.92, s(i, j) = 0.85 -- the centre is every row's nearest
    c = np.ones(d)
    z = (c + 5.0 * np.eye(N, d) + 0.01 * g.standard_normal((N, d))).astype(np.float32)
    z[5] = z[70] = c.astype(np.float32)
    got = _np(_call(z, None, None, k, True))
    O.check(got, z, None, None, k, True)
    idx, sim = got["knn_idx"], got["knn_sim"].view(np.int32)
    for i in range(N):
        if i in (5, 70):
            continue
        assert idx[i, 0] == 5 and idx[i, 1] == 70, (i, idx[i])
        assert sim[i, 0] == sim[i, 1], (i, got["knn_sim"][i])
    assert idx[5, 0] == 70 and idx[70, 0] == 5 and sim[5, 0] == sim[70, 0]
    # s_ij == s_ji bitwise wherever both directions were returned
    where = {(i, int(j)): sim[i, t] for i in range(N) for t, j in enumerate(idx[i])}
    both = [(i, j) for (i, j) in where if (j, i) in where]
    assert len(both) > N
    assert all(where[(i, j)] == where[(j, i)] for i, j in both)


@pytest.mark.parametrize("order,winner", [([7, 9, 9, 7, 3], 7), ([9, 7, 7, 9, 3], 9), ([3, 9, 7, 7, 9], 9)])
def test_vote_tie_goes_to_the_label_ranked_first(order, winner):
    # row 0 at angle 0, rows 1 .. 5 at 5, 10, ... degrees: its neighbours in rank order are 1, 2, 3, 4, 5 (counts 2-2-1)
    ang = np.deg2rad(np.array([0.0, 5.0, 10.0, 15.0, 20.0, 25.0]))
    z = np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)
    labels = np.array([[0] + order], dtype=np.int64)
    got = _np(_call(z, labels, None, 5, True))
    assert got["knn_idx"][0].tolist() == [1, 2, 3, 4, 5]
    assert got["pred"][0, 0] == winner
    O.check(got, z, labels, None, 5, True)


def test_zero_row_is_clamped_and_reported():
    z, labels, pair = _rows(65, 20, seed=5)
    z[3] = 0.0
    got = _np(_call(z, labels, pair, 5, True))
    assert got["scalars"][3] == 0.0
    assert np.all(np.isfinite(got["knn_sim"])) and np.all(np.isfinite(got["scalars"]))
    assert np.all(got["knn_idx"] >= 0) and np.all(got["pair_rank"][pair >= 0] >= 0)
    O.check(got, z, labels, pair, 5, True)


def test_row_scale_does_not_change_the_neighbours():
    g = np.random.default_rng(17)
    u = g.standard_normal((64, 20))
    u = (u / np.sqrt((u * u).sum(1, keepdims=True))).astype(np.float32)
    unit = _np(_call(u, None, None, 5, True))
    scale = np.where(np.arange(64) % 2 == 0, 1e3, 1e-3).astype(np.float32)[:, None]
    for zs in (u * np.float32(1e3), u * np.float32(1e-3), u * scale):
        got = _np(_call(zs.astype(np.float32), None, None, 5, True))
        assert np.array_equal(got["knn_idx"], unit["knn_idx"])
        O.check(got, zs, None, None, 5, True)


@pytest.mark.parametrize("N,d,k", [(258, 64, 10), (1026, 128, 32)])
def test_two_calls_give_the_same_bits(N, d, k):
    z, labels, pair = _rows(N, d, seed=23)
    a, b = _np(_call(z, labels, pair, k, True)), _np(_call(z, labels, pair, k, True))
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


def test_inputs_are_not_modified():
    F_hip = _F()
    z, labels, pair = _rows(130, 20, seed=29)
    zt, lt, pt = torch.from_numpy(z).to(DEV), torch.from_numpy(labels).to(DEV), torch.from_numpy(pair).to(DEV)
    F_hip.embedding_monitor(zt, lt, pt, k=5)
    torch.cuda.synchronize()
    assert np.array_equal(zt.cpu().numpy(), z) and np.array_equal(lt.cpu().numpy(), labels)
    assert np.array_equal(pt.cpu().numpy(), pair)


def test_row_pitch_of_a_column_slice():
    F_hip = _F()
    z, labels, pair = _rows(65, 20, seed=31)
    wide = torch.zeros(65, 37, device=DEV)
    wide[:, :20] = torch.from_numpy(z).to(DEV)
    view = wide[:, :20]
    assert view.stride(0) == 37
    a = _np(F_hip.embedding_monitor(view, torch.from_numpy(labels).to(DEV), torch.from_numpy(pair).to(DEV), k=5))
    b = _np(_call(z, labels, pair, 5, True))
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


def test_graph_replay_sees_inputs_overwritten_in_place():
    F_hip = _F()
    N, d, k = 130, 64, 5
    z1, l1, p1 = _rows(N, d, seed=37)
    z2, l2, p2 = _rows(N, d, seed=41)
    p2[:4] = -1
    zt = torch.from_numpy(z1).to(DEV)
    lt = torch.from_numpy(l1).to(torch.int32).to(DEV)
    pt = torch.from_numpy(p1).to(torch.int32).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        F_hip.embedding_monitor(zt, lt, pt, k=k)  # (workspace allocated outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = F_hip.embedding_monitor(zt, lt, pt, k=k)
    graph.replay()
    O.check(_np(res), z1, l1, p1, k, True)
    zt.copy_(torch.from_numpy(z2))
    lt.copy_(torch.from_numpy(l2))
    pt.copy_(torch.from_numpy(p2))
    graph.replay()
    got = _np(res)
    O.check(got, z2, l2, p2, k, True)
    eager = _np(_call(z2, l2, p2, k, True))
    for name in got:
        assert got[name].tobytes() == eager[name].tobytes(), name


def test_library_refuses_shapes_outside_the_limits():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    z = torch.zeros(4, 4, device=DEV)
    out = torch.zeros(1024, dtype=torch.uint8, device=DEV)
    for N, d, k in ((1, 4, 1), (8193, 4, 1), (4, 0, 1), (4, 513, 1), (4, 4, 0), (4, 4, 33)):
        assert native.call("spcl_embed_monitor_workspace_bytes", N, d, k) == 0
        with pytest.raises(RuntimeError, match="spcl_embed_monitor"):
            native.call("spcl_embed_monitor", native.ptr(z), max(d, 1), None, 0, None, N, d, k, 1, native.ptr(out),
                        native.ptr(out), None, None, native.ptr(out), native.ptr(out), native.ptr(out), out.numel(),
                        native.stream())
