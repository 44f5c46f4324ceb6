"""``functional.embedding_monitor(group=...)`` (``spcl_embed_monitor_grouped``) and ``functional.cell_majority``
(``spcl_cell_majority``; both csrc/embed_monitor.hip) on the device against tests/_dense_monitor_oracle.py: the grouped
neighbour lists by the tie-independent check of ``O.check`` (tol = (d + 8) 2^-24) plus the exact statement that no neighbour
shares its row's group; the cell labels and purities exactly."""
import numpy as np
import pytest
import torch

from tests import _dense_monitor_oracle as D

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _F():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    return F_hip


def _rows(N, d, seed, clusters=6, spread=0.35):
    """seeded clustered rows of uneven length, two label kinds and the two-view pair layout (row i <-> i + N // 2)"""
    g = np.random.default_rng(seed)
    centres = g.standard_normal((clusters, d))
    which = g.integers(0, clusters, N)
    z = centres[which] + spread * g.standard_normal((N, d))
    z *= g.uniform(0.5, 3.0, (N, 1))
    M = N // 2
    pair = np.full(N, -1, dtype=np.int64)
    pair[:M] = np.arange(M) + M
    pair[M:2 * M] = np.arange(M)
    return z.astype(np.float32), np.stack([which, which % 2]).astype(np.int64), pair


def _call(z, labels, pair, k, group, exclude_pair=True):
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).to(DEV)  # noqa: E731
    return _F().embedding_monitor(t(z), t(labels), t(pair), k=k, exclude_pair=exclude_pair, group=t(group))


def _np(res):
    return {name: getattr(res, name).cpu().numpy() for name in res._fields}


def _same_bits(a, b):
    for name in a:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), name


def _groups(N, d):
    """the groups of the three grouped cases"""
    if (N, d) == (130, 5):  # unequal sizes; group 2 is rows 60 .. 70, across the border of the 64-row tiles
        g = np.empty(N, dtype=np.int64)
        g[:7], g[7:60], g[60:71], g[71:100], g[100:] = 0, 1, 2, 3, 4
        return g
    if (N, d) == (300, 64):
        return np.random.default_rng(5).integers(0, 7, N)
    return np.repeat(np.arange(4), 48)


SHAPES = [(130, 5, 3), (300, 64, 20), (192, 256, 32)]


# ---- group == NULL is the call it always was
@pytest.mark.parametrize("N,d,k", SHAPES[:2])  # (2 and 4 column splits: the merge of the close runs)
def test_null_group_is_the_old_path_bit_for_bit(N, d, k, golden):
    gold = golden("g16_embed_monitor_bits.npz")
    tag = f"n{N}_d{d}_k{k}_"
    z, labels, pair = gold[tag + "z"], gold[tag + "labels"], gold[tag + "pair"]
    plain = _np(_call(z, labels, pair, k, None))
    # the outputs of `spcl_embed_monitor` as the library computed them before it knew of groups (ABI 29), recorded on an MI355X
    _same_bits(plain, {name: gold[tag + name] for name in plain})
    D.check(plain, z, labels, pair, k, True, None)
    # the same code path: the grouped entry with ids that leave nothing out gives the same bits
    _same_bits(plain, _np(_call(z, labels, pair, k, np.full(N, -1, dtype=np.int64))))
    _same_bits(plain, _np(_call(z, labels, pair, k, np.arange(N))))  # (every row its own group: only i == j is left out)


# ---- grouped against the oracle
@pytest.mark.parametrize("N,d,k", SHAPES)
def test_grouped_against_the_oracle(N, d, k):
    z, labels, pair = _rows(N, d, seed=100 * N + d)
    group = _groups(N, d)
    ref = D.O.similarity(z)
    for pr, excl in ((None, True), (pair, True), (pair, False)):
        got = _np(_call(z, labels, pr, k, group, excl))
        D.check(got, z, labels, pr, k, excl, group, ref=ref)
        idx = got["knn_idx"]  # (the exact statement once more, in the open)
        assert not np.any((idx >= 0) & (group[np.maximum(idx, 0)] == group[:, None]))
    # uniformity, alignment, pair_rank and min_norm do not see the groups: the same bits as the ungrouped call
    plain, grouped = _np(_call(z, labels, pair, k, None)), _np(_call(z, labels, pair, k, group))
    _same_bits({n: plain[n] for n in ("pair_rank", "scalars")}, {n: grouped[n] for n in ("pair_rank", "scalars")})


def test_few_candidates_leave_tails_and_one_group_leaves_nothing():
    N, d, k = 130, 5, 3
    z, labels, _ = _rows(N, d, seed=21)
    group = np.zeros(N, dtype=np.int64)
    group[64], group[129] = 1, 2  # all rows but two in one group
    got = _np(_call(z, labels, None, k, group))
    D.check(got, z, labels, None, k, True, group)
    for i in range(N):
        if i in (64, 129):  # a group of its own: every other row is a candidate
            assert np.all(got["knn_idx"][i] >= 0) and np.all(np.isfinite(got["knn_sim"][i]))
            continue
        assert sorted(got["knn_idx"][i, :2].tolist()) == [64, 129], i
        assert got["knn_idx"][i, 2] == -1 and np.isneginf(got["knn_sim"][i, 2]) and np.all(np.isfinite(got["knn_sim"][i, :2]))
    got = _np(_call(z, labels, None, k, np.full(N, 3, dtype=np.int64)))  # every row in one group
    assert np.all(got["knn_idx"] == -1) and np.all(np.isneginf(got["knn_sim"]))
    assert np.all(got["pred"] == -1) and got["correct"].tolist() == [0, 0]
    D.check(got, z, labels, None, k, True, np.full(N, 3, dtype=np.int64))


def test_negative_ids_exclude_nothing_beyond_the_row_itself():
    N, d, k = 130, 5, 3
    z, labels, pair = _rows(N, d, seed=22)
    group = _groups(N, d).copy()
    loose = np.arange(N) % 3 == 0
    group[loose] = -1 - (np.arange(N)[loose] % 2)  # -1 and -2: two rows with the SAME negative id still see each other
    got = _np(_call(z, labels, pair, k, group))
    D.check(got, z, labels, pair, k, True, group)
    plain = _np(_call(z, labels, pair, k, None))
    for name in ("knn_idx", "knn_sim"):  # an ungrouped row's list is the ungrouped call's
        assert np.array_equal(got[name][loose], plain[name][loose]), name
    assert np.array_equal(got["pred"][:, loose], plain["pred"][:, loose])
    assert not np.array_equal(got["knn_idx"][~loose], plain["knn_idx"][~loose])  # (the grouped rows do differ)


def test_exact_ties_go_to_the_lower_index_and_never_to_the_own_group():
    N, d, k = 130, 130, 4
    g = np.random.default_rng(23)
    # row i = centre + 5 e_i + a little noise: s(i, centre) = 0.92, s(i, j) = 0.85 -- the centre is every row's nearest
    c = np.ones(d)
    z = (c + 5.0 * np.eye(N, d) + 0.01 * g.standard_normal((N, d))).astype(np.float32)
    dup = [5, 66, 70, 129]  # four copies of the centre, every other row's nearest rows, on both sides of a tile border
    for i in dup:
        z[i] = c.astype(np.float32)
    group = np.arange(N) % 5 + 10
    group[5], group[66], group[70], group[129] = 0, 1, 0, 2
    got = _np(_call(z, None, None, k, group))
    D.check(got, z, None, None, k, True, group)
    idx, sim = got["knn_idx"], got["knn_sim"].view(np.int32)
    for i in range(N):
        want = [j for j in dup if j != i and group[j] != group[i]]  # in index order: equal bits, the lower index first
        assert idx[i, :len(want)].tolist() == want, (i, idx[i])
        assert len(set(sim[i, :len(want)].tolist())) == 1
    assert idx[5, :2].tolist() == [66, 129] and 70 not in idx[5]  # the duplicate in the row's own group never appears
    assert idx[70, :2].tolist() == [66, 129] and 5 not in idx[70]


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    N, d, k = 300, 64, 20
    z, labels, pair = _rows(N, d, seed=24)
    group = _groups(N, d)
    F_hip = _F()
    zt, lt, pt, gt = (torch.from_numpy(a).to(DEV) for a in (z, labels, pair, group))
    gt = gt.to(torch.int32)
    a = F_hip.embedding_monitor(zt, lt, pt, k=k, group=gt)  # (the shape's workspace exists before the capture)
    b = F_hip.embedding_monitor(zt, lt, pt, k=k, group=gt)
    _same_bits(_np(a), _np(b))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            c = F_hip.embedding_monitor(zt, lt, pt, k=k, group=gt)
    for t in c:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _same_bits(_np(a), _np(c))


@pytest.mark.parametrize("bad", ["short", "float", "bool", "cpu", "list"])
def test_bad_group_is_refused_on_the_host(bad):
    F_hip = _F()
    N = 8
    z = torch.randn(N, 4, device=DEV)
    group = {"short": torch.zeros(N - 1, dtype=torch.int64, device=DEV), "float": torch.zeros(N, device=DEV),
             "bool": torch.zeros(N, dtype=torch.bool, device=DEV), "cpu": torch.zeros(N, dtype=torch.int64),
             "list": [0] * N}[bad]
    with pytest.raises(ValueError, match="group"):
        F_hip.embedding_monitor(z, k=2, group=group)


# ---- spcl_cell_majority
def _maps(N, H, W, C, seed):
    """label maps of smooth regions (so that majorities are not all alike) with a sprinkle of noise"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((N, H, W), dtype=np.uint8)
    for n in range(N):
        field = np.sin(yy / (3.0 + n) + g.uniform(0, 6)) + np.cos(xx / (4.0 + n) + g.uniform(0, 6))
        out[n] = np.clip(((field + 2.0) / 4.0 * C).astype(np.int64), 0, C - 1)
    noise = g.random((N, H, W)) < 0.1
    out[noise] = g.integers(0, C, int(noise.sum()))
    return out


def _majority(labels, C, grid):
    cell, purity = _F().cell_majority(torch.from_numpy(labels).to(DEV), C, grid)
    return cell.cpu().numpy(), purity.cpu().numpy()


@pytest.mark.parametrize("C", [2, 4, 16])
@pytest.mark.parametrize("N,H,W,grid", [(2, 224, 224, (10, 10)), (3, 20, 30, (4, 7)), (1, 7, 5, (7, 5))])
def test_cell_majority_is_exact(N, H, W, grid, C):
    labels = _maps(N, H, W, C, seed=H + C)
    want_label, want_purity = D.cell_majority(labels, C, grid)
    label, purity = _majority(labels, C, grid)
    assert label.dtype == np.int32 and purity.dtype == np.float32 and label.shape == purity.shape == (N,) + grid
    assert np.array_equal(label, want_label)
    assert purity.tobytes() == want_purity.tobytes()
    if grid == (H, W):  # cell = pixel
        assert np.array_equal(label, labels) and np.all(purity == 1.0)
    elif C >= 4:
        assert len(np.unique(label)) > 1
    # values >= C are counted for no class: with C - 1 classes the top class drops out of every count
    if C > 2:
        want_label, want_purity = D.cell_majority(labels, C - 1, grid)
        label, purity = _majority(labels, C - 1, grid)
        assert np.array_equal(label, want_label) and purity.tobytes() == want_purity.tobytes()


def test_cell_majority_windows_are_those_of_adaptive_avg_pool():
    # 224 -> 10 does not divide: the windows overlap (rows 22 and 44 lie in two cells each)
    assert D.windows(224, 10)[:3] == [(0, 23), (22, 45), (44, 68)]
    labels = _maps(2, 224, 224, 4, seed=9)
    onehot = torch.nn.functional.one_hot(torch.from_numpy(labels).long(), 4).permute(0, 3, 1, 2).double()
    share = torch.nn.functional.adaptive_avg_pool2d(onehot, (10, 10))
    _, purity = _majority(labels, 4, (10, 10))
    assert np.allclose(purity, share.max(1).values.numpy(), rtol=0, atol=1e-6)


def test_cell_majority_ties_out_of_range_values_and_refusals():
    F_hip = _F()
    labels = np.zeros((1, 8, 8), dtype=np.uint8)
    labels[0, :4, :4] = 3
    labels[0, 0:2, :4] = 1      # cell (0, 0): eight 1s and eight 3s -- half and half, the lower class
    labels[0, :4, 4:] = 200     # cell (0, 1): only out-of-range values
    labels[0, 4:, :4] = 2
    labels[0, 4:6, 0:2] = 9     # cell (1, 0): four values >= C, twelve 2s
    label, purity = _majority(labels, 4, (2, 2))
    assert label[0].tolist() == [[1, -1], [2, 0]]
    assert purity[0].tolist() == [[0.5, 0.0], [0.75, 1.0]]
    want_label, want_purity = D.cell_majority(labels, 4, (2, 2))
    assert np.array_equal(label, want_label) and np.array_equal(purity, want_purity)
    lt = torch.from_numpy(labels).to(DEV)
    cell, none = F_hip.cell_majority(lt, 4, (2, 2), purity=False)
    assert none is None and cell.cpu().numpy()[0].tolist() == [[1, -1], [2, 0]]
    for C, size in ((4, (9, 2)), (4, (2, 9)), (4, (0, 2)), (1, (2, 2)), (17, (2, 2)), (4, (2, 2, 2))):
        with pytest.raises(ValueError, match="cell_majority"):
            F_hip.cell_majority(lt, C, size)
    with pytest.raises(ValueError, match="uint8"):
        F_hip.cell_majority(lt.long(), 4, (2, 2))
    # and the library's own check, before any launch
    from spcl_amd import native
    out = torch.empty(1, 9, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="spcl_cell_majority: grid 9 x 2"):
        native.call("spcl_cell_majority", native.ptr(lt), 1, 8, 8, 4, 9, 2, native.ptr(out), None, native.stream())


# ---- teeth: what the leave-one-scan-out vote can and cannot be fooled by
def _rates(z, labels, group, k=5, C=4):
    got = _np(_call(z, labels[None], None, k, group))
    pred = got["pred"][0]
    assert got["correct"][0] == int((pred == labels).sum())
    return D.knn_class(pred, labels), D.knn_dice(pred, labels, C)


def test_teeth_class_rows_score_one_and_scan_rows_score_nothing_across_scans():
    N, scans, d = 256, 8, 16
    g = np.random.default_rng(31)
    scan = np.repeat(np.arange(scans), N // scans)
    # rows that encode only the class: the same score with and without groups
    cls = g.integers(0, 4, N)
    cls[:8] = [0, 1, 2, 3, 0, 1, 2, 3]
    z = (np.eye(4, d)[cls] * g.uniform(0.5, 2.0, (N, 1))).astype(np.float32)
    assert _rates(z, cls, None) == (1.0, 1.0)
    assert _rates(z, cls, scan) == (1.0, 1.0)
    # rows that encode only the scan, the class constant within a scan and different across scans: a perfect score that a
    # row's own scan hands it, and exactly nothing once that scan is left out
    cls = scan.astype(np.int64)
    z = (np.eye(scans, d)[scan] + 0.05 * g.standard_normal((N, d))).astype(np.float32)
    assert _rates(z, cls, None, C=scans) == (1.0, 1.0)
    assert _rates(z, cls, scan, C=scans) == (0.0, 0.0)
