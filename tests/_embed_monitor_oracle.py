"""Float64 restatement of ``spcl_embed_monitor`` (csrc/embed_monitor.hip) by brute force: the full similarity matrix, a stable
argsort on (-s, index) and the vote rule, plus the tie-independent comparison the GPU tests run (a similarity computed in f32
cannot be compared with the float64 one by neighbour identity: seeded clustered rows have top-k gaps down to 1e-8).  numpy
only; nothing here touches the device."""
import numpy as np


def tol(d):
    """the forward error bound of a length-d f32 fma chain on unit rows, plus the normalisation's roundings"""
    return (d + 8) * 2.0 ** -24


def similarity(z):
    """-> (s [N, N] float64 of the rows normalised as F.normalize, norms [N])"""
    z = np.asarray(z, dtype=np.float64)
    norms = np.sqrt((z * z).sum(1))
    zh = z / np.maximum(norms, 1e-12)[:, None]
    return zh @ zh.T, norms


def candidates(N, pair, exclude_pair):
    """bool [N, N]: j is a candidate of row i"""
    c = ~np.eye(N, dtype=bool)
    if exclude_pair and pair is not None:
        rows = np.nonzero(pair >= 0)[0]
        c[rows, pair[rows]] = False
    return c


def vote(neighbour_labels):
    """the majority label of a rank-ordered list; equal counts go to the label whose best-ranked neighbour comes first;
    -1 for an empty list"""
    best, best_count = -1, 0
    seen = []
    for v in neighbour_labels:
        v = int(v)
        if v in seen:
            continue
        seen.append(v)
        count = sum(1 for u in neighbour_labels if int(u) == v)
        if count > best_count:  # (strict: a later label with the same count never takes over)
            best, best_count = v, count
    return best


def predictions(knn_idx, labels):
    """-> (pred [L, N], correct [L]) from a neighbour table (-1 = no neighbour) and labels [L, N]"""
    labels = np.asarray(labels).reshape(-1, knn_idx.shape[0]) if labels is not None else np.zeros((0, knn_idx.shape[0]), int)
    pred = np.full(labels.shape, -1, dtype=np.int64)
    for l in range(labels.shape[0]):
        for i in range(knn_idx.shape[0]):
            nb = knn_idx[i][knn_idx[i] >= 0]
            pred[l, i] = vote(labels[l][nb])
    return pred, (pred == labels).sum(1)


def embed_monitor(z, labels=None, pair=None, k=20, exclude_pair=True):
    """the whole call in float64 -> dict(s, norms, knn_idx, knn_sim, pred, correct, pair_rank, alignment, uniform_mean,
    uniformity, n_pairs, min_norm)"""
    s, norms = similarity(z)
    N = s.shape[0]
    pair = None if pair is None else np.asarray(pair, dtype=np.int64)
    cand = candidates(N, pair, exclude_pair)
    knn_idx = np.full((N, k), -1, dtype=np.int64)
    knn_sim = np.full((N, k), -np.inf)
    for i in range(N):
        js = np.nonzero(cand[i])[0]
        order = js[np.lexsort((js, -s[i, js]))][:k]  # by -s, then by index
        knn_idx[i, :len(order)] = order
        knn_sim[i, :len(order)] = s[i, order]
    pred, correct = predictions(knn_idx, labels)
    pair_rank = np.full(N, -1, dtype=np.int64)
    align = []
    if pair is not None:
        for i in np.nonzero(pair >= 0)[0]:
            p = pair[i]
            others = np.array([j for j in range(N) if j != i and j != p], dtype=np.int64)
            so = s[i, others]
            pair_rank[i] = int(((so > s[i, p]) | ((so == s[i, p]) & (others < p))).sum())
            align.append(2.0 - 2.0 * s[i, p])
    off = ~np.eye(N, dtype=bool)
    umean = np.exp(-4.0 * (1.0 - s[off])).mean()
    return dict(s=s, norms=norms, knn_idx=knn_idx, knn_sim=knn_sim, pred=pred, correct=correct, pair_rank=pair_rank,
                alignment=float(np.mean(align)) if align else float("nan"), uniform_mean=float(umean),
                uniformity=float(np.log(umean)), n_pairs=len(align), min_norm=float(norms.min()))


def check(result, z, labels=None, pair=None, k=20, exclude_pair=True, ref=None):
    """assert a device result (numpy arrays: knn_idx, knn_sim, pred, correct, pair_rank, scalars) against the float64
    restatement without comparing neighbour identities.  ``ref``: (s, norms) of ``similarity(z)`` computed before."""
    z = np.asarray(z)
    N, d = z.shape
    t = tol(d)
    s, norms = similarity(z) if ref is None else ref
    pair = None if pair is None else np.asarray(pair, dtype=np.int64)
    cand = candidates(N, pair, exclude_pair)
    idx, sim = np.asarray(result["knn_idx"]).astype(np.int64), np.asarray(result["knn_sim"]).astype(np.float64)
    assert idx.shape == sim.shape == (N, k)
    n_cand = cand.sum(1)
    valid = idx >= 0
    # the valid entries are a prefix of min(k, candidates) entries; the tail is -1 / -inf
    assert np.array_equal(valid.sum(1), np.minimum(k, n_cand))
    assert np.array_equal(valid, np.arange(k)[None, :] < valid.sum(1)[:, None])
    assert np.all(np.isneginf(sim[~valid])) and np.all(idx[~valid] == -1)
    assert idx.max() < N
    rows = np.repeat(np.arange(N), k).reshape(N, k)
    s_at = np.where(valid, s[rows, np.where(valid, idx, 0)], np.nan)
    assert np.all(cand[rows[valid], idx[valid]]), "a neighbour is not a candidate"
    taken = np.zeros((N, N), dtype=bool)
    taken[rows[valid], idx[valid]] = True
    assert np.array_equal(taken.sum(1), valid.sum(1)), "a neighbour is listed twice"
    # |knn_sim - s64| <= tol
    err = np.abs(sim[valid] - s_at[valid])
    assert err.size == 0 or err.max() <= t, (err.max(), t)
    # the set is valid: its smallest s64 >= the largest s64 of the candidates left out - 2 tol
    lo = np.where(valid, s_at, np.inf).min(1)
    left = cand & ~taken
    hi = np.where(left, s, -np.inf).max(1)
    assert np.all(lo >= hi - 2 * t), float((hi - lo).max())
    # the order is non-increasing within 2 tol
    both = valid[:, 1:] & valid[:, :-1]
    step = (s_at[:, 1:] - s_at[:, :-1])[both]
    assert step.size == 0 or step.max() <= 2 * t, step.max()
    # pred and correct from the kernel's OWN neighbours, exactly
    L = 0 if labels is None else np.asarray(labels).reshape(-1, N).shape[0]
    if L:
        pred, correct = predictions(idx, labels)
        assert np.array_equal(np.asarray(result["pred"]).astype(np.int64), pred)
        assert np.array_equal(np.asarray(result["correct"]).astype(np.int64), correct)
    else:
        assert np.asarray(result["pred"]).shape == (0, N) and np.asarray(result["correct"]).shape == (0,)
    # pair_rank between the strict and the loose count
    rank = np.asarray(result["pair_rank"]).astype(np.int64)
    scalars = np.asarray(result["scalars"], dtype=np.float64)
    paired = np.zeros(N, dtype=bool) if pair is None else pair >= 0
    assert np.all(rank[~paired] == -1)
    if paired.any():
        pi = np.nonzero(paired)[0]
        sp = s[pi, pair[pi]]
        others = np.ones((len(pi), N), dtype=bool)
        others[np.arange(len(pi)), pi] = False
        others[np.arange(len(pi)), pair[pi]] = False
        lo_r = ((s[pi] > sp[:, None] + 2 * t) & others).sum(1)
        hi_r = ((s[pi] >= sp[:, None] - 2 * t) & others).sum(1)
        assert np.all((rank[pi] >= lo_r) & (rank[pi] <= hi_r))
        assert abs(scalars[0] - np.mean(2.0 - 2.0 * sp)) <= 2 * t, (scalars[0], np.mean(2.0 - 2.0 * sp))
    else:
        assert np.isnan(scalars[0])
    assert scalars[2] == paired.sum()
    umean = np.exp(-4.0 * (1.0 - s[~np.eye(N, dtype=bool)])).mean()
    assert abs(np.exp(scalars[1]) - umean) <= (4 * t + 1e-6) * umean, (np.exp(scalars[1]), umean)
    mn = norms.min()
    assert abs(scalars[3] - mn) <= 4 * float(np.spacing(np.float32(mn))), (scalars[3], mn)
