"""Float64 restatement of ``spcl_embed_monitor_grouped`` and integer restatement of ``spcl_cell_majority``
(csrc/embed_monitor.hip) by brute force, on top of tests/_embed_monitor_oracle.py: the candidate rule with groups, the same
stable order and vote, the same tie-independent comparison at tol = (d + 8) 2^-24.  numpy only; nothing here touches the
device."""
import contextlib

import numpy as np

from tests import _embed_monitor_oracle as O

tol = O.tol
_plain_candidates = O.candidates  # (bound once: `check` below lends that module the grouped rule for the length of a call)


def candidates(N, pair, exclude_pair, group=None):
    """bool [N, N]: j is a candidate of row i -- all j != i, with exclude_pair j != pair[i], and with group[i] >= 0 also
    group[j] != group[i] (a negative id: ungrouped, nothing more is left out for that row)"""
    c = _plain_candidates(N, pair, exclude_pair)
    if group is not None:
        group = np.asarray(group, dtype=np.int64)
        same = (group[:, None] == group[None, :]) & (group[:, None] >= 0)
        c &= ~same
    return c


def embed_monitor_grouped(z, labels=None, pair=None, k=20, exclude_pair=True, group=None):
    """the whole grouped call in float64: ``O.embed_monitor`` with the neighbour lists, votes and counts redone under the
    grouped candidate rule (uniformity, alignment, pair_rank and min_norm do not see the groups)"""
    r = O.embed_monitor(z, labels, pair, k, exclude_pair)
    if group is None:
        return r
    s = r["s"]
    N = s.shape[0]
    pair = None if pair is None else np.asarray(pair, dtype=np.int64)
    cand = candidates(N, pair, exclude_pair, group)
    knn_idx = np.full((N, k), -1, dtype=np.int64)
    knn_sim = np.full((N, k), -np.inf)
    for i in range(N):
        js = np.nonzero(cand[i])[0]
        order = js[np.lexsort((js, -s[i, js]))][:k]  # by -s, then by index
        knn_idx[i, :len(order)] = order
        knn_sim[i, :len(order)] = s[i, order]
    pred, correct = O.predictions(knn_idx, labels)
    return dict(r, knn_idx=knn_idx, knn_sim=knn_sim, pred=pred, correct=correct)


@contextlib.contextmanager
def _grouped_candidates(group):
    """``O.check`` asks its module's ``candidates`` who may be a neighbour: for the length of one check that is the grouped
    rule above (the file itself stays as it is; every tolerance and every other assertion is the one it states)"""
    O.candidates = lambda N, pair, exclude_pair: candidates(N, pair, exclude_pair, group)
    try:
        yield
    finally:
        O.candidates = _plain_candidates


def check(result, z, labels=None, pair=None, k=20, exclude_pair=True, group=None, ref=None):
    """``O.check`` under the grouped candidate rule, plus the exact statement on ``knn_idx``: no returned neighbour shares
    its row's non-negative group"""
    with _grouped_candidates(group):
        O.check(result, z, labels, pair, k, exclude_pair, ref=ref)
    if group is not None:
        group = np.asarray(group, dtype=np.int64)
        idx = np.asarray(result["knn_idx"]).astype(np.int64)
        valid = idx >= 0
        rows = np.repeat(np.arange(idx.shape[0]), idx.shape[1]).reshape(idx.shape)
        gi, gj = group[rows[valid]], group[idx[valid]]
        assert not np.any((gi >= 0) & (gi == gj)), "a neighbour shares its row's group"


# ---- spcl_cell_majority
def windows(size, cells):
    """[(start, stop)] of nn.AdaptiveAvgPool2d's windows along one axis: floor(u size / cells) .. ceil((u + 1) size / cells)"""
    return [((u * size) // cells, -((-(u + 1) * size) // cells)) for u in range(cells)]


def cell_majority(labels, C, grid):
    """-> (cell_label [N, sh, sw] int64, purity [N, sh, sw] float32) by integer window counts: the class below C with the
    largest count, equal counts to the lower class; values >= C are counted for no class, a window of only such values gets
    -1 and purity 0; purity = float32(count) / float32(window size)"""
    labels = np.asarray(labels)
    N, H, W = labels.shape
    sh, sw = grid
    assert 1 <= sh <= H and 1 <= sw <= W
    out = np.full((N, sh, sw), -1, dtype=np.int64)
    purity = np.zeros((N, sh, sw), dtype=np.float32)
    for n in range(N):
        for u, (r0, r1) in enumerate(windows(H, sh)):
            for v, (c0, c1) in enumerate(windows(W, sw)):
                win = labels[n, r0:r1, c0:c1].ravel().astype(np.int64)
                counts = np.bincount(win[win < C], minlength=C)
                if counts.max() > 0:
                    best = int(np.argmax(counts))  # (the first of equal maxima: the lower class)
                    out[n, u, v] = best
                    purity[n, u, v] = np.float32(counts[best]) / np.float32(win.size)
    return out, purity


# ---- the monitor's two rates, from predictions and labels
def knn_class(pred, labels):
    return float(np.mean(np.asarray(pred) == np.asarray(labels)))


def knn_dice(pred, labels, C):
    """the mean over the foreground classes 1 .. C-1 that occur among the labels of 2 |P & T| / (|P| + |T|)"""
    pred, labels = np.asarray(pred), np.asarray(labels)
    scores = []
    for c in range(1, C):
        t = labels == c
        if t.any():
            p = pred == c
            scores.append(2.0 * (p & t).sum() / (p.sum() + t.sum()))
    return float(np.mean(scores)) if scores else float("nan")
