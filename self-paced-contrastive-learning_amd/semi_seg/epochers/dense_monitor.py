"""Dense pre-training monitor: a score for decoder pre-training (``main_pretrain_decoder.py``, ``_INFONCEDenseHook``,
``DenseProjectionHead``), the stage ``monitor.py`` names in ``skipped`` and leaves blind.  NOT in the reference.

``DenseEmbeddingMonitor`` keeps a FIXED set of slices of the pre-training store as their `val` views (centre crop) WITH their
label maps, runs them through the network in ``eval()`` mode up to the deepest hooked decoder feature, and scores the local
embeddings of every contrastive hook on a decoder feature -- ``dense_projection``: the hook's ``DenseProjectionHead`` output,
``dense_feature``: the adaptive average pool of the hooked map on the same grid -- by pixel-level k-NN classification: does a
cell's neighbourhood IN OTHER SCANS carry the same anatomical class?  A cell's class is the majority class of its pooling
window (``functional.cell_majority``); its own scan (or slice) is left out of its candidates
(``functional.embedding_monitor(group=...)``): the 100 cells of a slice and those of the neighbouring slices are near-duplicates
of each other, and a leave-one-row-out vote among them measures nothing.  One call per (hook, space); everything is read back
once, at the end of ``run``."""
import re

import torch

from ... import functional as F_hip
from ..arch.hook import SingleFeatureExtractor
from ..arch.unet import UNet, sort_arch
from ..data.augment import RecipeViews
from .monitor import _contrastive_hooks, monitor_indices, monitor_store

DENSE_SPACES = ("dense_feature", "dense_projection")
DENSE_METRICS = ("knn_class", "knn_dice", "uniform", "min_norm")
DENSE_LOWER_IS_BETTER = ("uniform",)
EXCLUDES = ("scan", "slice")
_KEY = re.compile(r"^[^/]+/(" + "|".join(DENSE_SPACES) + r")/(" + "|".join(DENSE_METRICS) + r")$")
DENSE_MONITOR_DEFAULTS = {"every": 1, "k": 20, "max_slices": 512, "space": None, "exclude": "scan", "select_by": None}


def parse_dense_monitor(section):
    """the trainers' ``dense_monitor=`` argument / the ``DenseMonitor`` section of a config -> a dict of every key of
    ``DENSE_MONITOR_DEFAULTS`` (``None`` / ``False`` -> ``None``: no dense monitor; ``True`` -> the defaults).  ``space``: None
    (both), "dense_feature" or "dense_projection"; ``exclude``: "scan" (a cell's candidates leave out its whole scan) or
    "slice"; ``select_by``: None (the first hook's ``dense_projection/knn_dice``), a key of the dict
    ``DenseEmbeddingMonitor.run`` returns, or ``False``: record, select nothing.  Anything else is a ``ValueError``."""
    if section is None or section is False:
        return None
    if section is True:
        section = {}
    if not isinstance(section, dict):
        raise ValueError(f"DenseMonitor: expected a mapping, given {type(section).__name__}")
    unknown = sorted(set(section) - set(DENSE_MONITOR_DEFAULTS))
    if unknown:
        raise ValueError(f"DenseMonitor: unknown keys {unknown}; known: {sorted(DENSE_MONITOR_DEFAULTS)}")
    out = dict(DENSE_MONITOR_DEFAULTS, **section)
    for key, lo, hi in (("every", 1, None), ("k", 1, F_hip.EMBED_MONITOR_MAX_K), ("max_slices", 1, F_hip.EMBED_MONITOR_MAX_N)):
        v = out[key]
        if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
            raise ValueError(f"DenseMonitor.{key} must be an integer in [{lo}, {hi if hi is not None else 'inf'}], given {v!r}")
    if out["space"] is not None and out["space"] not in DENSE_SPACES:
        raise ValueError(f"DenseMonitor.space must be one of {DENSE_SPACES} or None, given {out['space']!r}")
    if out["exclude"] not in EXCLUDES:
        raise ValueError(f"DenseMonitor.exclude must be one of {EXCLUDES}, given {out['exclude']!r}")
    sel = out["select_by"]
    if sel is not None and sel is not False:
        if not isinstance(sel, str) or _KEY.match(sel) is None:
            raise ValueError(f"DenseMonitor.select_by: {sel!r} is not a dense monitor key (<hook or feature>/<space>/<metric>, "
                             f"space in {DENSE_SPACES}, metric one of {DENSE_METRICS}) nor false")
        if out["space"] is not None and sel.split("/")[1] != out["space"]:
            raise ValueError(f"DenseMonitor.select_by {sel!r} names a space that DenseMonitor.space = {out['space']!r} leaves out")
    return out


def _grid(projector):
    """the (sh, sw) a hook's ``DenseProjectionHead`` pools to"""
    size = getattr(projector, "_spatial_size", (1, 1))
    return (int(size[0]), int(size[1]))


def dense_targets(hooks):
    """-> [(prefix, feature name, projector)] of the contrastive hooks on DECODER features: exactly the hooks
    ``monitor_targets`` reports as skipped.  ``prefix`` by its rule: the feature's name in lower case, or the hook's name where
    several hooks tap one feature.  Host only."""
    subs = [s for s in _contrastive_hooks(hooks) if s.feature_name not in UNet.encoder_names]
    taps = [s.feature_name for s in subs]
    return [(s.feature_name.lower() if taps.count(s.feature_name) == 1 else s.hook_name, s.feature_name, s.projector)
            for s in subs]


def dense_slices(hooks, max_slices):
    """M_d = min(max_slices, EMBED_MONITOR_MAX_N // (sh sw)), with the largest grid among the hooks: every (hook, space) fits
    one kernel call"""
    cells = max([g[0] * g[1] for g in (_grid(p) for _, _, p in dense_targets(hooks))] or [1])
    return max(1, min(int(max_slices), F_hip.EMBED_MONITOR_MAX_N // cells))


def expected_keys(model, hooks, space=None):
    """the keys ``DenseEmbeddingMonitor.run`` will report for these hooks, without running anything (host only): what a
    trainer checks ``select_by`` against in ``init()``.  An embedding known to be wider than the kernel takes is left out, as
    ``run`` leaves it out (into ``skipped``)."""
    targets = dense_targets(hooks)
    spaces = DENSE_SPACES if space is None else (space,)
    heads = []
    if "dense_feature" in spaces:
        for f in sort_arch(list({f for _, f, _ in targets})):
            if model.get_channel_dim(f) <= F_hip.EMBED_MONITOR_MAX_D:
                heads.append(f.lower() + "/dense_feature")
    if "dense_projection" in spaces:
        for prefix, _, projector in targets:
            if (getattr(projector, "_output_dim", None) or 0) <= F_hip.EMBED_MONITOR_MAX_D:
                heads.append(prefix + "/dense_projection")
    return [f"{h}/{m}" for h in heads for m in DENSE_METRICS]


def resolve_select_by(keys, select_by):
    """the key the trainer selects ``best.pth`` by, among the keys a run will report: ``select_by`` itself -- a ``ValueError``
    when the run cannot produce it --, for ``None`` the first ``.../dense_projection/knn_dice``, else the first ``knn_dice``,
    else ``None``; ``False``: ``None``, the monitor only records."""
    if select_by is False:
        return None
    if select_by is not None:
        if select_by not in keys:
            raise ValueError(f"DenseMonitor.select_by: {select_by!r} is not among the keys this monitor can report: "
                             f"{sorted(keys) if keys else 'none (no contrastive hook on a decoder feature)'}")
        return select_by
    for want in ("/dense_projection/knn_dice", "/knn_dice"):
        key = next((name for name in keys if name.endswith(want)), None)
        if key is not None:
            return key
    return None


def dice_from_confusion(conf):
    """``conf[t][p]``: rows labelled t and predicted p (column C: no prediction) -> the mean over the foreground classes
    1 .. C-1 that occur among the labels of 2 |P & T| / (|P| + |T|); NaN when no foreground class occurs"""
    C = len(conf)
    scores = []
    for c in range(1, C):
        t = sum(conf[c])
        if t > 0:
            p = sum(conf[r][c] for r in range(C))
            scores.append(2.0 * conf[c][c] / (p + t))
    return sum(scores) / len(scores) if scores else float("nan")


class DenseEmbeddingMonitor:
    def __init__(self, source, hooks, *, max_slices=512, k=20, space=None, exclude="scan", indices=None, num_classes=None,
                 out_hw=None, batch_size=32):
        """``source``: the contrastive loader (its ``.dataset`` is the pre-training store) or the store itself; the store must
        have ``targets`` (``ValueError`` otherwise).  ``hooks``: the trainer's hooks (their grids size the slice set).
        ``indices``: the slice set of an earlier monitor (a resumed trainer), else ``monitor_indices(len(store), M_d)``.
        ``num_classes``: C of the label maps, by default their largest code + 1 (one read-back, here and never again).  No
        random stream is touched: the `val` view draws nothing."""
        store = monitor_store(source)
        if getattr(store, "targets", None) is None:
            raise ValueError("DenseEmbeddingMonitor: the store has no label maps (DeviceSliceStore(..., targets=)); the dense "
                             "monitor votes on the classes of its `val` views")
        if space is not None and space not in DENSE_SPACES:
            raise ValueError(f"DenseEmbeddingMonitor: space must be one of {DENSE_SPACES} or None, given {space!r}")
        if exclude not in EXCLUDES:
            raise ValueError(f"DenseEmbeddingMonitor: exclude must be one of {EXCLUDES}, given {exclude!r}")
        m_d = dense_slices(hooks, max_slices)
        self.indices = [int(i) for i in indices] if indices is not None else monitor_indices(len(store), m_d)
        if not 1 <= len(self.indices) <= F_hip.EMBED_MONITOR_MAX_N or any(not 0 <= i < len(store) for i in self.indices):
            raise ValueError(f"DenseEmbeddingMonitor: {len(self.indices)} slice indices for a store of {len(store)} slices")
        self.k, self.spaces, self.exclude = int(k), DENSE_SPACES if space is None else (space,), exclude
        self._batch = int(batch_size)
        views = getattr(source, "views", None)
        out_hw = tuple(out_hw or getattr(views, "out_hw", None) or getattr(source, "out_hw", None) or (224, 224))
        resize = views.recipe.get("resize") if isinstance(views, RecipeViews) else None
        # a RecipeViews of its own, as ScanBatchLoader builds it: the `val` transform of image and label map
        val = RecipeViews(store.images, dict(degrees=0.0, flips=False, pad=0, crop_first=True, brightness=None, contrast=None,
                                             resize=resize), out_hw, labels=store.targets,
                          resized_to=getattr(store, "resized_to", None))
        images, targets = val.val(self.indices)
        self.images = images                                      # [M, 1, oh, ow]
        self.targets = targets[:, 0].to(torch.uint8).contiguous()  # [M, oh, ow]
        if num_classes is None:
            num_classes = max(2, int(self.targets.max()) + 1)
        if not 2 <= int(num_classes) <= F_hip.CELL_MAJORITY_MAX_C:
            raise ValueError(f"DenseEmbeddingMonitor: {num_classes} classes (2 .. {F_hip.CELL_MAJORITY_MAX_C})")
        self.num_classes = int(num_classes)
        scans = [store.meta(i)[2] for i in self.indices]
        order = {name: n for n, name in enumerate(sorted(set(scans)))}
        dev = self.images.device
        self._slice_group = {"scan": torch.tensor([order[s] for s in scans], dtype=torch.int32, device=dev),
                             "slice": torch.arange(len(scans), dtype=torch.int32, device=dev)}[exclude]
        self._grids = {}  # (sh, sw) -> (cell labels [M sh sw] int32, groups [M sh sw] int32), rows in (slice, u, v) order
        self.skipped = []

    def cells(self, grid):
        """(labels, groups) of the rows of one grid: ``cell_majority`` of the label maps, the slice's scan (or the slice)"""
        grid = (int(grid[0]), int(grid[1]))
        if grid not in self._grids:
            label, _ = F_hip.cell_majority(self.targets, self.num_classes, grid, purity=False)
            self._grids[grid] = (label.flatten(), self._slice_group.repeat_interleave(grid[0] * grid[1]))
        return self._grids[grid]

    def expected_keys(self, model, hooks):
        """the keys ``run`` will report for these hooks (host only)"""
        return expected_keys(model, hooks, None if len(self.spaces) == 2 else self.spaces[0])

    @torch.no_grad()
    def run(self, model, hooks):
        """-> a flat dict: ``<prefix>/<space>/knn_class`` (the share of cells whose k-NN vote among OTHER scans' cells is
        their class), ``/knn_dice`` (the mean over the foreground classes among the cell labels of 2 |P & T| / (|P| + |T|),
        P, T the cells predicted as / labelled with the class), ``/uniform``, ``/min_norm``, and ``skipped``.  ``<prefix>`` is
        the feature's name in lower case, or the hook's name where several hooks tap one feature (``dense_feature`` is then
        reported once, under the feature's name, on the first of those hooks' grids)."""
        targets = dense_targets(hooks)
        self.skipped = []
        modules = [model] + [p for _, _, p in targets]
        was_training = [m.training for m in modules]
        calls = []  # (key, EmbeddingMonitorResult, labels)
        try:
            for m in modules:
                m.eval()
            if targets:
                names = sort_arch(list({f for _, f, _ in targets}))
                until = names[-1]
                grid_of = {}
                for _, f, projector in targets:
                    grid_of.setdefault(f, _grid(projector))
                extractors = {f: SingleFeatureExtractor(model, f) for f in names}
                pooled, projected = {f: [] for f in names}, {prefix: [] for prefix, _, _ in targets}
                for e in extractors.values():
                    e.bind()
                try:
                    for chunk in self.images.split(self._batch):
                        for e in extractors.values():
                            e.clear()
                            e.set_enable(True)
                        model(chunk, until=until)
                        for f, e in extractors.items():
                            e.set_enable(False)
                            feature = e.feature()
                            if "dense_feature" in self.spaces:
                                pooled[f].append(self._rows(F_hip.adaptive_pool2d(feature, grid_of[f], "avg")))
                            if "dense_projection" in self.spaces:
                                for prefix, g, projector in targets:
                                    if g == f:
                                        projected[prefix].append(self._rows(projector(feature)))
                            e.clear()
                finally:
                    for e in extractors.values():
                        e.remove()
                spaces = [(f.lower() + "/dense_feature", grid_of[f], torch.cat(rows)) for f, rows in pooled.items() if rows]
                spaces += [(prefix + "/dense_projection", _grid(projector), torch.cat(projected[prefix]))
                           for prefix, _, projector in targets if projected[prefix]]
                M = len(self.indices)
                for key, grid, z in spaces:
                    if z.shape[1] > F_hip.EMBED_MONITOR_MAX_D or z.shape[0] != M * grid[0] * grid[1] or \
                            not 2 <= z.shape[0] <= F_hip.EMBED_MONITOR_MAX_N:
                        self.skipped.append(key)
                        continue
                    labels, groups = self.cells(grid)
                    calls.append((key, F_hip.embedding_monitor(z, labels, None, k=self.k, group=groups), labels))
        finally:
            for m, flag in zip(modules, was_training):
                m.train(flag)
        out = {}
        if calls:
            C = self.num_classes
            packed = []
            for _, r, labels in calls:
                pred = r.pred[0].long()
                # the confusion counts, on the device: conf[t][p], column C for a row without a neighbour
                conf = torch.bincount(labels.long() * (C + 1) + torch.where(pred < 0, torch.full_like(pred, C), pred),
                                      minlength=C * (C + 1))
                packed.append(torch.cat([r.correct.double() / labels.numel(), r.scalars, conf.double()]))
            host = torch.stack(packed).cpu().tolist()  # the one read-back
            for (key, _, _), row in zip(calls, host):
                conf = [[int(v) for v in row[5 + t * (C + 1):5 + (t + 1) * (C + 1)]] for t in range(C)]
                out[f"{key}/knn_class"], out[f"{key}/knn_dice"] = row[0], dice_from_confusion(conf)
                out[f"{key}/uniform"], out[f"{key}/min_norm"] = row[2], row[4]
        out["skipped"] = list(self.skipped)
        return out

    @staticmethod
    def _rows(maps):
        """[B, d, sh, sw] -> [B sh sw, d] f32 rows in (slice, u, v) order"""
        return maps.float().permute(0, 2, 3, 1).reshape(-1, maps.shape[1])
