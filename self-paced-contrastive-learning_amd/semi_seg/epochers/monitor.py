"""Pre-training monitor: a score for the pre-trained representation, computed on the device at epoch boundaries.  NOT in the
reference -- its ``InfoNCEPretrainMonitorEpocher`` dumps every projection with ``torch.save`` for a person to plot.

``EmbeddingMonitor`` keeps a FIXED set of slices of the pre-training store in two views (the `val` centre crop and ONE draw of
the data set's pre-train recipe, made once with a private generator and kept on the device), runs them through the encoder
in ``eval()`` mode and hands the embeddings of every contrastive hook on an encoder feature -- ``feature``: the global
average pool of the hooked map, ``projection``: the hook's projector output -- to ``functional.embedding_monitor`` (one call
per (hook, space); csrc/embed_monitor.hip): leave-one-out k-NN accuracy on the meta-labels the loss contrasts on, retrieval
of a slice's other view, alignment and uniformity.  Everything is read back once, at the end of ``run``."""
import random
import re

import torch

from ... import functional as F_hip
from ..arch.hook import SingleFeatureExtractor
from ..arch.unet import UNet, sort_arch
from ..data.augment import RecipeViews
from ..hooks.utils import contrast_kinds, get_label

SPACES = ("feature", "projection")
_METRICS = ("top1", "recall5", "align", "uniform", "min_norm")
LOWER_IS_BETTER = ("align", "uniform")
_KEY = re.compile(r"^[^/]+/(feature|projection)/(knn_[a-z]+|" + "|".join(_METRICS) + r")$")
MONITOR_DEFAULTS = {"every": 1, "k": 20, "max_slices": 512, "space": None, "select_by": None}


def parse_monitor(section):
    """the trainers' ``monitor=`` argument / the ``Monitor`` section of a config -> a dict of every key of
    ``MONITOR_DEFAULTS`` (``None`` / ``False`` -> ``None``: no monitor; ``True`` -> the defaults).  ``space``: None (both),
    "feature" or "projection"; ``select_by``: None (the first hook's ``projection/knn_patient``) or a key of the dict
    ``EmbeddingMonitor.run`` returns, ``<hook or feature>/<space>/<metric>``.  Anything else is a ``ValueError``."""
    if section is None or section is False:
        return None
    if section is True:
        section = {}
    if not isinstance(section, dict):
        raise ValueError(f"Monitor: expected a mapping, given {type(section).__name__}")
    unknown = sorted(set(section) - set(MONITOR_DEFAULTS))
    if unknown:
        raise ValueError(f"Monitor: unknown keys {unknown}; known: {sorted(MONITOR_DEFAULTS)}")
    out = dict(MONITOR_DEFAULTS, **section)
    for key, lo, hi in (("every", 1, None), ("k", 1, F_hip.EMBED_MONITOR_MAX_K),
                        ("max_slices", 1, F_hip.EMBED_MONITOR_MAX_N // 2)):
        v = out[key]
        if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
            raise ValueError(f"Monitor.{key} must be an integer in [{lo}, {hi if hi is not None else 'inf'}], given {v!r}")
    if out["space"] is not None and out["space"] not in SPACES:
        raise ValueError(f"Monitor.space must be one of {SPACES} or None, given {out['space']!r}")
    sel = out["select_by"]
    if sel is not None:
        if not isinstance(sel, str) or _KEY.match(sel) is None:
            raise ValueError(f"Monitor.select_by: {sel!r} is not a monitor key (<hook or feature>/<space>/<metric>, space in "
                             f"{SPACES}, metric knn_<label kind> or one of {_METRICS})")
        if out["space"] is not None and sel.split("/")[1] != out["space"]:
            raise ValueError(f"Monitor.select_by {sel!r} names a space that Monitor.space = {out['space']!r} leaves out")
    return out


def select_score(result, select_by):
    """(key, score) of a ``run`` result: the value under ``select_by`` (None: the first ``.../projection/knn_patient``, else
    the first ``knn_patient``), negated for the metrics where lower is better -- a larger score is an improvement.  A key
    the result does not hold is a ``ValueError``."""
    key = resolve_select_by([name for name in result if name != "skipped"], select_by)
    if key is None:
        raise ValueError("Monitor.select_by: the monitor reported no key to select by "
                         f"(skipped: {list(result.get('skipped', []))})")
    value = float(result[key])
    return key, -value if key.rsplit("/", 1)[1] in LOWER_IS_BETTER else value


def monitor_indices(n_store, max_slices):
    """``max_slices`` slice indices evenly spaced over the store's order (all of them when the store is smaller)"""
    m = min(int(max_slices), int(n_store))
    return [(i * n_store) // m for i in range(m)]


def monitor_store(source):
    """the pre-training store behind ``source`` (a loader's ``.dataset``, or the store itself); ``TypeError`` when there is none"""
    store = getattr(source, "dataset", source)
    if not hasattr(store, "images") or not hasattr(store, "meta"):
        raise TypeError("EmbeddingMonitor: expected a semi_seg.data.DeviceSliceStore (or a loader whose `.dataset` is one), "
                        f"got {type(store).__name__}")
    return store


def _contrastive_hooks(hooks):
    """the contrastive trainer hooks (those with a ``feature_name`` and a ``projector``) among ``hooks``, combined ones opened"""
    out = []
    for h in hooks:
        for sub in (h.hooks if hasattr(h, "hooks") else [h]):
            if hasattr(sub, "projector") and hasattr(sub, "feature_name"):
                out.append(sub)
    return out


def monitor_targets(hooks):
    """-> ([(prefix, feature name, projector)] of the hooks on encoder features, [names of the others]).  ``prefix`` is the
    feature's name in lower case, or the hook's name where several hooks tap one feature.  Host only."""
    subs, skipped = [], []
    for sub in _contrastive_hooks(hooks):
        (subs if sub.feature_name in UNet.encoder_names else skipped).append(sub)
    taps = [s.feature_name for s in subs]
    return ([(s.feature_name.lower() if taps.count(s.feature_name) == 1 else s.hook_name, s.feature_name, s.projector)
             for s in subs], [s.hook_name for s in skipped])


def expected_keys(model, hooks, data_name="acdc", space=None):
    """the keys ``EmbeddingMonitor.run`` will report for these hooks, without running anything (host only): what a trainer
    checks ``select_by`` against when it is initialised.  An embedding known to be wider than the kernel takes is left out,
    as ``run`` leaves it out."""
    targets, _ = monitor_targets(hooks)
    spaces = SPACES if space is None else (space,)
    metrics = [f"knn_{c}" for c in contrast_kinds(data_name) if c != "self"] + list(_METRICS)
    heads = []
    if "feature" in spaces:
        for f in sort_arch(list({f for _, f, _ in targets})):
            if model.get_channel_dim(f) <= F_hip.EMBED_MONITOR_MAX_D:
                heads.append(f.lower() + "/feature")
    if "projection" in spaces:
        for prefix, _, projector in targets:
            if (getattr(projector, "_output_dim", None) or 0) <= F_hip.EMBED_MONITOR_MAX_D:
                heads.append(prefix + "/projection")
    return [f"{h}/{m}" for h in heads for m in metrics]


def resolve_select_by(keys, select_by):
    """the key the trainer selects ``best.pth`` by, among the keys a run will report: ``select_by`` itself -- a ``ValueError``
    when the run cannot produce it --, or for ``None`` the first ``.../projection/knn_patient``, else the first
    ``knn_patient``, else ``None``: nothing to select by (no hook on an encoder feature), the monitor only records."""
    if select_by is not None:
        if select_by not in keys:
            raise ValueError(f"Monitor.select_by: {select_by!r} is not among the keys this monitor can report: "
                             f"{sorted(keys) if keys else 'none (no contrastive hook on an encoder feature)'}")
        return select_by
    for want in ("/projection/knn_patient", "/knn_patient"):
        key = next((name for name in keys if name.endswith(want)), None)
        if key is not None:
            return key
    return None


class EmbeddingMonitor:
    def __init__(self, source, *, max_slices=512, k=20, space=None, indices=None, out_hw=None, seed=0, batch_size=64):
        """``source``: the contrastive loader (its ``.dataset`` is the pre-training store) or the store itself.  ``indices``: the
        slice set of an earlier monitor (a resumed trainer), else ``monitor_indices``.  The pre-train view is drawn with
        ``random.Random(seed)``: the sampler's and the augmentation's streams stay where they were."""
        store = monitor_store(source)
        if space is not None and space not in SPACES:
            raise ValueError(f"EmbeddingMonitor: space must be one of {SPACES} or None, given {space!r}")
        views = getattr(source, "views", None)
        data_name = getattr(store, "data_name", "acdc")
        if not isinstance(views, RecipeViews):
            # (the legacy PretrainViews loader, a loader that builds its views with the first batch, a bare store): the data
            # set's pre-train recipe at the size the loader trains on
            name = "prostate_pretrain" if data_name == "prostate" else "acdc_pretrain"
            out_hw = tuple(out_hw or getattr(source, "out_hw", None) or (224, 224))
            views = RecipeViews(store.images, name, out_hw, resized_to=getattr(store, "resized_to", None))
        self.indices = [int(i) for i in indices] if indices is not None else monitor_indices(len(store), max_slices)
        if not 1 <= len(self.indices) <= F_hip.EMBED_MONITOR_MAX_N // 2 or any(not 0 <= i < len(store) for i in self.indices):
            raise ValueError(f"EmbeddingMonitor: {len(self.indices)} slice indices for a store of {len(store)} slices")
        self.k, self.spaces = int(k), SPACES if space is None else (space,)
        self._batch = int(batch_size)
        M = len(self.indices)
        plain = views.val(self.indices)
        plain = plain[0] if isinstance(plain, tuple) else plain
        drawn = views.apply(views.rows(self.indices, rng=random.Random(seed)))
        self.images = torch.cat([plain, drawn], dim=0)  # [2M, 1, oh, ow]: the `val` views, then the pre-train draws
        dev = self.images.device
        metas = [store.meta(i) for i in self.indices]
        partitions, scans = [m[1] for m in metas], [m[2] for m in metas]
        self.data_name = data_name
        self.kinds = [c for c in contrast_kinds(data_name) if c != "self"]  # ("self": every slice its own class -- no vote)
        rows = [get_label(c, data_name, partitions, scans) for c in self.kinds]
        self.labels = torch.tensor([list(r) + list(r) for r in rows], dtype=torch.int32, device=dev)  # [L, 2M]
        self.pair = ((torch.arange(2 * M, device=dev) + M) % (2 * M)).to(torch.int32)
        self.skipped = []

    def _targets(self, hooks):
        """[(prefix, feature name, projector)] of the hooks on encoder features; the others go to ``skipped``"""
        targets, self.skipped = monitor_targets(hooks)
        return targets

    def expected_keys(self, model, hooks):
        """the keys ``run`` will report for these hooks (host only)"""
        return expected_keys(model, hooks, self.data_name, None if len(self.spaces) == 2 else self.spaces[0])

    @torch.no_grad()
    def run(self, model, hooks):
        """-> a flat dict: ``<prefix>/<space>/knn_<kind>`` (leave-one-out k-NN accuracy, the row's other view left out of its
        neighbours), ``/top1`` and ``/recall5`` (the other view among all other rows), ``/align``, ``/uniform``, ``/min_norm``,
        and ``skipped``: the names of the dense (decoder) hooks.  ``<prefix>`` is the feature's name in lower case, or the
        hook's name where several hooks tap one feature (``feature`` is then reported once, under the feature's name)."""
        targets = self._targets(hooks)
        modules = [model] + [p for _, _, p in targets]
        was_training = [m.training for m in modules]
        calls = []  # (key prefix, EmbeddingMonitorResult)
        try:
            for m in modules:
                m.eval()
            if targets:
                names = sort_arch(list({f for _, f, _ in targets}))
                until = names[-1]
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
                            if "feature" in self.spaces:
                                pooled[f].append(F_hip.adaptive_pool2d(feature, (1, 1), "avg").flatten(1).float())
                            if "projection" in self.spaces:
                                for prefix, g, projector in targets:
                                    if g == f:
                                        projected[prefix].append(projector(feature).flatten(1).float())
                            e.clear()
                finally:
                    for e in extractors.values():
                        e.remove()
                spaces = [(f.lower() + "/feature", torch.cat(rows)) for f, rows in pooled.items() if rows]
                spaces += [(prefix + "/projection", torch.cat(rows)) for prefix, rows in projected.items() if rows]
                for key, z in spaces:
                    if z.shape[1] > F_hip.EMBED_MONITOR_MAX_D:
                        self.skipped.append(key)
                        continue
                    calls.append((key, F_hip.embedding_monitor(z, self.labels, self.pair, k=self.k, exclude_pair=True)))
        finally:
            for m, flag in zip(modules, was_training):
                m.train(flag)
        out = {}
        if calls:
            N, L = self.pair.numel(), len(self.kinds)
            packed = []
            for _, r in calls:
                ranks = r.pair_rank
                packed.append(torch.cat([r.correct.double() / N, r.scalars,
                                         torch.stack([(ranks == 0).sum(), ((ranks >= 0) & (ranks < 5)).sum()]).double()]))
            host = torch.stack(packed).cpu().tolist()  # the one read-back
            for (key, _), row in zip(calls, host):
                for kind, v in zip(self.kinds, row[:L]):
                    out[f"{key}/knn_{kind}"] = v
                align, uniform, n_pairs, min_norm, top1, recall5 = row[L:]
                out[f"{key}/top1"], out[f"{key}/recall5"] = top1 / n_pairs, recall5 / n_pairs
                out[f"{key}/align"], out[f"{key}/uniform"], out[f"{key}/min_norm"] = align, uniform, min_norm
        out["skipped"] = list(self.skipped)
        return out
