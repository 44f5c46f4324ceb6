"""CPU-only side of the dense pre-training monitor: the oracle of tests/_dense_monitor_oracle.py on hand-worked cases, the
``DenseMonitor`` config section, which keys a trainer can select by (decided from the hooks alone), the refusals of
``init()`` that need no device, and the C ABI's entries."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _dense_monitor_oracle as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "spcl_hip.h")
METRICS = ["knn_class", "knn_dice", "uniform", "min_norm"]


# ---- the oracle
def test_oracle_grouped_candidates_on_hand_worked_rows():
    ang = np.deg2rad(np.array([0.0, 5.0, 11.0, 15.0, 20.0, 26.0]))
    z = np.stack([np.cos(ang), np.sin(ang)], 1)
    labels = np.array([[0, 0, 1, 1, 2, 2]])
    group = np.array([0, 0, 1, 1, -1, -3])
    r = D.embed_monitor_grouped(z, labels, None, k=3, group=group)
    # rows 0, 1 leave each other out, rows 2, 3 too; rows 4 and 5 (negative ids) leave out nothing but themselves
    assert r["knn_idx"].tolist() == [[2, 3, 4], [2, 3, 4], [1, 4, 0], [4, 1, 5], [3, 5, 2], [4, 3, 2]]
    assert r["pred"].tolist() == [[1, 1, 0, 2, 1, 1]] and r["correct"].tolist() == [0]
    assert D.O.embed_monitor(z, labels, None, k=3)["correct"].tolist() == [2]  # (what the near-duplicates hand a row)
    plain = D.O.embed_monitor(z, labels, None, k=3)
    assert r["uniformity"] == plain["uniformity"] and r["min_norm"] == plain["min_norm"]  # groups do not enter them
    assert D.embed_monitor_grouped(z, labels, None, k=3, group=None)["knn_idx"].tolist() == plain["knn_idx"].tolist()
    everyone = D.embed_monitor_grouped(z, labels, None, k=2, group=np.zeros(6, dtype=int))
    assert np.all(everyone["knn_idx"] == -1) and everyone["pred"].tolist() == [[-1] * 6] and everyone["correct"].tolist() == [0]
    got = dict(knn_idx=r["knn_idx"], knn_sim=r["knn_sim"], pred=r["pred"], correct=r["correct"], pair_rank=r["pair_rank"],
               scalars=np.array([r["alignment"], r["uniformity"], r["n_pairs"], r["min_norm"]]))
    D.check(got, z, labels, None, 3, True, group)
    bad = dict(got, knn_idx=got["knn_idx"].copy())
    bad["knn_idx"][0, 0] = 1  # the nearest row of all -- but of row 0's own group
    with pytest.raises(AssertionError):
        D.check(bad, z, labels, None, 3, True, group)
    assert D.O.candidates(6, None, True).sum() == 30  # (the check leaves the module it borrows from as it was)


def test_oracle_cell_majority_windows_ties_and_out_of_range():
    assert D.windows(7, 7) == [(i, i + 1) for i in range(7)] and D.windows(5, 2) == [(0, 3), (2, 5)]
    assert D.windows(224, 10)[-1] == (201, 224) and D.windows(8, 2) == [(0, 4), (4, 8)]
    labels = np.zeros((1, 4, 5), dtype=np.uint8)
    labels[0, :, :3] = [[1, 1, 3], [3, 3, 1], [9, 9, 9], [9, 9, 9]]
    label, purity = D.cell_majority(labels, 4, (2, 2))
    # cell (0, 0): rows 0-1, columns 0-2: three 1s, three 3s -> 1;  cell (1, 0): only 9s -> -1
    assert label[0].tolist() == [[1, 0], [-1, 0]]
    # cells (0, 1) and (1, 1) share column 2 with their neighbours (5 -> 2 overlaps): four 0s among six values
    two_thirds = float(np.float32(4) / np.float32(6))
    assert purity[0].tolist() == [[0.5, two_thirds], [0.0, two_thirds]] and purity.dtype == np.float32
    assert D.knn_class([1, 2, 0, -1], [1, 2, 2, 0]) == 0.5
    # class 1: P = {0}, T = {0} -> 1;  class 2: P = {1}, T = {1, 2} -> 2/3;  class 3 does not occur
    assert abs(D.knn_dice([1, 2, 0, -1], [1, 2, 2, 0], 4) - (1.0 + 2.0 / 3.0) / 2) < 1e-15
    assert np.isnan(D.knn_dice([0, 0], [0, 0], 4))


def test_dice_from_confusion_agrees_with_the_oracle():
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.epochers.dense_monitor import dice_from_confusion
    g = np.random.default_rng(3)
    C = 4
    labels, pred = g.integers(0, C, 200), g.integers(-1, C, 200)
    labels[labels == 3] = 2  # (a foreground class that does not occur)
    conf = [[int(((labels == t) & (pred == (p if p < C else -1))).sum()) for p in range(C + 1)] for t in range(C)]
    assert abs(dice_from_confusion(conf) - D.knn_dice(pred, labels, C)) < 1e-15
    assert np.isnan(dice_from_confusion([[5, 0, 0], [0, 0, 0]]))


# ---- the DenseMonitor section
def test_dense_monitor_section_defaults_and_round_trip():
    import yaml
    import spcl_amd  # noqa: F401
    from spcl_amd import config
    from spcl_amd.semi_seg.epochers.dense_monitor import DENSE_MONITOR_DEFAULTS, parse_dense_monitor
    from spcl_amd.semi_seg.epochers.monitor import MONITOR_DEFAULTS
    assert config.parse_dense_monitor({}) is None and config.parse_dense_monitor(None) is None
    assert config.parse_dense_monitor({"DenseMonitor": None}) is None and parse_dense_monitor(False) is None
    assert config.parse_dense_monitor({"DenseMonitor": {}}) == parse_dense_monitor(True) == DENSE_MONITOR_DEFAULTS
    assert DENSE_MONITOR_DEFAULTS == {"every": 1, "k": 20, "max_slices": 512, "space": None, "exclude": "scan",
                                      "select_by": None}
    assert MONITOR_DEFAULTS == {"every": 1, "k": 20, "max_slices": 512, "space": None, "select_by": None}  # untouched
    text = ("DenseMonitor:\n  every: 2\n  k: 10\n  max_slices: 40\n  space: dense_projection\n  exclude: slice\n"
            "  select_by: up_conv3/dense_projection/knn_class\n")
    parsed = config.parse_dense_monitor(yaml.safe_load(text))
    assert parsed == {"every": 2, "k": 10, "max_slices": 40, "space": "dense_projection", "exclude": "slice",
                      "select_by": "up_conv3/dense_projection/knn_class"}
    assert config.parse_dense_monitor(yaml.safe_load(yaml.safe_dump({"DenseMonitor": parsed}))) == parsed
    assert parse_dense_monitor(parsed) == parsed
    off = config.parse_dense_monitor(yaml.safe_load("DenseMonitor:\n  select_by: false\n"))
    assert off["select_by"] is False and parse_dense_monitor(off) == off
    assert config.parse_monitor({"DenseMonitor": {}}) is None  # (the two sections do not see each other)


@pytest.mark.parametrize("section", [
    {"evry": 1}, {"every": 0}, {"every": 1.5}, {"k": 0}, {"k": 33}, {"k": True}, {"max_slices": 0}, {"max_slices": 8193},
    {"space": "projection"}, {"space": "feature"}, {"exclude": "patient"}, {"exclude": None}, "yes", [1],
    {"select_by": "knn_dice"}, {"select_by": "up_conv3/projection/knn_dice"}, {"select_by": "up_conv3/dense_projection/top1"},
    {"select_by": True}, {"select_by": 3}, {"select_by": "up_conv3/dense_projection/knn_dice/extra"},
    {"space": "dense_feature", "select_by": "up_conv3/dense_projection/knn_dice"},
])
def test_dense_monitor_section_refuses_bad_values(section):
    from spcl_amd.semi_seg.epochers.dense_monitor import parse_dense_monitor
    with pytest.raises(ValueError, match="DenseMonitor"):
        parse_dense_monitor(section)


# ---- which keys a trainer can select by, decided from the hooks alone (no device)
def _hooks(feature_names, net=None):
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.hooks import create_infonce_hooks
    net = net or UNet(input_dim=1, num_classes=4, max_channel=128)
    return net, [create_infonce_hooks(model=net, feature_names=feature_names, weights=1.0,
                                      contrast_ons=["partition", "patient", "partition"][:len(feature_names)], data_name="acdc")]


def test_expected_keys_and_the_default_select_by():
    from spcl_amd.semi_seg.epochers import dense_monitor as dm
    from spcl_amd.semi_seg.epochers.monitor import monitor_targets
    net, hooks = _hooks(["Conv5", "Up_conv3"])
    # exactly the hooks the monitor reports as skipped
    assert [p[0] for p in dm.dense_targets(hooks)] == ["up_conv3"] and monitor_targets(hooks)[1] == ["infonce_up_conv3_patient"]
    keys = dm.expected_keys(net, hooks)
    assert keys == [f"up_conv3/{s}/{m}" for s in ("dense_feature", "dense_projection") for m in METRICS]
    assert dm.expected_keys(net, hooks, "dense_feature") == [f"up_conv3/dense_feature/{m}" for m in METRICS]
    assert dm.resolve_select_by(keys, None) == "up_conv3/dense_projection/knn_dice"
    assert dm.resolve_select_by(dm.expected_keys(net, hooks, "dense_feature"), None) == "up_conv3/dense_feature/knn_dice"
    assert dm.resolve_select_by(keys, "up_conv3/dense_feature/uniform") == "up_conv3/dense_feature/uniform"
    assert dm.resolve_select_by(keys, False) is None
    with pytest.raises(ValueError, match="select_by"):
        dm.resolve_select_by(keys, "up_conv2/dense_projection/knn_dice")
    # two hooks on one feature: the projections go under the hooks' names, the feature once under its own
    net, hooks = _hooks(["Up_conv3", "Up_conv3"])
    heads = sorted({k.rsplit("/", 1)[0] for k in dm.expected_keys(net, hooks)})
    assert heads == ["infonce_up_conv3_partition/dense_projection", "infonce_up_conv3_patient/dense_projection",
                     "up_conv3/dense_feature"]
    # encoder hooks only: nothing
    net, hooks = _hooks(["Conv5"])
    assert dm.dense_targets(hooks) == [] and dm.expected_keys(net, hooks) == [] and dm.resolve_select_by([], None) is None
    with pytest.raises(ValueError, match="no contrastive hook on a decoder feature"):
        dm.resolve_select_by([], "up_conv3/dense_projection/knn_dice")


def test_slice_set_is_sized_by_the_grid():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    from spcl_amd.semi_seg.epochers import dense_monitor as dm
    _, hooks = _hooks(["Up_conv3"])  # the dense hooks pool to 10 x 10
    assert dm._grid(dm.dense_targets(hooks)[0][2]) == (10, 10)
    assert dm.dense_slices(hooks, 512) == F_hip.EMBED_MONITOR_MAX_N // 100 == 81 and dm.dense_slices(hooks, 16) == 16


class _Store:
    """what ``monitor_store`` asks of a store (host only)"""
    images, data_name = torch.zeros(4, 8, 8), "acdc"

    def __init__(self, targets):
        self.targets = targets

    def meta(self, i):
        return f"patient001_00_{i:02d}", "0", "patient001_00"

    def __len__(self):
        return 4


def _trainer(feature_names, store, **kwargs):
    from spcl_amd.semi_seg.trainers import PretrainDecoderTrainer
    net, hooks = _hooks(feature_names)
    tr = PretrainDecoderTrainer(model=net, chain_dataloader=store, max_epoch=2, num_batches=1, device="cpu", **kwargs)
    tr.register_hooks(*hooks)
    return tr


def test_trainers_take_the_keyword_and_refuse_in_init_before_any_device_work():
    import inspect
    from spcl_amd.semi_seg.trainers import PretrainDecoderTrainer, PretrainEncoderTrainer
    assert inspect.signature(PretrainEncoderTrainer.__init__).parameters["dense_monitor"].default is None
    assert issubclass(PretrainDecoderTrainer, PretrainEncoderTrainer)
    with pytest.raises(ValueError, match="DenseMonitor"):
        PretrainEncoderTrainer(model=torch.nn.Identity(), chain_dataloader=iter([]), dense_monitor={"exclude": "nobody"})
    labelled, bare = _Store(torch.zeros(4, 8, 8, dtype=torch.uint8)), _Store(None)
    # no contrastive hook on a decoder feature
    with pytest.raises(ValueError, match="no contrastive hook taps a decoder feature"):
        _trainer(["Conv5"], labelled, dense_monitor=True).init()
    # a store without label maps
    with pytest.raises(ValueError, match="no label maps"):
        _trainer(["Up_conv3"], bare, dense_monitor=True).init()
    # a select_by the registered hooks cannot produce
    with pytest.raises(ValueError, match="select_by"):
        _trainer(["Up_conv3"], labelled, dense_monitor={"select_by": "up_conv2/dense_projection/knn_dice"}).init()
    # two selectors: the message names both keys
    with pytest.raises(ValueError) as err:
        _trainer(["Conv5", "Up_conv3"], labelled, monitor=True, dense_monitor=True).init()
    assert "conv5/projection/knn_patient" in str(err.value) and "up_conv3/dense_projection/knn_dice" in str(err.value)


def test_one_selector_is_resolved_when_the_other_cannot_or_must_not_select():
    tr = _trainer(["Conv5", "Up_conv3"], _Store(torch.zeros(4, 8, 8, dtype=torch.uint8)), monitor=True,
                  dense_monitor={"select_by": False})
    tr._resolve_monitor_key()
    tr._resolve_dense_key()
    assert tr._monitor_key == "conv5/projection/knn_patient" and tr._dense_key is None
    tr = _trainer(["Up_conv3"], _Store(torch.zeros(4, 8, 8, dtype=torch.uint8)), monitor=True, dense_monitor=True)
    with pytest.warns(UserWarning, match="nothing to score"):
        tr._resolve_monitor_key()
    tr._resolve_dense_key()
    assert tr._monitor_key is None and tr._dense_key == "up_conv3/dense_projection/knn_dice"


# ---- the functional's refusals that need no device
def test_functional_refuses_a_bad_group_and_bad_label_maps_on_the_host():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    z = torch.zeros(4, 3)
    for group in (torch.zeros(3, dtype=torch.long), torch.zeros(4), torch.zeros(4, dtype=torch.bool), [0, 0, 1, 1],
                  torch.zeros(4, 1, dtype=torch.long)):
        with pytest.raises(ValueError, match="group"):
            F_hip.embedding_monitor(z, k=2, group=group)
    with pytest.raises(TypeError):
        F_hip.embedding_monitor(z, None, None, 2, True, False, torch.zeros(4, dtype=torch.long))  # keyword only
    with pytest.raises(RuntimeError, match="MI355X"):  # no CPU fallback
        F_hip.embedding_monitor(z, k=2, group=torch.zeros(4, dtype=torch.long))
    maps = torch.zeros(2, 8, 8, dtype=torch.uint8)
    for args in ((maps.long(), 4, (2, 2)), (maps, 1, (2, 2)), (maps, 17, (2, 2)), (maps, 4, (9, 2)), (maps, 4, (2, 0)),
                 (maps[0, 0], 4, (2, 2)), (maps, 4.0, (2, 2))):
        with pytest.raises(ValueError, match="cell_majority"):
            F_hip.cell_majority(*args)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.cell_majority(maps, 4, (2, 2))


# ---- the C ABI
def test_header_declares_the_two_entries_and_abi_30():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    hdr = open(HEADER).read()
    assert int(re.search(r"#define\s+SPCL_ABI_VERSION\s+(\d+)", hdr).group(1)) == native.ABI_VERSION >= 30
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int spcl_embed_monitor_grouped(const float* z, int64_t ldz, const int32_t* labels, int L, const int32_t* pair, "
            "const int32_t* group, int N, int d, int k, int exclude_pair, int32_t* knn_idx, float* knn_sim, int32_t* pred, "
            "int32_t* correct, int32_t* pair_rank, double* scalars, void* ws, size_t ws_bytes, void* stream);") in flat
    assert ("int spcl_cell_majority(const uint8_t* labels, int N, int H, int W, int C, int sh, int sw, int32_t* cell_label, "
            "float* purity, void* stream);") in flat
    assert len(native._SIGNATURES["spcl_embed_monitor_grouped"][1]) == 19
    assert len(native._SIGNATURES["spcl_cell_majority"][1]) == 10
    lib = native.lib()
    assert hasattr(lib, "spcl_embed_monitor_grouped") and hasattr(lib, "spcl_cell_majority")
