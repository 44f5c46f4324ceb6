"""CPU-only side of the pre-training monitor: the float64 oracle of tests/_embed_monitor_oracle.py on a hand-worked case, the
host-side refusals of ``functional.embedding_monitor``, the ``Monitor`` config section, and the C ABI's entry."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import _embed_monitor_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "spcl_hip.h")


# ---- the oracle
ANGLES = [0.0, 10.0, 25.0, 180.0, 200.0, 90.0]


def _six_rows():
    a = np.deg2rad(np.array(ANGLES))
    scale = np.array([1.0, 2.0, 3.0, 0.5, 4.0, 1.0])[:, None]
    z = np.stack([np.cos(a), np.sin(a)], 1) * scale
    return z, np.array([[0, 0, 1, 1, 1, 0]]), np.array([3, -1, -1, 0, -1, -1])


def test_oracle_on_six_hand_worked_rows():
    z, labels, pair = _six_rows()
    r = O.embed_monitor(z, labels, pair, k=2, exclude_pair=True)
    # worked by hand from the cosines of the angle differences
    assert r["knn_idx"].tolist() == [[1, 2], [0, 2], [1, 0], [4, 5], [3, 5], [2, 1]]
    cos = lambda i, j: math.cos(math.radians(ANGLES[i] - ANGLES[j]))  # noqa: E731
    for i, row in enumerate(r["knn_idx"]):
        for t, j in enumerate(row):
            assert abs(r["knn_sim"][i, t] - cos(i, j)) < 1e-12
    # votes: rows 0 and 1 see labels (0, 1) -- a tie, the best-ranked wins --, row 2 (0, 0), rows 3 and 4 (1, 0), row 5 (1, 0)
    assert r["pred"].tolist() == [[0, 0, 0, 1, 1, 1]] and r["correct"].tolist() == [4]
    # rows 0 and 3 are each other's opposite (s = -1): the four other rows all beat the pair
    assert r["pair_rank"].tolist() == [4, -1, -1, 4, -1, -1]
    assert abs(r["alignment"] - 4.0) < 1e-12 and r["n_pairs"] == 2 and r["min_norm"] == 0.5
    mean = sum(math.exp(-4.0 * (1.0 - cos(i, j))) for i in range(6) for j in range(6) if i != j) / 30.0
    assert abs(r["uniform_mean"] - mean) < 1e-12 and abs(r["uniformity"] - math.log(mean)) < 1e-12


def test_oracle_tie_rules_and_short_rows():
    e1, e2 = [1.0, 0.0], [0.0, 1.0]
    r = O.embed_monitor(np.array([e1, e2, e1, e1]), np.array([5, 6, 7, 7]), np.array([2, -1, 0, -1]), k=3, exclude_pair=False)
    assert r["knn_idx"].tolist() == [[2, 3, 1], [0, 2, 3], [0, 3, 1], [0, 2, 1]]  # equal similarities: the lower index first
    assert r["pair_rank"].tolist() == [0, -1, 0, -1]  # row 0: 3 ties the pair 2 but has the higher index
    r = O.embed_monitor(np.array([e1, e2, e1, e1]), np.array([5, 6, 7, 7]), np.array([2, -1, 0, -1]), k=3, exclude_pair=True)
    assert r["knn_idx"].tolist() == [[3, 1, -1], [0, 2, 3], [3, 1, -1], [0, 2, 1]]
    assert np.isneginf(r["knn_sim"][0, 2]) and r["pred"].tolist() == [[7, 7, 7, 5]]
    assert O.vote([]) == -1 and O.vote([7, 9, 9, 7, 3]) == 7 and O.vote([9, 7, 7, 9, 3]) == 9 and O.vote([3, 9, 9]) == 9
    r = O.embed_monitor(np.array([e1, e2]), np.array([1, 1]), np.array([1, 0]), k=2, exclude_pair=True)
    assert r["knn_idx"].tolist() == [[-1, -1], [-1, -1]] and r["pred"].tolist() == [[-1, -1]] and r["correct"].tolist() == [0]


def test_oracle_check_accepts_itself_and_rejects_a_wrong_neighbour():
    z, labels, pair = _six_rows()
    r = O.embed_monitor(z, labels, pair, k=2)
    got = dict(knn_idx=r["knn_idx"], knn_sim=r["knn_sim"], pred=r["pred"], correct=r["correct"], pair_rank=r["pair_rank"],
               scalars=np.array([r["alignment"], r["uniformity"], r["n_pairs"], r["min_norm"]]))
    O.check(got, z, labels, pair, 2, True)
    bad = dict(got, knn_idx=got["knn_idx"].copy())
    bad["knn_idx"][0, 1] = 4  # the row's opposite instead of its second neighbour
    with pytest.raises(AssertionError):
        O.check(bad, z, labels, pair, 2, True)
    assert O.tol(128) == 136 * 2.0 ** -24


# ---- the functional's refusals: ValueError on the host, before any device work (these tensors live on the CPU)
def _F():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    return F_hip


@pytest.mark.parametrize("kwargs", [
    dict(z=torch.zeros(4, 3, dtype=torch.float64)),
    dict(z=torch.zeros(4, 3, dtype=torch.bfloat16)),
    dict(z=torch.zeros(4)),
    dict(z=torch.zeros(2, 4, 3)),
    dict(z=torch.zeros(1, 3)),
    dict(z=torch.zeros(8193, 2)),
    dict(z=torch.zeros(4, 513)),
    dict(z=torch.zeros(4, 3), k=0),
    dict(z=torch.zeros(4, 3), k=33),
    dict(z=torch.zeros(4, 3), k=2.0),
    dict(z=torch.zeros(4, 3), labels=torch.zeros(5, dtype=torch.long)),
    dict(z=torch.zeros(4, 3), labels=torch.zeros(5, 4, dtype=torch.long)),
    dict(z=torch.zeros(4, 3), labels=torch.zeros(4)),
    dict(z=torch.zeros(4, 3), labels=torch.zeros(1, 1, 4, dtype=torch.long)),
    dict(z=torch.zeros(4, 3), labels=torch.tensor([0, 1, 2, 65536]), check_labels=True),
    dict(z=torch.zeros(4, 3), labels=torch.tensor([0, -1, 2, 3]), check_labels=True),
    dict(z=torch.zeros(4, 3), pair=torch.zeros(3, dtype=torch.long)),
    dict(z=torch.zeros(4, 3), pair=torch.zeros(4)),
    dict(z=torch.zeros(4, 3), pair=[1, 0, 3, 2]),
])
def test_functional_refuses_on_the_host(kwargs):
    kwargs = dict(kwargs)
    z = kwargs.pop("z")
    with pytest.raises(ValueError, match="embedding_monitor"):
        _F().embedding_monitor(z, **kwargs)


def test_functional_has_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="MI355X"):
        _F().embedding_monitor(torch.zeros(4, 3), torch.zeros(4, dtype=torch.long), torch.tensor([1, 0, 3, 2]), k=2)


def test_result_is_a_named_tuple_of_the_six_outputs():
    assert _F().EmbeddingMonitorResult._fields == ("knn_idx", "knn_sim", "pred", "correct", "pair_rank", "scalars")


# ---- the Monitor section
def test_monitor_section_round_trip():
    import yaml
    import spcl_amd  # noqa: F401
    from spcl_amd import config
    from spcl_amd.semi_seg.epochers.monitor import MONITOR_DEFAULTS, parse_monitor
    assert config.parse_monitor({}) is None and config.parse_monitor(None) is None
    assert config.parse_monitor({"Monitor": None}) is None and parse_monitor(False) is None
    assert config.parse_monitor({"Monitor": {}}) == parse_monitor(True) == MONITOR_DEFAULTS
    assert MONITOR_DEFAULTS == {"every": 1, "k": 20, "max_slices": 512, "space": None, "select_by": None}
    text = "Monitor:\n  every: 2\n  k: 10\n  max_slices: 256\n  space: projection\n  select_by: conv5/projection/knn_partition\n"
    parsed = config.parse_monitor(yaml.safe_load(text))
    assert parsed == {"every": 2, "k": 10, "max_slices": 256, "space": "projection",
                      "select_by": "conv5/projection/knn_partition"}
    assert config.parse_monitor(yaml.safe_load(yaml.safe_dump({"Monitor": parsed}))) == parsed
    assert parse_monitor(parsed) == parsed


@pytest.mark.parametrize("section", [
    {"evry": 1}, {"every": 0}, {"every": 1.5}, {"k": 0}, {"k": 33}, {"k": True}, {"max_slices": 0}, {"max_slices": 4097},
    {"space": "logits"}, "yes", [1],
])
def test_monitor_section_refuses_bad_values(section):
    from spcl_amd.semi_seg.epochers.monitor import parse_monitor
    with pytest.raises(ValueError, match="Monitor"):
        parse_monitor(section)


@pytest.mark.parametrize("select_by", ["knn_patient", "conv5/logits/knn_patient", "conv5/projection/accuracy",
                                       "conv5/projection/knn_", "conv5/projection", 3, "conv5/projection/top1/extra"])
def test_unknown_select_by_keys_are_refused(select_by):
    from spcl_amd.semi_seg.epochers.monitor import parse_monitor
    with pytest.raises(ValueError, match="select_by"):
        parse_monitor({"select_by": select_by})


def test_select_by_must_lie_in_the_monitored_space_and_in_the_result():
    from spcl_amd.semi_seg.epochers.monitor import monitor_indices, parse_monitor, select_score
    with pytest.raises(ValueError, match="select_by"):
        parse_monitor({"space": "feature", "select_by": "conv5/projection/knn_patient"})
    result = {"conv5/feature/knn_patient": 0.5, "conv5/projection/knn_patient": 0.75, "conv5/projection/uniform": -2.0,
              "skipped": []}
    assert select_score(result, None) == ("conv5/projection/knn_patient", 0.75)
    assert select_score(result, "conv5/projection/uniform") == ("conv5/projection/uniform", 2.0)  # lower is better
    assert select_score({"conv5/feature/knn_patient": 0.5, "skipped": []}, None) == ("conv5/feature/knn_patient", 0.5)
    for key in ("conv4/projection/knn_patient", "skipped"):
        with pytest.raises(ValueError, match="select_by"):
            select_score(result, key)
    assert monitor_indices(10, 4) == [0, 2, 5, 7] and monitor_indices(3, 512) == [0, 1, 2]


def test_trainers_take_the_monitor_keyword():
    import inspect
    from spcl_amd.semi_seg.trainers import PretrainDecoderTrainer, PretrainEncoderTrainer
    assert inspect.signature(PretrainEncoderTrainer.__init__).parameters["monitor"].default is None
    assert issubclass(PretrainDecoderTrainer, PretrainEncoderTrainer)
    with pytest.raises(ValueError, match="select_by"):
        PretrainEncoderTrainer(model=torch.nn.Identity(), chain_dataloader=iter([]), monitor={"select_by": "nonsense"})


# ---- the C ABI
def test_header_declares_the_entry_and_abi_29():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    hdr = open(HEADER).read()
    assert int(re.search(r"#define\s+SPCL_ABI_VERSION\s+(\d+)", hdr).group(1)) == native.ABI_VERSION >= 29
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "size_t spcl_embed_monitor_workspace_bytes(int N, int d, int k);" in flat
    assert ("int spcl_embed_monitor(const float* z, int64_t ldz, const int32_t* labels, int L, const int32_t* pair, int N, "
            "int d, int k, int exclude_pair, int32_t* knn_idx, float* knn_sim, int32_t* pred, int32_t* correct, "
            "int32_t* pair_rank, double* scalars, void* ws, size_t ws_bytes, void* stream);") in flat
    assert len(native._SIGNATURES["spcl_embed_monitor"][1]) == 18
    assert len(native._SIGNATURES["spcl_embed_monitor_workspace_bytes"][1]) == 3


def test_workspace_entry_refuses_outside_the_limits():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    ws = lambda N, d, k: native.call("spcl_embed_monitor_workspace_bytes", N, d, k)  # noqa: E731
    assert ws(2, 1, 1) > 0 and ws(8192, 512, 32) > 8192 * 512 * 4
    for N, d, k in ((1, 4, 1), (8193, 4, 1), (4, 0, 1), (4, 513, 1), (4, 4, 0), (4, 4, 33)):
        assert ws(N, d, k) == 0
    assert native.call("spcl_embed_monitor_workspace_bytes", 130, 20, 5) % 4 == 0


# ---- which keys a trainer can select by, decided from the hooks alone (no device)
def _hooks(feature_names, net=None):
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.hooks import create_infonce_hooks
    net = net or UNet(input_dim=1, num_classes=4, max_channel=128)
    return net, [create_infonce_hooks(model=net, feature_names=feature_names, weights=1.0,
                                      contrast_ons=["partition", "patient", "partition"][:len(feature_names)], data_name="acdc")]


def test_expected_keys_follow_the_hooks():
    from spcl_amd.semi_seg.epochers.monitor import expected_keys, monitor_targets, resolve_select_by
    from spcl_amd.semi_seg.hooks.utils import contrast_kinds
    assert contrast_kinds("acdc") == ["partition", "patient", "self", "cycle"]
    assert contrast_kinds("prostate") == ["partition", "patient", "self"]
    with pytest.raises(NotImplementedError):
        contrast_kinds("nowhere")
    metrics = ["knn_partition", "knn_patient", "knn_cycle", "top1", "recall5", "align", "uniform", "min_norm"]
    net, hooks = _hooks(["Conv5", "Up_conv3"])
    assert monitor_targets(hooks)[1] == ["infonce_up_conv3_patient"]
    keys = expected_keys(net, hooks, "acdc")
    assert keys == [f"conv5/{s}/{m}" for s in ("feature", "projection") for m in metrics]
    assert expected_keys(net, hooks, "prostate", "feature") == [f"conv5/feature/{m}" for m in metrics if m != "knn_cycle"]
    assert resolve_select_by(keys, None) == "conv5/projection/knn_patient"
    assert resolve_select_by(expected_keys(net, hooks, "acdc", "feature"), None) == "conv5/feature/knn_patient"
    assert resolve_select_by(keys, "conv5/feature/uniform") == "conv5/feature/uniform"
    with pytest.raises(ValueError, match="select_by"):
        resolve_select_by(keys, "conv4/projection/knn_patient")
    # two hooks on one feature: the projections go under the hooks' names, the feature once under its own
    net, hooks = _hooks(["Conv5", "Conv5"])
    heads = sorted({k.rsplit("/", 1)[0] for k in expected_keys(net, hooks, "acdc")})
    assert heads == ["conv5/feature", "infonce_conv5_partition/projection", "infonce_conv5_patient/projection"]


def test_dense_hooks_alone_leave_nothing_to_select_by():
    from spcl_amd.semi_seg.epochers.monitor import expected_keys, resolve_select_by
    net, hooks = _hooks(["Up_conv3"])
    assert expected_keys(net, hooks, "acdc") == [] and resolve_select_by([], None) is None
    with pytest.raises(ValueError, match="no contrastive hook on an encoder feature"):
        resolve_select_by([], "conv5/projection/knn_patient")
