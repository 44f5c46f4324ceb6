"""CPU: the restatements tests/_pixel_contrast_oracle.py are what the GPU tests compare against, so they are checked here --
the key is injective, the selection it induces is uniform, the float64 criterion equals the definition term by term -- together
with the host-side refusals of the functional wrappers, the config wiring and the C ABI's declarations."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import _pixel_contrast_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("spcl_pixel_sample_workspace_bytes", "spcl_pixel_sample", "spcl_rows_gather_forward", "spcl_rows_gather_backward",
           "spcl_pixel_supcon_workspace_bytes", "spcl_pixel_supcon_forward", "spcl_pixel_supcon_backward")


def _F():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional
    return functional


@pytest.mark.parametrize("seed", [0, 1, 2 ** 32 - 1])
def test_keys_of_distinct_cells_are_distinct(seed):
    k = O.keys(2 ** 20, seed)
    assert int(k.max()) < 2 ** 32 and np.unique(k).size == 2 ** 20


def test_key_of_known_words():
    """fmix32 against values worked out by hand from the definition (Python integers)"""
    def fmix(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)
    for seed in (0, 7, 0x80000000, 0xFFFFFFFF):
        want = [fmix((((i + 1) * 0x9E3779B1) & 0xFFFFFFFF) ^ seed) for i in range(50)]
        assert O.keys(50, seed).tolist() == want


def test_selection_is_uniform_over_seeds():
    """2 x 16 x 16 cells: 379 of class 0, 128 of class 1, 5 ineligible; K = 40; seeds 0 .. 3999.  Every cell's selection
    frequency lies within 5 binomial standard deviations of K / n_c"""
    lab = np.concatenate([np.zeros(379), np.ones(128), -np.ones(5)]).astype(np.int32).reshape(2, 16, 16)
    n_seeds, K = 4000, 40
    hits = np.zeros(512, dtype=np.int64)
    for seed in range(n_seeds):
        idx, count = O.sample(lab, 2, K, seed)
        assert count.tolist() == [K, K]
        hits[idx.reshape(-1)] += 1
    assert hits[507:].sum() == 0
    for c, cells in ((0, slice(0, 379)), (1, slice(379, 507))):
        n_c = cells.stop - cells.start
        p = K / n_c
        sd = math.sqrt(n_seeds * p * (1 - p))
        worst = float(np.abs(hits[cells] - n_seeds * p).max() / sd)
        print(f"class {c}: n_c = {n_c}, worst deviation {worst:.2f} standard deviations")
        assert worst < 5.0


def test_oracle_sample_orders_by_index_and_pads():
    lab = np.array([0, 1, 0, 0, -1, 1, 0, 7], dtype=np.int32)
    idx, count = O.sample(lab, 2, 3, 5)
    assert count.tolist() == [3, 2] and idx[1].tolist() == [1, 5, -1]
    k = O.keys(8, 5)
    zeros = sorted(sorted([0, 2, 3, 6], key=lambda i: int(k[i]))[:3])
    assert idx[0].tolist() == zeros


@pytest.mark.parametrize("count", [[4, 2, 0], [4, 1, 3], [4, 4, 4], [1, 1, 1]])
def test_float64_restatement_equals_the_brute_force_definition(count):
    C, K, d = 3, 4, 8
    g = torch.Generator().manual_seed(2)
    z = torch.nn.functional.normalize(torch.randn(C * K, d, generator=g).double(), dim=1)
    for t in (0.07, 1.0):
        got = float(O.supcon(z, count, K, t))
        want = O.supcon_bruteforce(z.numpy(), count, K, t)
        assert got == pytest.approx(want, rel=1e-12, abs=1e-12)
    valid, _ = O.slots(count, K)
    poisoned = z.clone()
    poisoned[~valid] = float("nan")
    assert float(O.supcon(poisoned, count, K, 0.1)) == float(O.supcon(z, count, K, 0.1))
    assert O.anchors(count) == sum(c for c in count if c >= 2)


def test_sampler_refusals():
    F = _F()
    lab = torch.zeros(2, 4, 4, dtype=torch.int32)
    for C, K in ((1, 4), (17, 4), (4, 0), (4, 1025), (16, 257), (True, 4), (4, 2.0)):
        with pytest.raises(ValueError):
            F.pixel_sample(lab, C, K, 0)
    with pytest.raises(ValueError):
        F.pixel_sample(lab.long(), 4, 4, 0)
    with pytest.raises(ValueError):
        F.pixel_sample(lab[0], 4, 4, 0)
    for seed in (-1, 2 ** 32, 1.5, True, torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(ValueError):
            F.pixel_sample(lab, 4, 4, seed)
    with pytest.raises(RuntimeError, match="MI355X"):
        F.pixel_sample(lab, 4, 4, 0)


def test_gather_refusals():
    F = _F()
    feat, idx = torch.zeros(2, 8, 4, 4), torch.zeros(6, dtype=torch.int32)
    with pytest.raises(ValueError):
        F.gather_rows(feat.double(), idx)
    with pytest.raises(ValueError):
        F.gather_rows(feat[0], idx)
    with pytest.raises(ValueError):
        F.gather_rows(feat, idx.long())
    with pytest.raises(ValueError):
        F.gather_rows(feat, idx[:0])
    with pytest.raises(RuntimeError, match="MI355X"):
        F.gather_rows(feat, idx)


def test_criterion_refusals():
    F = _F()
    count = torch.tensor([2, 2], dtype=torch.int32)
    z = torch.zeros(8, 8)
    with pytest.raises(ValueError):
        F.pixel_supcon(z.double(), count, 4)
    with pytest.raises(ValueError):
        F.pixel_supcon(z, count.long(), 4)
    with pytest.raises(ValueError):
        F.pixel_supcon(z, count, 3)  # 8 rows are not 2 x 3
    with pytest.raises(ValueError):
        F.pixel_supcon(z, count[:1], 8)  # C = 1
    with pytest.raises(ValueError):
        F.pixel_supcon(torch.zeros(17 * 4, 8), torch.zeros(17, dtype=torch.int32), 4)
    with pytest.raises(ValueError):
        F.pixel_supcon(torch.zeros(16 * 257, 8), torch.zeros(16, dtype=torch.int32), 257)  # C K > 4096
    for d in (2, 6, 260):
        with pytest.raises(ValueError):
            F.pixel_supcon(torch.zeros(8, d), count, 4)
    for t in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            F.pixel_supcon(z, count, 4, t)
    with pytest.raises(RuntimeError, match="MI355X"):
        F.pixel_supcon(z, count, 4)


def _config(**sections):
    return dict({"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 2}}, **sections)


def test_config_section_builds_the_hook_and_its_absence_none():
    import spcl_amd  # noqa: F401
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.hooks import PixelContrastTrainerHook
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    assert create_hook_from_config(model, _config()) == []
    (hook,) = create_hook_from_config(model, _config(PixelContrastParameters={"weight": 0.5, "samples_per_class": 16, "seed": 9}))
    assert isinstance(hook, PixelContrastTrainerHook)
    assert hook.draw.dtype == torch.int32 and hook.draw.tolist() == [9] and "draw" in hook.state_dict()
    cin = model.get_channel_dim("Up_conv3")
    assert sum(p.numel() for p in hook.parameters()) == (cin * 128 + 128) + (128 * 64 + 64)
    key = hook().graph_key()
    assert key is not None and hash(key) is not None and 16 in key and "Up_conv3" in key
    (linear,) = create_hook_from_config(model, _config(PixelContrastParameters={
        "weight": 1.0, "feature_name": "Up_conv2", "head_type": "linear", "output_dim": 32, "unlabeled_threshold": 0.9}))
    assert sum(p.numel() for p in linear.parameters()) == model.get_channel_dim("Up_conv2") * 32 + 32
    with pytest.raises(RuntimeError, match="pretrain"):
        create_hook_from_config(model, _config(PixelContrastParameters={"weight": 0.5}), is_pretrain=True)
    for bad in ({"samples_per_class": 2048}, {"temperature": 0.0}, {"unlabeled_threshold": 1.5}, {"seed": -1},
                {"feature_name": "nowhere"}, {"output_dim": 6}, {"head_type": "conv"}):
        with pytest.raises(ValueError):
            create_hook_from_config(model, _config(PixelContrastParameters=dict({"weight": 0.5}, **bad)))


def test_hook_call_without_label_maps_names_the_missing_keyword():
    import types

    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.meters import MeterInterface
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.hooks import PixelContrastTrainerHook
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    hook = PixelContrastTrainerHook(name="pixelcontrast", model=model, weight=1.0)
    eh = hook()
    meters = MeterInterface(default_focus="semi")
    eh.meters = meters
    eh.configure_meters(meters)
    eh._epocher = types.SimpleNamespace(_model=model)
    with pytest.raises(ValueError, match="labeled_target"):
        eh(unlabeled_logits=None, seed=1)
    eh.close()


def test_abi_header_declares_the_new_entries():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    hdr = open(os.path.join(REPO, "include", "spcl_hip.h")).read()
    assert int(re.search(r"#define\s+SPCL_ABI_VERSION\s+(\d+)", hdr).group(1)) == native.ABI_VERSION >= 34
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in native._SIGNATURES and hasattr(native.lib(), name)
    lib = native.lib()
    assert lib.spcl_pixel_supcon_workspace_bytes(4097, 64) == 0 and lib.spcl_pixel_supcon_workspace_bytes(64, 6) == 0
    assert lib.spcl_pixel_supcon_workspace_bytes(68, 8) == (1 + 3 * 2 + 2 * 8) * 128 * 4  # 2 row blocks: 2 column splits
    assert lib.spcl_pixel_supcon_workspace_bytes(64, 8) == (1 + 3 + 8) * 64 * 4
    assert lib.spcl_pixel_supcon_workspace_bytes(4096, 256) == (1 + 3 * 4 + 4 * 256) * 4096 * 4
    assert lib.spcl_pixel_sample_workspace_bytes(0) == 0
    assert lib.spcl_pixel_sample_workspace_bytes(2 ** 31 - 1) > lib.spcl_pixel_sample_workspace_bytes(64) > 4 * 16 * 256 * 4
