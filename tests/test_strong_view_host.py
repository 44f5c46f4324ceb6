"""CPU: the strong intensity view's oracle (tests/_strong_view_oracle.py), ``functional.StrongViewConfig``, the hook
(semi_seg/hooks/strongview.py), its config section and the epocher's seam -- everything that needs no device."""
import ctypes
import os
import re
import struct
from contextlib import nullcontext

import numpy as np
import pytest
import torch

from tests import _strong_view_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("gamma", "contrast", "brightness", "blur", "noise")


def _cfg(**ops):
    from spcl_amd.functional import StrongViewConfig
    return StrongViewConfig(**ops)


def _all(p):
    return {name: {"p": p} for name in OPS}


def _image(shape, seed=0):
    return np.random.default_rng(seed).random(shape)


# ------------------------------------------------------------------------------------------------------------- ABI
def test_header_binding_and_library_agree_and_export_the_entry_points():
    from spcl_amd import functional as F_hip
    from spcl_amd import native
    header = open(os.path.join(ROOT, "include", "spcl_hip.h")).read()
    version = int(re.search(r"#define SPCL_ABI_VERSION (\d+)", header).group(1))
    L = native.lib()
    assert version == native.ABI_VERSION == L.spcl_abi_version() and version >= 37
    for name, nargs in (("spcl_strong_view_params", 10), ("spcl_strong_view_apply", 10), ("spcl_strong_view_tile", 2)):
        assert name in header and len(native._SIGNATURES[name][1]) == nargs
        assert getattr(L, name, None) is not None, name
    th, tw = F_hip.strong_view_tile()
    assert (th, tw) == tuple(int(re.search(rf"#define SPCL_SV_TILE_{d} (\d+)", header).group(1)) for d in "HW")
    assert F_hip.STRONG_VIEW_COLS == O.COLS == int(re.search(r"#define SPCL_SV_COLS (\d+)", header).group(1))
    # the flip keeps its signature
    assert len(native._SIGNATURES["spcl_flip_batch"][1]) == 9


def _words(**change):
    """the 15 host words of the defaults with single words replaced: ``gamma_p16=...``, ``blur_lo=...``, ``noise_hi=...``"""
    w = list(_cfg().words())
    for key, v in change.items():
        op, what = key.rsplit("_", 1)
        at = 3 * OPS.index(op) + ("p16", "lo", "hi").index(what)
        w[at] = v if what == "p16" else struct.unpack("<i", struct.pack("<f", v))[0]
    return (ctypes.c_int32 * 15)(*w)


PARAMS_REFUSALS = [
    ({"x": None}, b"null"), ({"seed": None}, b"null"), ({"cfg": None}, b"null"), ({"table": None}, b"null"),
    ({"dtype": 2}, b"dtype"), ({"N": 0}, b"N = 0"), ({"N": (1 << 20) + 1}, b"2^20"), ({"C": 0}, b"bad shape"),
    ({"H": -1}, b"bad shape"), ({"W": 0}, b"bad shape"), ({"C": 2, "H": 32768, "W": 32768}, b"too many"),
    ({"cfg": ("gamma_p16", -1)}, b"gamma p16"), ({"cfg": ("noise_p16", 65537)}, b"noise p16"),
    ({"cfg": ("contrast_lo", 2.0)}, b"contrast range"), ({"cfg": ("blur_hi", float("nan"))}, b"blur range"),
    ({"cfg": ("gamma_lo", 0.0)}, b"gamma lo"), ({"cfg": ("brightness_lo", -0.5)}, b"brightness lo"),
    ({"cfg": ("contrast_lo", -0.1)}, b"contrast lo"), ({"cfg": ("blur_lo", -0.25)}, b"blur lo"),
    ({"cfg": ("blur_hi", 1.5)}, b"blur hi"), ({"cfg": ("noise_lo", -0.01)}, b"noise lo"),
]
APPLY_REFUSALS = [
    ({"x": None}, b"null"), ({"out": None}, b"null"), ({"flags": None}, b"null"), ({"table": None}, b"null"),
    ({"dtype": -1}, b"dtype"), ({"N": 0}, b"bad shape"), ({"C": -2}, b"bad shape"), ({"H": 0}, b"bad shape"),
    ({"W": 0}, b"bad shape"), ({"C": 2, "H": 32768, "W": 32768}, b"too many"), ({"out": "x"}, b"one buffer"),
]


def call_params(L, x, seed, table, change):
    kw = dict(x=x, dtype=0, N=3, C=1, H=20, W=24, seed=seed, cfg=_words(), table=table)
    kw.update(change)
    if isinstance(kw["cfg"], tuple):
        kw["cfg"] = _words(**{kw["cfg"][0]: kw["cfg"][1]})
    return L.spcl_strong_view_params(kw["x"], kw["dtype"], kw["N"], kw["C"], kw["H"], kw["W"], kw["seed"], kw["cfg"],
                                     kw["table"], None)


def call_apply(L, x, out, flags, table, change):
    kw = dict(x=x, out=out, dtype=0, N=3, C=1, H=20, W=24, flags=flags, table=table)
    kw.update(change)
    if kw["out"] == "x":
        kw["out"] = kw["x"]
    return L.spcl_strong_view_apply(kw["x"], kw["out"], kw["dtype"], kw["N"], kw["C"], kw["H"], kw["W"], kw["flags"],
                                    kw["table"], None)


def test_the_entries_report_their_refusals():
    """every refusal happens on the host, before any device call: an error code and a message, not a crash"""
    from spcl_amd import native
    L = native.lib()
    a, b, c, d = (ctypes.c_void_p(4096 * k) for k in range(1, 5))  # never dereferenced
    for change, word in PARAMS_REFUSALS:
        assert call_params(L, a, b, c, change) == -1, change
        assert word in L.spcl_last_error(), (change, L.spcl_last_error())
    for change, word in APPLY_REFUSALS:
        assert call_apply(L, a, b, c, d, change) == -1, change
        assert word in L.spcl_last_error(), (change, L.spcl_last_error())


def test_the_functionals_have_no_cpu_path_and_no_backward():
    from spcl_amd import functional as F_hip
    x = torch.zeros(2, 1, 8, 8)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.strong_view_params(x, 0, _cfg())
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.strong_view_apply(x, torch.zeros(2, dtype=torch.uint8), torch.zeros(2, 16))
    with pytest.raises(ValueError, match="requires a gradient"):
        F_hip.strong_view(x.clone().requires_grad_(True), torch.zeros(2, dtype=torch.uint8), 0, _cfg())
    with pytest.raises(ValueError, match="StrongViewConfig"):
        F_hip.strong_view_params(x, 0, {"gamma": {"p": 1.0}})
    with pytest.raises(ValueError, match="seed"):
        F_hip.strong_view_params(x, 2 ** 32, _cfg())
    for bad in (x[0], x.double(), x[:0], "image"):
        with pytest.raises(ValueError, match=r"\[N, C, H, W\]"):
            F_hip.strong_view_params(bad, 0, _cfg())


# ---------------------------------------------------------------------------------------------------------- oracle
def test_the_key_is_the_samplers_key():
    """fmix32(((i + 1) * 0x9E3779B1 mod 2^32) ^ seed) restated with Python integers"""
    def key(i, seed):
        h = (((i + 1) * 0x9E3779B1) & 0xFFFFFFFF) ^ seed
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)

    for seed in (0, 23, 2 ** 32 - 1):
        idx = [0, 1, 16, 12345, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]
        assert O.key(np.array(idx, dtype=np.uint64), seed).tolist() == [key(i, seed) for i in idx]


def test_all_gates_shut_is_the_identity():
    cfg = _cfg(**_all(0.0))
    x = _image((5, 2, 9, 11)) * 1.5 - 0.25  # values beyond [0, 1] as well: a neutral row does not clamp
    flags = [0, 1, 2, 3, 1]
    t = O.table(x, 7, cfg.p16, cfg.lo, cfg.hi)
    assert np.array_equal(t[:, :5], np.tile(np.array(O.NEUTRAL, dtype=np.float32), (5, 1)))
    assert not t[:, 5].any() and not t[:, 8].any() and not t[:, 9:].any()
    assert np.array_equal(t[:, 7], O.mean64(x).astype(np.float32))
    pre, out = O.apply(x, flags, t)
    assert np.array_equal(out, O.flip(x, flags)) and np.array_equal(pre, out)
    assert np.array_equal(O.flip(x, [0] * 5), x)
    assert np.array_equal(O.flip(x, flags)[3], x[3, :, ::-1, ::-1]) and np.array_equal(O.flip(x, flags)[1], x[1, :, ::-1, :])


def test_all_gates_open_applies_every_op_and_the_values_lie_in_their_ranges():
    cfg = _cfg(**_all(1.0))
    assert cfg.p16 == [65536] * 5
    N = 4096
    values, mask, nseed = O.draws(3, N, cfg.p16, cfg.lo, cfg.hi)
    assert (mask == 31).all()
    for k in range(5):
        lo, hi = np.float32(cfg.lo[k]), np.float32(cfg.hi[k])
        assert values.dtype == np.float32 and (values[:, k] >= lo).all() and (values[:, k] <= hi).all(), OPS[k]
        # the draws fill their range: both ends are approached within 1 % of its width
        assert values[:, k].min() < lo + 0.01 * (hi - lo) and values[:, k].max() > hi - 0.01 * (hi - lo), OPS[k]
    assert len(set(nseed.tolist())) == N  # distinct indices have distinct keys


def test_the_ends_of_the_unit_draw_give_the_ends_of_the_range():
    """u = 0 gives lo exactly; u = 2^24 - 1 gives at most hi (the min bites where the rounded difference carries the sum one
    spacing past hi), in float32 arithmetic"""
    f_top = np.float32((2 ** 24 - 1) * 2.0 ** -24)
    for lo, hi in ((0.7, 1.5), (0.75, 1.25), (0.25, 1.0), (0.0, 0.05), (0.1, 0.30000001), (1.0, 1.0)):
        lo, hi = np.float32(lo), np.float32(hi)
        d = np.float32(hi - lo)
        assert np.float32(lo + np.float32(d * np.float32(0.0))) == lo
        top = np.minimum(hi, np.float32(lo + np.float32(d * f_top)))
        assert lo <= top <= hi and hi - top <= 2 * np.spacing(hi)


def test_a_degenerate_range_and_a_half_open_gate():
    cfg = _cfg(gamma={"p": 0.5, "range": (1.25, 1.25)}, contrast={"p": 0.0}, brightness={"p": 0.0}, blur={"p": 0.0},
               noise={"p": 0.0})
    values, mask, _ = O.draws(11, 8192, cfg.p16, cfg.lo, cfg.hi)
    on = mask == 1
    assert set(mask.tolist()) == {0, 1} and 0.47 < on.mean() < 0.53
    assert (values[on, 0] == np.float32(1.25)).all() and (values[~on, 0] == np.float32(1.0)).all()


def test_the_noise_sum_is_standard_normal_to_one_percent():
    z = O.noise_z(0x1234ABCD, 1, 1024, 1024).astype(np.float64)  # 2^20 draws
    assert z.min() >= -131070 and z.max() <= 131070
    g = z * 2.0 ** -16 * float(O.SQRT3_F32)
    print(f"Irwin-Hall noise over 2^20 draws: mean {g.mean():.5f}, variance {g.var():.5f}, |max| {np.abs(g).max():.3f}")
    assert abs(g.mean()) < 0.01 and abs(g.var() - 1.0) < 0.01
    # light tails by construction: |g| <= 2 sqrt(3)
    assert np.abs(g).max() <= 2.0 * np.sqrt(3.0) + 1e-6
    other = O.noise_z(0x1234ABCE, 1, 8, 8)
    assert not np.array_equal(other, O.noise_z(0x1234ABCD, 1, 8, 8))


def test_the_blur_keeps_constants_commutes_with_the_flip_and_has_unit_variance():
    const = np.full((1, 7, 9), 0.37)
    assert np.allclose(O.binomial(const), const, rtol=0, atol=1e-15)
    a = _image((2, 6, 5), seed=4)  # smaller than the halo in W
    for sl in ((slice(None), slice(None, None, -1), slice(None)), (slice(None), slice(None), slice(None, None, -1))):
        assert np.allclose(O.binomial(a[sl]), O.binomial(a)[sl], rtol=0, atol=1e-15)
    taps = np.array([1, 4, 6, 4, 1]) / 16.0
    assert taps.sum() == 1.0 and float((taps * np.arange(-2, 3) ** 2).sum()) == 1.0  # variance 1 at t = 1
    impulse = np.zeros((1, 9, 9))
    impulse[0, 4, 4] = 1.0
    assert np.allclose(O.binomial(impulse)[0, 2:7, 2:7], np.outer(taps, taps), rtol=0, atol=1e-15)


def test_each_op_alone_does_what_its_formula_says():
    x = _image((1, 1, 6, 7), seed=5)
    m = float(np.float32(x.mean()))

    def run(col, v):
        t = O.neutral_table(1, m)
        t[0, col] = v
        return O.apply(x, [0], t)

    g = float(np.float32(1.3))
    assert np.allclose(run(0, 1.3)[1], x ** g, rtol=0, atol=1e-15)
    c = float(np.float32(1.2))
    pre, out = run(1, 1.2)
    assert np.allclose(pre, (x - m) * c + m, rtol=0, atol=1e-15) and np.array_equal(out, np.clip(pre, 0, 1))
    assert abs(pre.mean() - x.mean()) < 1e-6  # contrast about the mean keeps the mean
    pre, out = run(2, 1.25)
    assert np.allclose(pre, x * 1.25, rtol=0, atol=1e-15) and out.max() == 1.0
    assert np.allclose(run(3, 1.0)[1], O.binomial(x[0])[None], rtol=0, atol=1e-15)
    assert np.allclose(run(3, 0.5)[1], 0.5 * x + 0.5 * O.binomial(x[0])[None], rtol=0, atol=1e-15)
    t = O.neutral_table(1, m)
    t[0, 4] = 0.05
    t[0, 6:7] = np.array([99], dtype=np.uint32).view(np.float32)
    pre, _ = O.apply(x, [0], t)
    want = x + float(np.float32(0.05)) * float(O.SQRT3_F32) * O.noise_z(99, 1, 6, 7) * 2.0 ** -16
    assert np.allclose(pre, want[None], rtol=0, atol=1e-15)


def test_the_noise_is_drawn_in_the_output_frame():
    x = np.full((2, 1, 4, 6), 0.5)
    t = O.neutral_table(2, 0.5)
    t[:, 4] = 0.05
    t[:, 6] = np.array([7, 7], dtype=np.uint32).view(np.float32)
    pre, _ = O.apply(x, [0, 3], t)
    assert np.array_equal(pre[0], pre[1])  # a constant image: the flip moves nothing, and the noise does not follow it


# ---------------------------------------------------------------------------------------------------------- config
def test_the_defaults_and_their_normal_form():
    from spcl_amd import functional as F_hip
    cfg = _cfg()
    assert cfg.p16 == [19661, 32768, 32768, 13107, 9830]
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    assert cfg.lo == [f32(0.7), 0.75, 0.75, 0.25, 0.0] and cfg.hi == [1.5, 1.25, 1.25, 1.0, f32(0.05)]
    assert tuple(name for name, *_ in cfg.key()) == F_hip.STRONG_VIEW_OPS == OPS
    w = list(cfg.words())
    assert len(w) == 15 and w[0::3] == cfg.p16
    assert [struct.unpack("<f", struct.pack("<i", v))[0] for v in w[1::3]] == cfg.lo
    assert [struct.unpack("<f", struct.pack("<i", v))[0] for v in w[2::3]] == cfg.hi
    assert cfg == _cfg(gamma={"p": 0.3}) and hash(cfg) == hash(_cfg()) and cfg != _cfg(gamma={"p": 0.31})
    off = F_hip.StrongViewConfig.off()
    assert off.p16 == [0] * 5 and off.lo == cfg.lo
    assert _cfg(blur={"p": 1, "range": [0, 1]}).p16[3] == 65536
    assert "gamma" in repr(cfg)


def test_config_refuses_an_unknown_op():
    with pytest.raises(ValueError, match="sharpen"):
        _cfg(sharpen={"p": 0.5})


def test_config_refuses_an_unknown_key_of_an_op():
    with pytest.raises(ValueError, match="gamma.*sigma"):
        _cfg(gamma={"p": 0.5, "sigma": 1.0})


def test_config_refuses_a_section_that_is_no_mapping():
    with pytest.raises(ValueError, match="contrast must be a mapping"):
        _cfg(contrast=0.5)


@pytest.mark.parametrize("p", [-0.1, 1.5, "often", True, None])
def test_config_refuses_a_bad_probability(p):
    with pytest.raises(ValueError, match="noise p"):
        _cfg(noise={"p": p})


@pytest.mark.parametrize("rng", [0.5, (0.5,), (0.5, 1.0, 1.5), ("a", "b"), None, (1e60, 1e61)])
def test_config_refuses_a_range_that_is_no_pair_of_float32(rng):
    with pytest.raises(ValueError, match="brightness range"):
        _cfg(brightness={"range": rng})


def test_config_refuses_lo_above_hi():
    with pytest.raises(ValueError, match="contrast range.*lo <= hi"):
        _cfg(contrast={"range": (1.25, 0.75)})


def test_config_refuses_a_nan_or_infinite_range():
    for rng in ((float("nan"), 1.0), (0.5, float("inf"))):
        with pytest.raises(ValueError, match="gamma range"):
            _cfg(gamma={"range": rng})


@pytest.mark.parametrize("op", ["gamma", "brightness"])
def test_config_refuses_a_non_positive_gamma_or_brightness(op):
    for lo in (0.0, -0.5):
        with pytest.raises(ValueError, match=f"{op} range.*above 0"):
            _cfg(**{op: {"range": (lo, 1.5)}})


@pytest.mark.parametrize("op", ["contrast", "noise"])
def test_config_refuses_a_negative_contrast_or_noise(op):
    with pytest.raises(ValueError, match=f"{op} range.*negative"):
        _cfg(**{op: {"range": (-0.01, 0.05)}})
    _cfg(**{op: {"range": (0.0, 0.05)}})


def test_config_refuses_a_blur_beyond_the_filter():
    for rng in ((-0.1, 0.5), (0.5, 1.01)):
        with pytest.raises(ValueError, match=r"blur range.*\[0, 1\]"):
            _cfg(blur={"range": rng})


# ------------------------------------------------------------------------------------------------------------ hook
def _model():
    from spcl_amd.semi_seg.arch import UNet
    torch.manual_seed(0)
    return UNet(input_dim=1, num_classes=4, max_channel=128)


def _config(**sections):
    return dict({"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 30}}, **sections)


def test_config_section_builds_the_hook():
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.hooks import StrongViewTrainerHook
    model = _model()
    (hook,) = create_hook_from_config(model, _config(StrongViewParameters={}))
    assert isinstance(hook, StrongViewTrainerHook) and hook._hook_name == "strongview"
    assert hook.config == _cfg() and hook.draw.tolist() == [0] and hook.draw.dtype == torch.int32
    assert list(hook.parameters()) == [] and hook.learnable_modules == []
    section = {"seed": 11, "gamma": {"p": 1.0, "range": [0.5, 2.0]}, "noise": {"p": 0.0}}
    (hook,) = create_hook_from_config(model, _config(StrongViewParameters=section))
    assert hook.draw.tolist() == [11] and hook.config == _cfg(gamma={"p": 1.0, "range": (0.5, 2.0)}, noise={"p": 0.0})
    eh = hook()
    assert eh.contributes_loss is False and eh.graph_key() == ("_StrongViewEpocherHook", hook.config.key())
    assert eh.graph_key() == create_hook_from_config(model, _config(StrongViewParameters=dict(section, seed=12)))[0]().graph_key()
    both = create_hook_from_config(model, _config(PseudoLabelParameters={"weight": 1.0}, StrongViewParameters={}))
    assert [type(h).__name__ for h in both] == ["PseudoLabelTrainerHook", "StrongViewTrainerHook"]
    with pytest.raises(RuntimeError, match="StrongViewParameters are not supported for pretrain"):
        create_hook_from_config(model, _config(StrongViewParameters={}), is_pretrain=True)


def test_the_section_refuses_an_unknown_key_by_name():
    from spcl_amd.hook_creator import create_hook_from_config
    with pytest.raises(ValueError, match="sharpness"):
        create_hook_from_config(_model(), _config(StrongViewParameters={"sharpness": {"p": 0.1}}))


@pytest.mark.parametrize("seed", [-1, 2 ** 31, 1.5, True, "0"])
def test_the_hook_refuses_a_bad_seed(seed):
    from spcl_amd.semi_seg.hooks import StrongViewTrainerHook
    with pytest.raises(ValueError, match="seed"):
        StrongViewTrainerHook("strongview", seed=seed)


def test_the_hook_refuses_a_config_beside_op_sections_and_a_config_of_another_type():
    from spcl_amd.semi_seg.hooks import StrongViewTrainerHook
    with pytest.raises(ValueError, match="both"):
        StrongViewTrainerHook("strongview", config=_cfg(), gamma={"p": 0.1})
    with pytest.raises(ValueError, match="StrongViewConfig"):
        StrongViewTrainerHook("strongview", config={"gamma": {"p": 0.1}})
    assert StrongViewTrainerHook("strongview", config=_cfg(**_all(0.0))).config.p16 == [0] * 5


def test_the_draw_buffer_round_trips_through_state_dict():
    from spcl_amd.semi_seg.hooks import StrongViewTrainerHook
    hook = StrongViewTrainerHook("strongview", seed=5)
    assert sorted(hook.state_dict()) == ["draw"]
    hook.draw.add_(3)
    sd = {k: v.clone() for k, v in hook.state_dict().items()}
    late = StrongViewTrainerHook("strongview", seed=99)
    late.load_state_dict(sd)
    assert late.draw.tolist() == [8] and late.draw.dtype == torch.int32
    assert late.seed_word(torch.device("cpu")) is late.draw


class _Meters(dict):
    def register_meter(self, key, meter):
        self[key] = meter

    def focus_on(self, name):
        return nullcontext()


def _bare(cls):
    """an epocher of ``cls`` with the two attributes ``add_hook`` touches"""
    ep = cls.__new__(cls)
    ep._hooks, ep.meters = [], _Meters()
    return ep


def test_the_epocher_refuses_two_strong_view_hooks():
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    from spcl_amd.semi_seg.hooks import StrongViewTrainerHook, create_consistency_hook
    ep = _bare(SemiSupervisedEpocher)
    ep.add_hook(create_consistency_hook(1.0)())
    first = StrongViewTrainerHook("strongview")()
    ep.add_hook(first)
    assert "ops" in ep.meters
    with pytest.raises(ValueError, match="second hook offers `strong_view`"):
        ep.add_hook(StrongViewTrainerHook("strongview2", seed=1)())
    assert len(ep._hooks) == 2 and ep._hooks[1] is first and ep._strong_view is first


def test_the_epocher_refuses_a_strong_view_hook_inside_a_combined_hook():
    """a CombineEpochHook sums its members' results, and this hook has none to add"""
    from spcl_amd.contrastyou.hooks.base import CombineEpochHook
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    from spcl_amd.semi_seg.hooks import StrongViewTrainerHook, create_consistency_hook
    ep = _bare(SemiSupervisedEpocher)
    inner = CombineEpochHook(create_consistency_hook(1.0)(), StrongViewTrainerHook("strongview3")())
    for hook in (inner, CombineEpochHook(create_consistency_hook(1.0)(), inner)):
        with pytest.raises(ValueError, match="inside a combined hook"):
            ep.add_hook(hook)
    assert ep._hooks == [] and ep._strong_view is None and "ops" not in ep.meters


@pytest.mark.parametrize("name", ["MixUpEpocher", "AdversarialEpocher"])
def test_epochers_without_an_unlabelled_pair_refuse_the_hook(name):
    from spcl_amd.semi_seg.epochers import mixup
    from spcl_amd.semi_seg.hooks import StrongViewTrainerHook
    ep = _bare(getattr(mixup, name))
    with pytest.raises(RuntimeError, match=f"{name} runs a step of its own.*no second view"):
        ep.add_hook(StrongViewTrainerHook("strongview")())
    assert "ops" not in ep.meters


def test_a_hook_that_contributes_no_loss_is_called_and_left_out_of_the_sum():
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    calls = []

    class Silent:
        contributes_loss = False

        def __call__(self, **kwargs):
            calls.append(("silent", sorted(kwargs)))
            return None

    class Loud:
        def __init__(self, v):
            self.v = v

        def __call__(self, **kwargs):
            calls.append(("loud", sorted(kwargs)))
            return torch.tensor(self.v)

    ep = SemiSupervisedEpocher.__new__(SemiSupervisedEpocher)
    ep._device = torch.device("cpu")
    ep._hooks = [Silent()]
    zero = ep._regularization(seed=1)
    assert zero.shape == () and zero.dtype == torch.float32 and float(zero) == 0.0 and calls == [("silent", ["seed"])]
    ep._hooks = [Loud(1.5), Silent(), Loud(2.0)]
    assert float(ep._regularization(seed=1)) == 3.5 and [c[0] for c in calls[1:]] == ["loud", "silent", "loud"]
    ep._hooks = [Loud(1.5)]
    assert float(ep._regularization(seed=1)) == 1.5
    ep._hooks = []
    assert float(ep._regularization(seed=1)) == 0.0
