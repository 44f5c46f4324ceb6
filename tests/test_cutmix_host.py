"""CPU: CutMix for cross pseudo supervision is wired in -- header, binding and library agree on the C ABI (>= 36) and export the
four entry points of csrc/cutmix.hip, whose argument checks answer with an error code and a message before any device call;
the workspace grows with the pixels; the functionals have no CPU path; the oracle's box rule hits its fixed points, keeps every
box inside its image and reaches both ends of the area range; the oracle without boxes is ``_cps_oracle``'s; the config section
builds the hook (defaults, the section without the map name is refused, ``draw`` and ``mixed`` exist only with CutMix on, the
five-element graph key) and is refused during pre-training."""
import ctypes
import os
import re
from contextlib import nullcontext

import pytest
import torch

from tests import _cps_oracle as CO
from tests import _cutmix_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("spcl_cutmix_boxes", "spcl_cutmix_images", "spcl_cross_pseudo_mixed_workspace_bytes", "spcl_cross_pseudo_ce_mixed")


def _config(**sections):
    return dict({"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 30}}, **sections)


def _model(seed=0):
    from spcl_amd.semi_seg.arch import UNet
    torch.manual_seed(seed)
    return UNet(input_dim=1, num_classes=4, max_channel=128)


def test_header_binding_and_library_agree_and_export_the_entry_points():
    from spcl_amd import native
    header = open(os.path.join(ROOT, "include", "spcl_hip.h")).read()
    version = int(re.search(r"#define SPCL_ABI_VERSION (\d+)", header).group(1))
    L = native.lib()
    assert version == native.ABI_VERSION == L.spcl_abi_version() and version >= 36
    for name in ENTRIES:
        assert name in native._SIGNATURES and name in header
        assert getattr(L, name, None) is not None, name
    res, args = native._SIGNATURES["spcl_cross_pseudo_ce_mixed"]
    assert res is ctypes.c_int and len(args) == 22
    assert args[4:8] == [ctypes.c_int] * 4 and args[9] is ctypes.c_int and args[11] is ctypes.c_float
    assert args[20] is ctypes.c_size_t
    assert len(native._SIGNATURES["spcl_cutmix_boxes"][1]) == 8 and len(native._SIGNATURES["spcl_cutmix_images"][1]) == 11
    # the sibling keeps its signature
    assert len(native._SIGNATURES["spcl_cross_pseudo_ce"][1]) == 18


def test_workspace_grows_with_the_pixels_and_refuses_what_the_entry_refuses():
    from spcl_amd import native
    ws = native.lib().spcl_cross_pseudo_mixed_workspace_bytes
    assert 0 < ws(1, 4, 8, 8) < ws(2, 4, 192, 200) < ws(10, 4, 224, 224)
    assert ws(10, 2, 224, 224) < ws(10, 4, 224, 224) < ws(10, 16, 224, 224)
    # one row of 2 doubles and 4 C + 2 counters per 1024 pixels, and the ticket
    nblk = (10 * 224 * 224 + 1023) // 1024
    assert ws(10, 4, 224, 224) >= nblk * (2 * 8 + 18 * 4) + 4
    assert ws(1, 17, 8, 8) == 0 and ws(1, 0, 8, 8) == 0 and ws(0, 4, 8, 8) == 0 and ws(1, 4, 0, 8) == 0 and ws(1, 4, 8, -1) == 0
    assert ws(32768, 4, 256, 256) == 0  # N H W == 2^31
    assert ws(32767, 4, 256, 256) > 0


def test_the_criterion_entry_reports_its_refusals():
    """every refusal below happens on the host, before any device call: an error code and a message, not a crash"""
    from spcl_amd import native
    L = native.lib()
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)  # never dereferenced: each call is refused before a launch

    def call(C=4, sa=fake, sb=fake, ta=fake, tb=fake, boxes=fake, roll=1, loss=fake, parts=fake, da=fake, db=other, hist=fake,
             ws=fake, ws_bytes=1 << 20, N=3, H=20, W=24):
        return L.spcl_cross_pseudo_ce_mixed(sa, sb, ta, tb, N, C, H, W, boxes, roll, None, ctypes.c_float(1.0), loss, parts, da,
                                            db, hist, None, None, ws, ws_bytes, None)

    for kwargs, word in (({"C": 17}, b"C <= 16"), ({"C": 0}, b"C <= 16"), ({"N": 0}, b"bad shape"), ({"H": 0}, b"bad shape"),
                         ({"W": -1}, b"bad shape"), ({"sa": None}, b"null"), ({"sb": None}, b"null"), ({"ta": None}, b"null"),
                         ({"tb": None}, b"null"), ({"loss": None}, b"null"), ({"parts": None}, b"null"), ({"da": None}, b"null"),
                         ({"db": None}, b"null"), ({"hist": None}, b"null"), ({"ws": None}, b"null"),
                         ({"N": 32768, "H": 256, "W": 256}, b"too many pixels"), ({"ws_bytes": 64}, b"workspace"),
                         ({"db": fake}, b"one buffer"), ({"ws": ctypes.c_void_p(4100)}, b"aligned"),
                         ({"roll": 0}, b"roll"), ({"roll": 3}, b"roll"), ({"roll": -1}, b"roll"), ({"N": 1}, b"roll")):
        assert call(**kwargs) == -1, kwargs
        assert word in L.spcl_last_error(), (kwargs, L.spcl_last_error())


def test_the_box_and_image_entries_report_their_refusals():
    from spcl_amd import native
    L = native.lib()
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)

    def boxes(seed=fake, N=3, H=20, W=24, lo=16384, hi=32768, out=fake):
        return L.spcl_cutmix_boxes(seed, N, H, W, lo, hi, out, None)

    for kwargs, word in (({"seed": None}, b"null"), ({"out": None}, b"null"), ({"N": 0}, b"N = 0"), ({"N": (1 << 20) + 1}, b"2^20"),
                         ({"H": 0}, b"bad shape"), ({"W": -3}, b"bad shape"), ({"lo": 0}, b"bad range"),
                         ({"lo": 40000}, b"bad range"), ({"hi": 65537}, b"bad range"), ({"lo": -1, "hi": -1}, b"bad range")):
        assert boxes(**kwargs) == -1, kwargs
        assert word in L.spcl_last_error(), (kwargs, L.spcl_last_error())

    def images(x=fake, out=other, dtype=0, N=3, C=1, H=20, W=24, cl=0, bx=fake, roll=1):
        return L.spcl_cutmix_images(x, out, dtype, N, C, H, W, cl, bx, roll, None)

    for kwargs, word in (({"x": None}, b"null"), ({"out": None}, b"null"), ({"bx": None}, b"null"), ({"dtype": 2}, b"dtype"),
                         ({"N": 0}, b"bad shape"), ({"C": 0}, b"bad shape"), ({"H": -1}, b"bad shape"), ({"W": 0}, b"bad shape"),
                         ({"N": 32768, "H": 256, "W": 256}, b"too many"), ({"out": fake}, b"one buffer"),
                         ({"roll": 0}, b"roll"), ({"roll": 3}, b"roll"), ({"N": 1}, b"roll")):
        assert images(**kwargs) == -1, kwargs
        assert word in L.spcl_last_error(), (kwargs, L.spcl_last_error())


def test_the_functionals_have_no_cpu_path():
    from spcl_amd import functional as F_hip
    t = torch.zeros(2, 4, 8, 8)
    bx = torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.cross_pseudo_ce_mixed(t, t, t, t, bx, 1)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.cutmix_images(torch.zeros(2, 1, 8, 8), bx, 1)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.cutmix_boxes(0, 2, 8, 8, device="cpu")
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.cutmix_boxes(torch.zeros(1, dtype=torch.int32), 2, 8, 8)
    # what the host refuses, it refuses before it looks for a device
    with pytest.raises(ValueError, match="prop_range"):
        F_hip.cutmix_boxes(0, 2, 8, 8, (0.0, 0.5), device="cpu")
    with pytest.raises(ValueError, match="prop_range"):
        F_hip.cutmix_boxes(0, 2, 8, 8, (0.6, 0.5), device="cpu")
    with pytest.raises(ValueError, match="seed"):
        F_hip.cutmix_boxes(2 ** 32, 2, 8, 8, device="cpu")


# ------------------------------------------------------------------------------------------------------------------ oracle
def test_the_oracle_hits_the_fixed_boxes():
    assert O.boxes(23, 3, 20, 24).tolist() == [[6, 8, 14, 10], [2, 11, 18, 12], [5, 3, 9, 17]]
    assert O.key(0, 0) != O.key(1, 0) and 0 <= O.key(5, 2 ** 32 - 1) < 2 ** 32
    from tests import _pixel_contrast_oracle as PO  # the sampler's keys: one hash for both
    for seed in (0, 23, 2 ** 31 + 5, 2 ** 32 - 1):
        assert [O.key(i, seed) for i in range(40)] == [int(v) for v in PO.keys(40, seed)]
    # the binding's units: round(p * 65536)
    assert (O.share16(0.25), O.share16(0.5), O.share16(1.0), O.share16(1 / 65536)) == (16384, 32768, 65536, 1)


@pytest.mark.parametrize("hw", [(5, 7), (9, 33), (224, 224)])
def test_oracle_boxes_lie_inside_the_image_and_keep_the_area_range(hw):
    H, W = hw
    lo16, hi16 = O.share16(0.25), O.share16(0.5)
    shares, tall = [], 0
    for k in range(2000):
        seed, n = (k * 2654435761 + 12345) % 2 ** 32, k % 7
        y0, x0, bh, bw = O.box(n, seed, H, W, lo16, hi16)
        assert 0 <= y0 and 0 <= x0 and 1 <= bh and 1 <= bw and y0 + bh <= H and x0 + bw <= W, (seed, n)
        shares.append(bh * bw / (H * W))
        tall += bh * W > bw * H
    if hw == (224, 224):  # (side rounding moves a share by less than (bh + bw + 1) / (H W) < 0.5 % there)
        assert 0.245 <= min(shares) and max(shares) <= 0.505, (min(shares), max(shares))
        assert 0.36 <= sum(shares) / len(shares) <= 0.39
        assert 0.45 <= tall / 2000 <= 0.55


def test_oracle_boxes_at_the_ends_of_the_range():
    for H, W in ((5, 7), (9, 33), (224, 224)):
        for seed in (0, 23, 2 ** 31 + 5):
            assert O.boxes(seed, 4, H, W, (1.0, 1.0)).tolist() == [[0, 0, H, W]] * 4
    # The smallest share, P = 1: the side shares S, T = 65536 / S multiply to it, so ONE side rounds to less than a pixel and is
    # raised to 1 -- a strip one pixel thin, whatever the other side is (S is uniform in [1, 65535]).  Both sides are 1 only
    # where the longer one rounds below 1.5 pixels too: 513 of 2100 draws on 5 x 7 (seeds 0 .. 299), never all of them.
    tiny = 1 / 65536
    sizes = set()
    for seed in range(50):
        b = O.boxes(seed, 7, 5, 7, (tiny, tiny))
        assert bool((b[:, 2:].min(dim=1).values == 1).all()), b.tolist()
        assert bool((b[:, 0] >= 0).all() and (b[:, 0] + b[:, 2] <= 5).all())
        assert bool((b[:, 1] >= 0).all() and (b[:, 1] + b[:, 3] <= 7).all())
        sizes |= {tuple(r) for r in b[:, 2:].tolist()}
    assert (1, 1) in sizes and (5, 1) in sizes and (1, 7) in sizes  # from a single pixel to a whole row or column


def test_the_src_map_and_the_gather():
    bx = torch.tensor([[1, 2, 2, 3], [0, 0, 1, 1], [2, 0, 1, 4]], dtype=torch.int32)
    m = O.src(bx, 3, 3, 4, roll=1)
    assert m[0].tolist() == [[0, 0, 0, 0], [0, 0, 1, 1], [0, 0, 1, 1]]
    assert m[1].tolist() == [[2, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]]
    assert m[2].tolist() == [[2, 2, 2, 2], [2, 2, 2, 2], [0, 0, 0, 0]]
    assert torch.equal(O.src(None, 3, 3, 4), torch.arange(3).view(3, 1, 1).expand(3, 3, 4))
    assert O.src(bx, 3, 3, 4, roll=2)[0, 1, 2] == 2
    t = torch.arange(3 * 2 * 3 * 4, dtype=torch.float32).view(3, 2, 3, 4)
    g = O.gather(t, m)
    assert torch.equal(g[0, :, 0, 0], t[0, :, 0, 0]) and torch.equal(g[0, :, 1, 2], t[1, :, 1, 2])
    assert torch.equal(g[2, :, 2, 3], t[0, :, 2, 3])
    assert torch.equal(O.mix_images(t, bx, 1), g)  # the image mix is the same gather


def test_every_slab_boundary_of_the_large_maps_has_pixels_inside_a_box_around_it():
    """what the shapes are chosen for, on the oracle alone: boxes cross slab boundaries (a teacher pixel read from another
    sample on either side of a workgroup's edge)"""
    for shape in ((2, 4, 64, 66), (10, 4, 224, 224), (2, 3, 40, 52)):
        N, _, H, W = shape
        flat = O.inside(O.boxes(23, N, H, W), H, W).flatten()
        edges = torch.arange(1024, flat.numel(), 1024)
        crossed = flat[edges] & flat[edges - 1]
        assert int(crossed.sum()) >= 3, (shape, int(crossed.sum()))


@pytest.mark.parametrize("weight", [1.0, 2.5])
def test_the_oracle_without_boxes_and_with_the_students_as_teachers_is_the_cps_oracle(weight):
    g = torch.Generator().manual_seed(23)
    a, b = 3.0 * torch.randn(2, 3, 5, 7, generator=g), 3.0 * torch.randn(2, 3, 5, 7, generator=g)
    confA, yA, confB, yB = O.teachers(a, b, None)
    (wantA, wyA), (wantB, wyB) = CO.conf_and_label(a), CO.conf_and_label(b)
    assert torch.equal(confA, wantA) and torch.equal(yA, wyA) and torch.equal(confB, wantB) and torch.equal(yB, wyB)
    keepA, keepB = confA >= 0.6, confB >= 0.6
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    got = O.loss(a64, b64, yA, yB, keepA, keepB, weight)
    want = CO.loss(a.double(), b.double(), yA, yB, keepA, keepB, weight)
    assert float(got.detach()) == float(want)
    got.backward()
    assert bool(a64.grad.any()) and bool(b64.grad.any())
    h = O.hist(yA, yB, keepA, keepB, 3, None)
    assert h.shape == (14,) and torch.equal(h[:13], CO.hist(yA, yB, keepA, keepB, 3)) and int(h[13]) == 0
    # with boxes the labels come from the next sample inside them, and the count of inside pixels is the boxes' area
    bx = O.boxes(23, 2, 5, 7)
    _, yA2, _, _ = O.teachers(a, b, bx, 1)
    inside = O.inside(bx, 5, 7)
    assert torch.equal(yA2[inside], wyA.roll(-1, 0)[inside]) and torch.equal(yA2[~inside], wyA[~inside])
    assert int(O.hist(yA2, yB, keepA, keepB, 3, bx)[13]) == int((bx[:, 2] * bx[:, 3]).sum())


# -------------------------------------------------------------------------------------------------------------------- hook
def test_config_section_builds_the_hook():
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.hooks import CrossPseudoTrainerHook, create_cross_pseudo_hook
    from spcl_amd.semi_seg.hooks.cps import MAPS
    assert MAPS == ("labeled", "unlabeled", "unlabeled_tf", "cutmix")
    model = _model()
    params = {"weight": 1.5, "threshold": 0.8, "on": ["unlabeled", "cutmix"], "cutmix": {"prop_range": [0.1, 0.3], "seed": 11}}
    (hook,) = create_hook_from_config(model, _config(CrossPseudoParameters=params))
    assert isinstance(hook, CrossPseudoTrainerHook) and hook._on == ("unlabeled", "cutmix") and hook.cutmix
    assert hook._prop_range == (0.1, 0.3)
    assert hook.draw.dtype == torch.int32 and hook.draw.tolist() == [11] and hook.seed_word(torch.device("cpu")) is hook.draw
    assert "draw" in hook.state_dict() and hook.state_dict()["draw"].tolist() == [11]
    assert hook().graph_key() == ("_CrossPseudoEpocherHook", 1.5, ("unlabeled", "cutmix"), "tau", (0.1, 0.3))
    with pytest.raises(RuntimeError):
        create_hook_from_config(model, _config(CrossPseudoParameters=params), is_pretrain=True)
    # the map name without the section: the defaults
    only = create_cross_pseudo_hook(model=model, weight=2.0, on=["cutmix"])
    assert only._on == ("cutmix",) and only._prop_range == (0.25, 0.5) and only.draw.tolist() == [0]
    assert only().graph_key() == ("_CrossPseudoEpocherHook", 2.0, ("cutmix",), "plain", (0.25, 0.5))
    part = create_cross_pseudo_hook(model=model, weight=2.0, on=["cutmix"], cutmix={"seed": 5})
    assert part._prop_range == (0.25, 0.5) and part.draw.tolist() == [5]
    # the section without the map name: refused, and the message names what is missing
    with pytest.raises(ValueError, match='"cutmix"'):
        create_cross_pseudo_hook(model=model, weight=2.0, cutmix={"seed": 5})
    with pytest.raises(ValueError, match='"cutmix"'):
        create_hook_from_config(model, _config(CrossPseudoParameters={"weight": 1.0, "on": ["labeled"], "cutmix": {}}))
    for bad in ({"prop_range": [0.0, 0.5]}, {"prop_range": [0.5, 0.25]}, {"prop_range": [0.5, 1.5]}, {"prop_range": 0.5},
                {"prop_range": [0.1, 0.2, 0.3]}):
        with pytest.raises(ValueError, match="prop_range"):
            create_cross_pseudo_hook(model=model, weight=1.0, on=["cutmix"], cutmix=bad)
    for bad in ({"seed": -1}, {"seed": 2 ** 31}, {"seed": 1.5}, {"seed": True}):
        with pytest.raises(ValueError, match="seed"):
            create_cross_pseudo_hook(model=model, weight=1.0, on=["cutmix"], cutmix=bad)
    with pytest.raises(ValueError, match="no key"):
        create_cross_pseudo_hook(model=model, weight=1.0, on=["cutmix"], cutmix={"prop": [0.25, 0.5]})
    with pytest.raises(ValueError, match="twice"):
        create_cross_pseudo_hook(model=model, weight=1.0, on=["cutmix", "cutmix"])


def test_draw_mixed_and_the_fifth_key_element_exist_only_with_cutmix_on():
    from spcl_amd.semi_seg.hooks import CrossPseudoTrainerHook

    class _Meters(dict):
        def register_meter(self, key, meter):
            self[key] = meter

        def focus_on(self, name):
            return nullcontext()

    def meters_of(hook):
        class Epocher:
            meters = _Meters()

        ep = Epocher()
        hook().set_epocher(ep)
        return sorted(ep.meters)

    model = _model()
    plain = CrossPseudoTrainerHook("cps", 1.0, model)
    assert not plain.cutmix and plain._on == ("labeled", "unlabeled", "unlabeled_tf")  # never part of the default
    assert not hasattr(plain, "draw") and "draw" not in plain.state_dict()
    assert sorted(k for k in plain.state_dict() if not k.startswith("_peer.")) == ["tau"]
    assert meters_of(plain) == ["agree", "kept", "loss", "peer_sup_loss"]
    assert len(plain().graph_key()) == 4
    mixed = CrossPseudoTrainerHook("cps", 1.0, model, on=("labeled", "unlabeled", "unlabeled_tf", "cutmix"))
    assert mixed.cutmix and sorted(k for k in mixed.state_dict() if not k.startswith("_peer.")) == ["draw", "tau"]
    assert meters_of(mixed) == ["agree", "kept", "loss", "mixed", "peer_sup_loss"]
    assert len(mixed().graph_key()) == 5 and mixed().graph_key()[:4] == plain().graph_key()[:2] + (mixed._on, "plain")
    # the seed word travels in the state dict
    late = CrossPseudoTrainerHook("cps", 1.0, model, on=("cutmix",), cutmix={"seed": 9})
    mixed.draw.add_(3)
    late.load_state_dict(mixed.state_dict())
    assert late.draw.tolist() == [3]


def test_class_maps_of_another_size_than_the_images_are_refused():
    """the boxes are drawn for the images and applied to the class maps: a network whose output is smaller than its input is a
    RuntimeError that says so, before a box is drawn"""
    from spcl_amd.semi_seg.hooks import CrossPseudoTrainerHook

    class _Meters(dict):
        def register_meter(self, key, meter):
            self[key] = meter

        def focus_on(self, name):
            return nullcontext()

    class Epocher:
        meters = _Meters()

    owner = CrossPseudoTrainerHook("cps", 1.0, _model(), on=("cutmix",), cutmix={"seed": 4})
    hook = owner()
    hook.set_epocher(Epocher())
    image, full, half = torch.zeros(2, 1, 8, 8), torch.zeros(2, 4, 8, 8), torch.zeros(2, 4, 4, 4)
    for mine, theirs in ((half, full), (full, half), (half, half)):
        with pytest.raises(RuntimeError, match="input's size"):
            hook._cutmix_term(image, mine, theirs, None, 1.0, [])
    assert owner.draw.tolist() == [4]


def test_the_epocher_has_the_forward_for_one_unlabelled_batch():
    """``_forward_unlabeled`` runs a given network once; under ``two_stage`` inside ``_bn_context`` of THAT network"""
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    events = []

    class Net:
        def __init__(self, name):
            self.name = name

        def __call__(self, image):
            events.append(("forward", self.name, image))
            return ("logits", self.name)

        def set_bn_track(self, flag):
            events.append(("bn_track", self.name, flag))
            return nullcontext()

    ep = SemiSupervisedEpocher.__new__(SemiSupervisedEpocher)
    model, peer = Net("model"), Net("peer")
    ep._model, ep._two_stage, ep._disable_bn = model, False, True
    assert ep._forward_unlabeled("x") == ("logits", "model") and events == [("forward", "model", "x")]
    events.clear()
    ep._two_stage = True
    assert ep._forward_unlabeled("x", model=peer) == ("logits", "peer")
    assert events == [("bn_track", "peer", False), ("forward", "peer", "x")]
    events.clear()
    ep._disable_bn = False
    assert ep._forward_unlabeled("y") == ("logits", "model") and events == [("forward", "model", "y")]
