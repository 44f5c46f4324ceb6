"""The Prostate data seam on the GPU: `spcl_resize_nearest_pil` (label maps through ``Image.resize(NEAREST)``) bit for bit
against PIL and tests/golden/g14_prostate_resize.npz, ``RecipeViews`` with label maps under the Prostate recipes, and
``get_data({"name": "prostate"})`` end to end -- a 240^2 store the product resizes itself against the same slices resized by
PIL on the host, then one ``FineTuneTrainer`` epoch."""
import functools
import math
import random
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import spcl_oracle as O
from tests import _prostate_oracle as PO


def _mods():
    import spcl_amd  # noqa: F401
    from spcl_amd import native as _n
    from spcl_amd.semi_seg.data import augment as A
    return A, _n


# ---- the kernel
@pytest.mark.parametrize("case", range(7))
def test_resize_labels_is_pils_nearest(case):
    """every case of g14 -- (97,130) -> 50x67 (an odd width: byte stores), 64^2 -> 224^2 (repeated indices), 240^2 -> 224^2
    (blobs and per-pixel random), (256,320) -> (224,280), (320,256) -> (280,224), 1x1 -> 3x3 --: the fixture's bits, and
    PIL's of today"""
    A, _ = _mods()
    g = PO.g14()
    h, w, oh, ow = g["shapes"][case].tolist()
    lab = g[f"label{case}"]
    got = A.resize_labels(torch.from_numpy(lab).cuda()[None], min(oh, ow))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, oh, ow)
    np.testing.assert_array_equal(got[0].cpu().numpy(), g[f"resized{case}"])
    np.testing.assert_array_equal(got[0].cpu().numpy(), PO.pil_resize_nearest(lab, (oh, ow)))


def test_resize_labels_returns_its_argument_when_nothing_changes():
    A, _ = _mods()
    t = torch.zeros(2, 224, 224, dtype=torch.uint8, device="cuda")
    assert A.resize_labels(t, 224) is t
    wide = torch.zeros(2, 224, 280, dtype=torch.uint8, device="cuda")
    assert A.resize_labels(wide, 224) is wide


@pytest.mark.parametrize("hw,size", [((97, 130), 50), ((60, 44), 32), ((60, 44), 36)])
def test_resize_labels_five_slices(hw, size):
    """S = 5 different per-pixel random maps (slice stride of source and output; 50x67: byte stores, 43x32: 128-bit
    stores, 49x36: 32-bit stores)"""
    A, _ = _mods()
    labs = np.random.RandomState(hw[0]).randint(0, 4, size=(5, *hw)).astype(np.uint8)
    oh, ow = A.resize_shorter_edge(hw, size)
    got = A.resize_labels(torch.from_numpy(labs).cuda(), size).cpu().numpy()
    for k in range(5):
        np.testing.assert_array_equal(got[k], PO.pil_resize_nearest(labs[k], (oh, ow)), err_msg=f"slice {k}")


def _launch(_n, A, src, S, HS, WS, out, OH, OW):
    tx = torch.tensor(A.nearest_resize_table(WS, OW), dtype=torch.int32).cuda()
    ty = torch.tensor(A.nearest_resize_table(HS, OH), dtype=torch.int32).cuda()
    _n.call("spcl_resize_nearest_pil", _n.ptr(src), S, HS, WS, _n.ptr(tx), _n.ptr(ty), _n.ptr(out), OH, OW, _n.stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("lead", [16, 1, 2])
@pytest.mark.parametrize("hw,ohw", [((30, 30), (24, 24)), ((30, 41), (24, 33)), ((40, 44), (27, 32))])
def test_resize_nearest_unaligned_views_and_guard_bytes(lead, hw, ohw):
    """source and output are views that start `lead` bytes into their buffers (16: aligned -- 128-bit stores at width 32,
    32-bit stores at width 24, byte stores at width 33 --; 1 and 2: byte stores whatever the width): the result is PIL's, the
    bytes in front of and behind the output keep their pattern, and a second run gives the same bits"""
    A, _n = _mods()
    S, (HS, WS), (OH, OW) = 3, hw, ohw
    labs = np.random.RandomState(lead + WS).randint(0, 4, size=(S, HS, WS)).astype(np.uint8)
    sbuf = torch.zeros(lead + S * HS * WS + 8, dtype=torch.uint8, device="cuda")
    src = sbuf[lead:lead + S * HS * WS]
    src.copy_(torch.from_numpy(labs).cuda().reshape(-1))
    n = S * OH * OW
    obuf = torch.full((lead + n + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    out = obuf[lead:lead + n]
    assert out.data_ptr() % 16 == lead % 16 and src.data_ptr() % 16 == lead % 16
    _launch(_n, A, src, S, HS, WS, out, OH, OW)
    first = obuf.clone()
    got = out.reshape(S, OH, OW).cpu().numpy()
    for k in range(S):
        np.testing.assert_array_equal(got[k], PO.pil_resize_nearest(labs[k], (OH, OW)), err_msg=f"slice {k}")
    assert int((obuf[:lead] != 0xAB).sum()) == 0 and int((obuf[lead + n:] != 0xAB).sum()) == 0
    _launch(_n, A, src, S, HS, WS, out, OH, OW)
    assert torch.equal(obuf, first)


def test_resize_nearest_refuses_bad_arguments():
    A, _n = _mods()
    src = torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda")
    out = torch.zeros(1, 4, 4, dtype=torch.uint8, device="cuda")
    tab = torch.zeros(8, dtype=torch.int32, device="cuda")
    p, st = _n.ptr, _n.stream()
    for args in ((None, 1, 8, 8, p(tab), p(tab), p(out), 4, 4, st), (p(src), 1, 8, 8, None, p(tab), p(out), 4, 4, st),
                 (p(src), 1, 8, 8, p(tab), None, p(out), 4, 4, st), (p(src), 1, 8, 8, p(tab), p(tab), None, 4, 4, st)):
        with pytest.raises(RuntimeError, match="null pointer"):
            _n.call("spcl_resize_nearest_pil", *args)
    for S, HS, WS, OH, OW in ((0, 8, 8, 4, 4), (1, 0, 8, 4, 4), (1, 8, 0, 4, 4), (1, 8, 8, 0, 4), (1, 8, 8, 4, 0), (-1, 8, 8, 4, 4)):
        with pytest.raises(RuntimeError, match="bad shape"):
            _n.call("spcl_resize_nearest_pil", p(src), S, HS, WS, p(tab), p(tab), p(out), OH, OW, st)
    with pytest.raises(RuntimeError, match="2\\^31"):  # (refused before any launch: 2^15 x 256 x 256 output bytes)
        _n.call("spcl_resize_nearest_pil", p(src), 1 << 15, 8, 8, p(tab), p(tab), p(out), 256, 256, st)
    assert int(out.sum()) == 0
    with pytest.raises(TypeError):
        A.resize_labels(torch.zeros(1, 8, 8, dtype=torch.int64, device="cuda"), 4)


# ---- RecipeViews with label maps under a recipe that resizes
@functools.lru_cache(maxsize=None)
def _arrays(n_scans, first=0, seed=0):
    """(stems, images u8, label maps u8) at 240^2 and the same slices resized to 224^2 by PIL on the host; computed once"""
    scans = [f"Case{k:02d}" for k in range(first, first + n_scans)]
    stems, imgs, labs = PO.prostate_arrays(scans, per_scan=2, size=240, seed=seed, classes=2)
    rimgs, rlabs = PO.pil_resized_arrays(imgs, labs, (224, 224))
    for a in (imgs, labs, rimgs, rlabs):
        a.setflags(write=False)
    return stems, imgs, labs, rimgs, rlabs


@pytest.mark.parametrize("recipe", ["prostate_pretrain", "prostate_label"])
def test_recipe_views_resize_images_and_label_maps(recipe):
    """a 240^2 store of 8-bit levels with label maps through a recipe with ``resize=224``: the image views are the bits the
    unlabelled ``RecipeViews`` gives for the same rows, image and label views are ``oracle.recipe_view`` of the slice and label
    map PIL resized (BILINEAR / NEAREST)"""
    A, _ = _mods()
    f32 = lambda i: struct.unpack("<f", struct.pack("<i", i))[0]  # noqa: E731
    f64 = lambda lo, hi: struct.unpack("<d", struct.pack("<ii", lo, hi))[0]  # noqa: E731
    _, imgs, labs, rimgs, rlabs = _arrays(3)
    images = torch.from_numpy(imgs.astype(np.float32) / np.float32(255)).cuda()
    views = A.RecipeViews(images, recipe, (224, 224), labels=torch.from_numpy(labs.copy()).cuda())
    plain = A.RecipeViews(images, recipe, (224, 224))
    assert tuple(views.images.shape) == (6, 224, 224) == tuple(views.labels.shape) and views.labels.dtype == torch.uint8
    np.testing.assert_array_equal(views.labels.cpu().numpy(), rlabs)
    np.testing.assert_array_equal(torch.round(views.images * 255).cpu().numpy().astype(np.uint8), rimgs)
    rng = random.Random(11)
    rows = views.rows([rng.randrange(6) for _ in range(6)], rng)
    img, lab = views.apply(rows, with_labels=True)
    assert torch.equal(img, plain.apply(rows)) and lab.dtype == torch.int64
    compared = 0
    for k, r in enumerate(rows):
        fl = r[1]
        ang = -np.degrees(np.arctan2(f64(r[16], r[17]), f64(r[14], r[15])))
        if O.pil_affine_q16(float(ang), 224, 224) != r[8:14]:
            continue  # (the angle recovered from the row's matrix differs from the drawn one in its last bit)
        want, wlab = O.recipe_view(rimgs[r[0]], rlabs[r[0]], (224, 224), angle=float(ang), vflip=bool(fl & 2), hflip=bool(fl & 1),
                                   top=r[2], left=r[3], pad=r[4], crop_first=bool(fl & 16), brightness=f32(r[5]),
                                   contrast=f32(r[6]), contrast_first=bool(fl & 4))
        np.testing.assert_array_equal(img[k, 0].cpu().numpy(), want.astype(np.float32) / np.float32(255), err_msg=str(r[:8]))
        np.testing.assert_array_equal(lab[k, 0].cpu().numpy(), wlab.astype(np.int64), err_msg=str(r[:8]))
        compared += 1
    assert compared >= 3, compared
    # a store already marked as resized to the recipe's size is taken as it is
    marked = A.RecipeViews(views.images, recipe, (224, 224), labels=views.labels, resized_to=224)
    assert marked.images.data_ptr() == views.images.data_ptr() and marked.labels.data_ptr() == views.labels.data_ptr()


# ---- get_data on a store the product resizes == get_data on the slices PIL resized
def _batches(loaders, seed):
    lab, unl, val, test = loaders
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    out = []
    for ld in (lab, unl):
        it = iter(ld)
        out += [next(it), next(it)]
    out += list(val)
    return out


def _assert_same_batches(a, b):
    assert len(a) == len(b) and len(a) >= 5
    for (ta, na, ma), (tb, nb, mb) in zip(a, b):
        assert na == nb and ma == mb and len(ta) == len(tb)
        for x, y in zip(ta, tb):
            assert x.dtype == y.dtype and torch.equal(x, y)


@pytest.mark.parametrize("pretrain,n_train", [(True, 8), (False, 50)])
def test_get_data_on_a_240_store_equals_get_data_on_pil_resized_slices(pretrain, n_train):
    """store A: 240^2 levels k / 255 with label maps, resized by ``create_dataset`` on the device; store B: the same slices
    resized to 224^2 by PIL on the host.  Under the same seeds both give the same first two labelled and unlabelled batches and
    the same validation batches, bit for bit (images, label maps, file names, partitions, scans)."""
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.data import creator as C
    tr, va = _arrays(n_train), _arrays(3, first=50, seed=1)
    got = {}
    for which in ("A", "B"):
        pick = (lambda t: (t[0], t[1], t[2])) if which == "A" else (lambda t: (t[0], t[3], t[4]))
        C.register_dataset("prostate", lambda mode, pick=pick: PO.prostate_store(*pick(tr if mode == "train" else va), "cuda"))
        try:
            loaders = C.get_data({"name": "prostate", "labeled_scan_num": 5}, {"batch_size": 2}, {"batch_size": 2},
                                 pretrain=pretrain)
        finally:
            C._FACTORIES.pop("prostate")
        assert all(ld.dataset.resized_to == 224 and tuple(ld.dataset.images.shape[1:]) == (224, 224) for ld in loaders)
        got[which] = _batches(loaders, seed=7)
    _assert_same_batches(got["A"], got["B"])
    (img, img2, tgt, tgt2), names, _ = got["A"][0]
    assert tuple(img.shape) == (2, 1, 224, 224) == tuple(tgt.shape) and tgt.dtype == torch.int64 and int(tgt.max()) <= 1
    if not pretrain:
        assert {n.split("_")[0] for b in got["A"][:2] for n in b[1]} <= set(C.labeled_filenames["prostate"][5])


def test_finetune_epoch_on_prostate_through_get_data(tmp_path):
    """what the issue is for: ``get_data`` on Prostate feeds ``FineTuneTrainer`` -- one epoch of two batches, finite loss,
    a Dice in [0, 1]"""
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.data import creator as C
    from spcl_amd.semi_seg.trainers import FineTuneTrainer
    tr, va = _arrays(50), _arrays(3, first=50, seed=1)
    C.register_dataset("prostate", lambda mode: PO.prostate_store(*(tr if mode == "train" else va)[:3], "cuda"))
    try:
        lab, unl, val, test = C.get_data({"name": "prostate", "labeled_scan_num": 5}, {"batch_size": 2}, {"batch_size": 2})
    finally:
        C._FACTORIES.pop("prostate")
    torch.manual_seed(0)
    random.seed(0)
    trainer = FineTuneTrainer(model=UNet(input_dim=1, num_classes=2), labeled_loader=lab, val_loader=val, test_loader=test,
                              criterion=KL_div(verbose=False), save_dir=str(tmp_path), max_epoch=1, num_batches=2,
                              device="cuda", lr=1e-4, warmup_max=1, multiplier=1)
    trainer.init()
    hist = trainer.start_training()
    assert len(hist) == 1
    assert math.isfinite(hist[0]["tra"]["semi"]["sup_loss"]["mean"])
    assert 0.0 <= hist[0]["score"] <= 1.0
    assert "DSC_mean" in hist[0]["val"]["eval"]["dice"]
