"""CPU: the host side of the Prostate data seam -- the NEAREST index table against PIL itself, ``get_data`` on a Prostate
store (train and pre-train mode), ``DeviceSliceStore.resized`` / ``resized_to`` and ``from_folder(resize=)``."""
import numpy as np
import pytest
import torch

from tests import _prostate_oracle as PO


def _A():
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.data import augment as A
    return A


def test_nearest_table_is_pils_over_the_sweep():
    """``nearest_resize_table`` == the indices ``Image.resize(NEAREST)`` itself picks on an `I`-mode ramp: n_in 1 .. 399,
    13 output lengths (5187 cases)"""
    A = _A()
    cases = bad = 0
    for n_in in PO.SWEEP_IN:
        for n_out in PO.SWEEP_OUT:
            cases += 1
            if A.nearest_resize_table(n_in, n_out) != PO.pil_nearest_table(n_in, n_out):
                bad += 1
    assert cases == 5187 and bad == 0, (cases, bad)


def test_closed_form_differs_from_pil_somewhere():
    """the trap: ``int((x + 0.5) * scale)`` is NOT PIL's rule (PIL accumulates ``xo += scale``); 256 -> 224 and 320 -> 224,
    sizes a Prostate folder may well have, are among the places where the two part"""
    A = _A()
    differing = [(i, o) for i in PO.SWEEP_IN for o in PO.SWEEP_OUT if PO.closed_form_table(i, o) != A.nearest_resize_table(i, o)]
    assert differing, "the closed form matched everywhere: the sweep no longer documents the trap"
    assert (256, 224) in differing and (320, 224) in differing
    i, o = differing[0]
    assert PO.pil_nearest_table(i, o) == A.nearest_resize_table(i, o) != PO.closed_form_table(i, o)


def test_nearest_table_reproduces_the_fixture():
    """g14 (what PIL ``pil_version`` wrote, tools/gen_golden_prostate.py): gathering by the two tables gives every resized map"""
    A = _A()
    g = PO.g14()
    assert len(g["shapes"]) >= 5
    for k, (h, w, oh, ow) in enumerate(g["shapes"].tolist()):
        lab, want = g[f"label{k}"], g[f"resized{k}"]
        assert lab.shape == (h, w) and want.shape == (oh, ow) and A.resize_shorter_edge((h, w), min(oh, ow)) == (oh, ow)
        ytab, xtab = A.nearest_resize_table(h, oh), A.nearest_resize_table(w, ow)
        np.testing.assert_array_equal(lab[np.asarray(ytab)][:, np.asarray(xtab)], want, err_msg=f"case {k} (PIL {g['pil_version']})")
        np.testing.assert_array_equal(PO.pil_resize_nearest(lab, (oh, ow)), want, err_msg=f"PIL drifted since {g['pil_version']}")


def test_nearest_table_refuses_an_index_outside_the_source(monkeypatch):
    A = _A()
    assert A.nearest_resize_table(1, 3) == [0, 0, 0] and A.nearest_resize_table(5, 1) == [2]
    # (no real pair leaves the source -- the sweep above --; the check is there for a rule someone edits)
    monkeypatch.setattr(A, "int", lambda v: 7, raising=False)
    with pytest.raises(ValueError):
        A.nearest_resize_table(4, 2)


TRAIN_SCANS = [f"Case{k:02d}" for k in range(50)]
VAL_SCANS = ["Case50", "Case51", "Case52"]


def _cpu_store(scans, size=224, per_scan=2):
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.data import ProstateSliceStore
    names = [f"{s}_{k:02d}" for s in scans for k in range(per_scan)]
    imgs = (torch.arange(len(names), dtype=torch.float32)[:, None, None] / 255.0).expand(-1, size, size)
    return ProstateSliceStore(imgs, names, targets=(torch.arange(len(names))[:, None, None] % 2).to(torch.uint8).expand(-1, size, size))


@pytest.mark.parametrize("pretrain", [False, True])
def test_get_data_returns_four_prostate_loaders(pretrain):
    """``get_data({"name": "prostate", ..})`` on 224^2 stores with label maps: four loaders (no ``NotImplementedError`` from
    the recipes' ``resize``), the published labelled scans, disjoint sets, everything marked ``resized_to``"""
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.data import creator as C
    C.register_dataset("prostate", lambda mode: _cpu_store(TRAIN_SCANS if mode == "train" else VAL_SCANS))
    try:
        loaders = C.get_data({"name": "prostate", "labeled_scan_num": 5}, {"batch_size": 2}, {"batch_size": 2}, pretrain=pretrain)
    finally:
        C._FACTORIES.pop("prostate")
    assert len(loaders) == 4
    lab, unl, val, test = loaders
    lab_scans, unl_scans = set(lab.dataset.get_scan_list()), set(unl.dataset.get_scan_list())
    assert not (lab_scans & unl_scans) and lab_scans | unl_scans == set(TRAIN_SCANS)
    if pretrain:
        assert len(lab_scans) == 25
    else:
        assert sorted(lab_scans) == sorted(C.labeled_filenames["prostate"][5])
    assert set(val.dataset.get_scan_list()) | set(test.dataset.get_scan_list()) == set(VAL_SCANS)
    assert len(val) == 1 and len(test) == 2
    for ld in loaders:
        assert ld.dataset.resized_to == 224 and tuple(ld.dataset.images.shape[1:]) == (224, 224)
        assert tuple(ld._views.images.shape[1:]) == (224, 224) and ld._views.labels.dtype == torch.uint8
    assert lab._views.recipe["resize"] == 224 and lab._views.recipe["pad"] == 20  # ProstateStrongTransforms.pretrain


def test_resized_is_idempotent_and_the_mark_survives_splits():
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.data import creator as C
    store = _cpu_store(TRAIN_SCANS[:6])
    assert store.resized_to is None
    r = store.resized(224)  # (slices already 224^2: no device call, so this runs on a CPU store)
    assert r is not store and type(r) is type(store) and r.resized_to == 224 and store.resized_to is None
    assert r.resized(224) is r
    assert torch.equal(r.images, store.images) and torch.equal(r.targets, store.targets)
    assert r.get_memory_dictionary() == store.get_memory_dictionary() and r._scan_info == store._scan_info
    sub = C.extract_sub_dataset_based_on_scan_names(r, TRAIN_SCANS[1:3])
    assert sub.resized_to == 224 and sub.resized(224) is sub
    assert all(s.resized_to == 224 for s in C.split_dataset(r, 0.5))
    assert C.extract_sub_dataset_based_on_scan_names(store, TRAIN_SCANS[1:3]).resized_to is None
    # a store that does need the kernel says so on a CPU tensor (no fallback)
    with pytest.raises(RuntimeError, match="MI355X"):
        _cpu_store(TRAIN_SCANS[:2], size=32).resized(24)


def _write_folder(root, sizes):
    from PIL import Image
    rs = np.random.RandomState(3)
    (root / "img").mkdir()
    (root / "gt").mkdir()
    for k, hw in enumerate(sizes):
        stem = f"Case{k // 3:02d}_{k % 3:02d}"
        Image.fromarray(rs.randint(0, 256, size=hw).astype(np.uint8), "L").save(root / "img" / f"{stem}.png")
        Image.fromarray(rs.randint(0, 2, size=hw).astype(np.uint8), "L").save(root / "gt" / f"{stem}.png")


def test_from_folder_resize_on_slices_that_need_none(tmp_path):
    """224^2 PNGs: ``from_folder(resize=224)`` is ``from_folder()`` (same bits, no device call) plus the mark"""
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.data import ProstateSliceStore
    _write_folder(tmp_path, [(224, 224)] * 6)
    a = ProstateSliceStore.from_folder(str(tmp_path), device="cpu")
    b = ProstateSliceStore.from_folder(str(tmp_path), device="cpu", resize=224)
    assert torch.equal(a.images, b.images) and torch.equal(a.targets, b.targets) and b.targets.dtype == torch.uint8
    assert a.get_memory_dictionary() == b.get_memory_dictionary() and a._scan_info == b._scan_info
    assert a.resized_to is None and b.resized_to == 224
    with pytest.raises(ValueError):
        ProstateSliceStore.from_folder(str(tmp_path), device="cpu", size=224, resize=224)


def test_from_folder_resize_refuses_slices_of_different_resized_shapes(tmp_path):
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.data import ProstateSliceStore
    _write_folder(tmp_path, [(224, 224), (224, 280), (224, 224)])
    with pytest.raises(ValueError, match=r"224, 280"):
        ProstateSliceStore.from_folder(str(tmp_path), device="cpu", resize=224)
