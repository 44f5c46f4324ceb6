"""The dense pre-training monitor through the trainer: ``PretrainDecoderTrainer(dense_monitor=...)`` on the synthetic
ACDC-like store with label maps, one dense hook on ``Up_conv3``.  It must report exactly the keys it promises, select a
``best.pth``, stay invisible to training (same losses, same parameters, bit for bit) and to the encoder monitor beside it, and
keep its slice set through a resume."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCANS = 6
DENSE = {"k": 5, "max_slices": 16}


def _store(targets=True):
    from spcl_amd.semi_seg.data.dataset import synthetic_slice_store
    store = synthetic_slice_store(scans=SCANS, slices_per_scan=(8, 11), size=72, device="cuda", seed=2)
    if targets:  # four classes by intensity: the blobs' cores, rims and the background
        store.targets = (store.images * 4.0).clamp_(0, 3).to(torch.uint8)
    return store


def _trainer(save_dir, feature_names=("Up_conv3",), store=None, max_epoch=3, seed=7, **kwargs):
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.data.loader import ContrastiveDeviceLoader
    from spcl_amd.semi_seg.data.rearr import ContrastBatchSampler
    from spcl_amd.semi_seg.hooks import create_infonce_hooks
    from spcl_amd.semi_seg.trainers import PretrainDecoderTrainer
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    net = UNet(input_dim=1, num_classes=4, max_channel=128).cuda()
    store = store if store is not None else _store()
    loader = ContrastiveDeviceLoader(store, batch_sampler=ContrastBatchSampler(store, scan_sample_num=3,
                                                                                partition_sample_num=1), out_hw=(64, 64))
    for p in net.parameters():  # main_pretrain_decoder.py:66-69: the encoder frozen, the decoder up to the tapped block trains
        p.requires_grad_(False)
    for name in ("Up5", "Up_conv5", "Up4", "Up_conv4", "Up3", "Up_conv3"):
        getattr(net, "_" + name).requires_grad_(True)
    tr = PretrainDecoderTrainer(model=net, chain_dataloader=loader, max_epoch=max_epoch, num_batches=3, device="cuda", lr=1e-3,
                                save_dir=str(save_dir), **kwargs)
    tr.register_hooks(create_infonce_hooks(model=net, feature_names=list(feature_names), weights=0.5,
                                           contrast_ons="partition", data_name="acdc", sync_checks=False))
    tr.forward_until = "Up_conv3"
    return tr, net


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """two epochs from the same seeds: without either monitor, with the dense one, with the encoder monitor, with both"""
    import warnings
    out = {}
    for name, kwargs in (("plain", {}), ("dense", {"dense_monitor": DENSE}), ("monitor", {"monitor": {"k": 5, "max_slices": 16}}),
                         ("both", {"monitor": {"k": 5, "max_slices": 16}, "dense_monitor": DENSE})):
        save_dir = tmp_path_factory.mktemp(name)
        tr, net = _trainer(save_dir, **kwargs)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)  # (the encoder monitor says once that it has nothing to score)
            tr.init()
        out[name] = (tr, net, tr.start_training(), save_dir)
    torch.cuda.synchronize()
    return out


def test_history_holds_the_expected_keys_and_best_checkpoint_follows_the_selected_one(runs):
    tr, _, hist, save_dir = runs["dense"]
    assert len(hist) == 2 and tr._dense_key == "up_conv3/dense_projection/knn_dice"
    keys = tr._dense_monitor.expected_keys(tr._model, tr.__hooks__)
    assert len(keys) == 8 and tr._dense_key in keys
    for h in hist:
        m = h["dense_monitor"]
        assert set(m) == set(keys) | {"skipped"} and m["skipped"] == []
        for key, v in m.items():
            if key.endswith(("/knn_class", "/knn_dice")):
                assert 0.0 <= v <= 1.0, (key, v)
            elif key != "skipped":
                assert np.isfinite(v), (key, v)
        assert m["up_conv3/dense_feature/min_norm"] >= 0 and m["up_conv3/dense_projection/uniform"] <= 0
    scores = [h["dense_monitor"][tr._dense_key] for h in hist]
    assert tr._best_score == max(scores) and tr._best_epoch == 1 + scores.index(max(scores))
    assert os.path.exists(os.path.join(save_dir, "last.pth")) and os.path.exists(os.path.join(save_dir, "best.pth"))
    best = torch.load(os.path.join(save_dir, "best.pth"), map_location="cpu")["_buffers"]
    assert best["_best_score"] == tr._best_score and best["_cur_epoch"] == tr._best_epoch
    assert best["_dense_monitor_indices"] == tr._dense_monitor.indices and len(tr._dense_monitor.indices) == 16
    # the rows: 16 slices of 10 x 10 cells, labelled by the majority of their window, grouped by scan
    labels, groups = tr._dense_monitor.cells((10, 10))
    assert labels.shape == groups.shape == (1600,) and int(labels.min()) >= 0 and int(labels.max()) <= 3
    assert len(torch.unique(labels)) > 1 and len(torch.unique(groups)) == SCANS
    assert torch.equal(groups.view(16, 100)[:, 0], groups.view(16, 100)[:, 99])


def test_training_is_bit_identical_with_and_without_the_dense_monitor(runs):
    (tr0, net0, h0, plain_dir), (_, net1, h1, _) = runs["plain"], runs["dense"]
    assert len(h0) == len(h1) == 2
    for a, b in zip(h0, h1):
        assert "dense_monitor" not in a and "dense_monitor" in b
        assert a == {k: v for k, v in b.items() if k != "dense_monitor"}
        assert np.isfinite(a["semi"]["reg_loss"]["mean"])
    for (n0, p0), (n1, p1) in zip(net0.state_dict().items(), net1.state_dict().items()):
        assert n0 == n1 and torch.equal(p0, p1), n0
    # opt-in: without the argument the files and the checkpoint's buffers are what they were
    assert not os.path.exists(os.path.join(plain_dir, "best.pth"))
    assert set(tr0.state_dict()["_buffers"]) == {"_cur_epoch", "_start_epoch", "_best_score"} and tr0._best_score == 0


def test_the_encoder_monitor_beside_it_reports_what_it_reported_alone(runs):
    (tr1, _, h1, _), (tr2, net2, h2, _) = runs["monitor"], runs["both"]
    assert tr2._monitor_key is None and tr2._dense_key == "up_conv3/dense_projection/knn_dice"
    for a, b in zip(h1, h2):
        assert a["monitor"] == b["monitor"] == {"skipped": ["infonce_up_conv3_partition"]}
        assert a == {k: v for k, v in b.items() if k != "dense_monitor"}
    assert [h["dense_monitor"] for h in h2] == [h["dense_monitor"] for h in runs["dense"][2]]
    assert tr1._best_epoch is None and tr2._best_epoch is not None
    for (n0, p0), (n1, p1) in zip(runs["plain"][1].state_dict().items(), net2.state_dict().items()):
        assert torch.equal(p0, p1), n0


def test_run_is_deterministic_and_leaves_modes_statistics_and_random_streams_alone(tmp_path):
    tr, net = _trainer(tmp_path, dense_monitor=DENSE, max_epoch=2)
    tr.init()
    net.train()
    state = random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state()
    stats = {k: v.clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}
    a = tr._dense_monitor.run(net, tr.__hooks__)
    b = tr._dense_monitor.run(net, tr.__hooks__)
    assert a == b and net.training and all(p.training for h in tr.__hooks__ for p in h.modules())
    assert random.getstate() == state[0] and torch.equal(torch.get_rng_state(), state[2])
    assert torch.equal(torch.cuda.get_rng_state(), state[3])
    assert all(np.array_equal(x, y) for x, y in zip(np.random.get_state()[1:2], state[1][1:2]))
    for k, v in stats.items():
        assert torch.equal(net.state_dict()[k], v), k
    # leaving the slice out instead of the scan lets the neighbouring slices vote: another number
    tr2, net2 = _trainer(tmp_path, dense_monitor=dict(DENSE, exclude="slice"), max_epoch=2)
    tr2.init()
    c = tr2._dense_monitor.run(net2, tr2.__hooks__)
    assert set(c) == set(a) and c["up_conv3/dense_feature/min_norm"] == a["up_conv3/dense_feature/min_norm"]
    assert c["up_conv3/dense_feature/knn_class"] != a["up_conv3/dense_feature/knn_class"]


def test_resumed_trainer_keeps_the_score_and_the_slice_set(runs, tmp_path):
    tr1, _, _, save_dir = runs["dense"]
    tr2, _ = _trainer(tmp_path, dense_monitor={"k": 5, "max_slices": 8}, seed=9)
    tr2.init()
    assert len(tr2._dense_monitor.indices) == 8
    tr2.resume_from_path(os.path.join(save_dir, "last.pth"))
    assert tr2._best_score == tr1._best_score and tr2._best_epoch == tr1._best_epoch
    assert tr2._dense_monitor.indices == tr1._dense_monitor.indices and tr2._dense_monitor.images.shape[0] == 16
    assert torch.equal(tr2._dense_monitor.images, tr1._dense_monitor.images)
    assert torch.equal(tr2._dense_monitor.targets, tr1._dense_monitor.targets)


def test_a_store_without_label_maps_and_encoder_hooks_only_are_refused_in_init(tmp_path):
    tr, _ = _trainer(tmp_path, store=_store(targets=False), dense_monitor=DENSE)
    with pytest.raises(ValueError, match="no label maps"):
        tr.init()
    tr, _ = _trainer(tmp_path, feature_names=("Conv5",), dense_monitor=DENSE)
    with pytest.raises(ValueError, match="no contrastive hook taps a decoder feature"):
        tr.init()
    assert tr.history == [] and not os.path.exists(os.path.join(tmp_path, "last.pth"))


def test_select_by_false_records_without_selecting(tmp_path):
    tr, _ = _trainer(tmp_path, dense_monitor=dict(DENSE, select_by=False), max_epoch=2)
    tr.init()
    hist = tr.start_training()
    assert len(hist) == 1 and "up_conv3/dense_projection/knn_dice" in hist[0]["dense_monitor"]
    assert tr._dense_key is None and tr._best_score == 0 and tr._best_epoch is None
    assert os.path.exists(os.path.join(tmp_path, "last.pth")) and not os.path.exists(os.path.join(tmp_path, "best.pth"))
