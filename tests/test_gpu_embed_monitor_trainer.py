"""The pre-training monitor through the trainer: ``PretrainEncoderTrainer(monitor=...)`` on the synthetic ACDC-like store.
The monitor must be invisible to training (same losses, same parameters, bit for bit), deterministic on an unchanged model,
sensitive to a trained one, and must call a dead encoder dead."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCANS = 6


def _trainer(save_dir, monitor, max_epoch=3, seed=5, init=True):
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.data.dataset import synthetic_slice_store
    from spcl_amd.semi_seg.data.loader import ContrastiveDeviceLoader
    from spcl_amd.semi_seg.data.rearr import ContrastBatchSampler
    from spcl_amd.semi_seg.hooks import create_sp_infonce_hooks
    from spcl_amd.semi_seg.trainers import PretrainEncoderTrainer
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    net = UNet(input_dim=1, num_classes=4, max_channel=128).cuda()
    store = synthetic_slice_store(scans=SCANS, slices_per_scan=(8, 11), size=48, device="cuda", seed=2)
    loader = ContrastiveDeviceLoader(store, batch_sampler=ContrastBatchSampler(store, scan_sample_num=3,
                                                                                partition_sample_num=1), out_hw=(32, 32))
    with net.set_grad(False, start="Conv5", include_start=False):
        tr = PretrainEncoderTrainer(model=net, chain_dataloader=loader, max_epoch=max_epoch, num_batches=4, device="cuda",
                                    lr=1e-3, save_dir=str(save_dir), monitor=monitor)
        tr.register_hooks(create_sp_infonce_hooks(model=net, feature_names="Conv5", weights=1.0, contrast_ons="partition",
                                                  begin_values=5.0, end_values=50.0, mode="soft", max_epoch=max_epoch, p=0.5,
                                                  correct_grad=True, data_name="acdc", sync_checks=False))
        tr.forward_until = "Conv5"
        if init:
            tr.init()
    return tr, net, store


def _trainer_uninitialised(save_dir, monitor):
    return _trainer(save_dir, monitor, init=False)


def _train(tr, net):
    with net.set_grad(False, start="Conv5", include_start=False):
        return tr.start_training()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """two epochs without and with the monitor, from the same seeds"""
    plain_dir, mon_dir = tmp_path_factory.mktemp("plain"), tmp_path_factory.mktemp("monitored")
    tr0, net0, _ = _trainer(plain_dir, None)
    h0 = _train(tr0, net0)
    tr1, net1, _ = _trainer(mon_dir, {"k": 5, "max_slices": 24})
    h1 = _train(tr1, net1)
    torch.cuda.synchronize()
    return dict(plain=(tr0, net0, h0, plain_dir), monitored=(tr1, net1, h1, mon_dir))


def test_training_is_bit_identical_with_and_without_the_monitor(runs):
    (_, net0, h0, _), (_, net1, h1, _) = runs["plain"], runs["monitored"]
    assert len(h0) == len(h1) == 2
    for a, b in zip(h0, h1):
        assert "monitor" not in a and "monitor" in b
        assert a == {k: v for k, v in b.items() if k != "monitor"}
        assert np.isfinite(a["semi"]["reg_loss"]["mean"])
    for (n0, p0), (n1, p1) in zip(net0.state_dict().items(), net1.state_dict().items()):
        assert n0 == n1 and torch.equal(p0, p1), n0


def test_history_keys_best_checkpoint_and_buffers(runs):
    (tr0, _, _, plain_dir), (tr1, _, h1, mon_dir) = runs["plain"], runs["monitored"]
    assert os.path.exists(os.path.join(plain_dir, "last.pth")) and not os.path.exists(os.path.join(plain_dir, "best.pth"))
    assert os.path.exists(os.path.join(mon_dir, "last.pth")) and os.path.exists(os.path.join(mon_dir, "best.pth"))
    assert set(tr0.state_dict()["_buffers"]) == {"_cur_epoch", "_start_epoch", "_best_score"} and tr0._best_score == 0
    m = h1[-1]["monitor"]
    for key in ("knn_partition", "knn_patient", "knn_cycle", "top1", "recall5", "align", "uniform", "min_norm"):
        for space in ("feature", "projection"):
            assert np.isfinite(m[f"conv5/{space}/{key}"]), (space, key)
    for key, v in m.items():
        if key.rsplit("/", 1)[-1].startswith(("knn_", "top1", "recall5")):
            assert 0.0 <= v <= 1.0, (key, v)
    assert m["skipped"] == [] and m["conv5/feature/min_norm"] > 0
    assert m["conv5/projection/recall5"] >= m["conv5/projection/top1"]
    scores = [h["monitor"]["conv5/projection/knn_patient"] for h in h1]
    assert tr1._best_score == max(scores) and tr1._best_epoch == 1 + scores.index(max(scores))
    buffers = tr1.state_dict()["_buffers"]
    assert buffers["_monitor_indices"] == tr1._monitor.indices and len(buffers["_monitor_indices"]) == 24
    best = torch.load(os.path.join(mon_dir, "best.pth"), map_location="cpu")
    assert best["_buffers"]["_best_score"] == tr1._best_score and best["_buffers"]["_cur_epoch"] == tr1._best_epoch


def test_resumed_trainer_keeps_the_score_and_the_slice_set(runs, tmp_path):
    tr1, _, _, mon_dir = runs["monitored"]
    tr2, _, store = _trainer(tmp_path, {"k": 5, "max_slices": 16}, seed=9)
    assert len(tr2._monitor.indices) == 16
    tr2.resume_from_path(os.path.join(mon_dir, "last.pth"))
    assert tr2._best_score == tr1._best_score and tr2._best_epoch == tr1._best_epoch
    assert tr2._monitor.indices == tr1._monitor.indices and tr2._monitor.images.shape[0] == 48
    assert torch.equal(tr2._monitor.images, tr1._monitor.images)


def test_run_is_deterministic_and_follows_the_model(tmp_path):
    tr, net, _ = _trainer(tmp_path, {"k": 5, "max_slices": 24}, max_epoch=2)
    state = random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state()
    stats = {k: v.clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}
    a = tr._monitor.run(net, tr.__hooks__)
    b = tr._monitor.run(net, tr.__hooks__)
    assert a == b and net.training
    assert random.getstate() == state[0] and torch.equal(torch.get_rng_state(), state[2])
    assert torch.equal(torch.cuda.get_rng_state(), state[3])
    assert all(np.array_equal(x, y) for x, y in zip(np.random.get_state()[1:2], state[1][1:2]))
    for k, v in stats.items():
        assert torch.equal(net.state_dict()[k], v), k
    hist = _train(tr, net)
    c = hist[-1]["monitor"]
    assert set(c) == set(a) and c != a


def test_dead_encoder_is_reported(tmp_path):
    tr, net, _ = _trainer(tmp_path, {"k": 5, "max_slices": 24}, max_epoch=2)
    with torch.no_grad():
        for p in net._Conv5.parameters():
            p.zero_()
    m = tr._monitor.run(net, tr.__hooks__)
    assert m["conv5/feature/min_norm"] == 0.0
    # every similarity is equal: the neighbours are the lowest indices, every row gets the same vote -- one patient's share
    for space in ("feature", "projection"):
        assert m[f"conv5/{space}/knn_patient"] <= 2.0 / SCANS, m
        assert m[f"conv5/{space}/top1"] <= 0.1, m


def test_a_loader_without_a_store_is_refused(tmp_path):
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.trainers import PretrainEncoderTrainer
    from spcl_amd.synthetic import SyntheticPretrainLoader
    net = UNet(input_dim=1, num_classes=4, max_channel=128).cuda()
    loader = SyntheticPretrainLoader(bs=9, size=32, device="cuda", seed=3, resident=True, pool=3)
    tr = PretrainEncoderTrainer(model=net, chain_dataloader=loader, max_epoch=2, num_batches=2, device="cuda", lr=1e-3,
                                save_dir=str(tmp_path), monitor={"k": 5})
    with pytest.raises(TypeError, match="DeviceSliceStore"):
        tr.init()


# ---- decoder pre-training: its hooks are dense, the monitor has nothing to score and must not get in the way
def _decoder_trainer(save_dir, monitor, feature_names, max_epoch=2, seed=7):
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.data.dataset import synthetic_slice_store
    from spcl_amd.semi_seg.data.loader import ContrastiveDeviceLoader
    from spcl_amd.semi_seg.data.rearr import ContrastBatchSampler
    from spcl_amd.semi_seg.hooks import create_infonce_hooks
    from spcl_amd.semi_seg.trainers import PretrainDecoderTrainer
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    net = UNet(input_dim=1, num_classes=4, max_channel=128).cuda()
    store = synthetic_slice_store(scans=SCANS, slices_per_scan=(8, 11), size=72, device="cuda", seed=2)
    loader = ContrastiveDeviceLoader(store, batch_sampler=ContrastBatchSampler(store, scan_sample_num=3,
                                                                                partition_sample_num=1), out_hw=(64, 64))
    for p in net.parameters():  # main_pretrain_decoder.py:66-69: the encoder frozen, the decoder up to the tapped block trains
        p.requires_grad_(False)
    for name in ("Up5", "Up_conv5", "Up4", "Up_conv4", "Up3", "Up_conv3"):
        getattr(net, "_" + name).requires_grad_(True)
    tr = PretrainDecoderTrainer(model=net, chain_dataloader=loader, max_epoch=max_epoch, num_batches=3, device="cuda", lr=1e-3,
                                save_dir=str(save_dir), monitor=monitor)
    tr.register_hooks(create_infonce_hooks(model=net, feature_names=feature_names, weights=0.5, contrast_ons="partition",
                                           data_name="acdc", sync_checks=False))
    tr.forward_until = "Up_conv3"
    return tr


def test_decoder_trainer_with_dense_hooks_only_records_what_it_skipped(tmp_path):
    tr = _decoder_trainer(tmp_path, {"k": 5, "max_slices": 16}, ["Up_conv3"])
    with pytest.warns(UserWarning, match="nothing to score"):
        tr.init()
    assert tr._monitor_key is None
    hist = tr.start_training()
    assert len(hist) == 1 and hist[0]["monitor"] == {"skipped": ["infonce_up_conv3_partition"]}
    assert np.isfinite(hist[0]["semi"]["reg_loss"]["mean"])
    assert os.path.exists(os.path.join(tmp_path, "last.pth")) and not os.path.exists(os.path.join(tmp_path, "best.pth"))
    assert tr._best_score == 0 and tr._best_epoch is None
    assert torch.load(os.path.join(tmp_path, "last.pth"), map_location="cpu")["_buffers"]["_cur_epoch"] == 1


def test_decoder_trainer_refuses_a_key_it_cannot_report_before_training(tmp_path):
    tr = _decoder_trainer(tmp_path, {"k": 5, "max_slices": 16, "select_by": "conv5/projection/knn_patient"}, ["Up_conv3"])
    with pytest.raises(ValueError, match="select_by"):
        tr.init()
    assert tr.history == [] and not os.path.exists(os.path.join(tmp_path, "last.pth"))


def test_decoder_trainer_scores_the_encoder_hook_beside_a_dense_one(tmp_path):
    tr = _decoder_trainer(tmp_path, {"k": 5, "max_slices": 16}, ["Conv5", "Up_conv3"])
    tr.init()
    assert tr._monitor_key == "conv5/projection/knn_patient"
    hist = tr.start_training()
    m = hist[0]["monitor"]
    assert m["skipped"] == ["infonce_up_conv3_partition"] and set(m) - {"skipped"} == set(tr._monitor.expected_keys(tr._model, tr.__hooks__))
    assert tr._best_score == m["conv5/projection/knn_patient"] and tr._best_epoch == 1
    assert os.path.exists(os.path.join(tmp_path, "best.pth"))


def test_last_checkpoint_is_written_even_when_the_monitor_fails(tmp_path):
    tr, net, _ = _trainer(tmp_path, {"k": 5, "max_slices": 24}, max_epoch=2)

    def broken(model, hooks):
        raise RuntimeError("monitor failed")
    tr._monitor.run = broken
    with pytest.raises(RuntimeError, match="monitor failed"):
        _train(tr, net)
    saved = torch.load(os.path.join(tmp_path, "last.pth"), map_location="cpu")
    assert saved["_buffers"]["_cur_epoch"] == 1 and not os.path.exists(os.path.join(tmp_path, "best.pth"))


def test_unknown_select_by_is_refused_at_init(tmp_path):
    tr, _, _ = _trainer_uninitialised(tmp_path, {"k": 5, "select_by": "conv4/projection/knn_patient"})
    with pytest.raises(ValueError, match="select_by"):
        tr.init()


# ---- construction
def test_construction_leaves_every_random_stream_alone_and_takes_the_loaders_size():
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.data.creator import UnlabeledDeviceLoader
    from spcl_amd.semi_seg.data.dataset import synthetic_slice_store
    from spcl_amd.semi_seg.data.loader import ContrastiveDeviceLoader
    from spcl_amd.semi_seg.data.rearr import ContrastBatchSampler
    from spcl_amd.semi_seg.epochers import EmbeddingMonitor
    store = synthetic_slice_store(scans=SCANS, slices_per_scan=(8, 11), size=48, device="cuda", seed=2)
    sampler = ContrastBatchSampler(store, scan_sample_num=3, partition_sample_num=1)
    loaders = [ContrastiveDeviceLoader(store, batch_sampler=sampler, out_hw=(32, 32)),
               ContrastiveDeviceLoader(store, batch_sampler=sampler, out_hw=(32, 32), degrees=45.0),  # the legacy views
               UnlabeledDeviceLoader(store, batch_size=4, out_hw=(32, 32))]  # (no views before its first batch)
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    state = random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state()
    monitors = [EmbeddingMonitor(loader, max_slices=16, k=5) for loader in loaders]
    after = random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state()
    assert after[0] == state[0] and torch.equal(after[2], state[2]) and torch.equal(after[3], state[3])
    assert after[1][0] == state[1][0] and np.array_equal(after[1][1], state[1][1]) and after[1][2:] == state[1][2:]
    for m in monitors:
        assert tuple(m.images.shape) == (32, 1, 32, 32)
    assert torch.equal(monitors[0].images, monitors[2].images)  # the same recipe, the same private draw
    assert tuple(EmbeddingMonitor(store, max_slices=16, k=5, out_hw=(40, 40)).images.shape) == (32, 1, 40, 40)
