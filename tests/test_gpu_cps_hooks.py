"""GPU: the cross-pseudo-supervision hook (semi_seg/hooks/cps.py) on the tiny UNet of tests/test_gpu_semi_reg_hooks.py
(``max_channel`` 128, 2 + 2 slices of 64 x 64).

One ``SemiSupervisedEpocher.step`` returns ``peer_sup + weight * sum`` of the losses ``functional.cross_pseudo_ce`` gives on the
step's own student and peer logits (the same bits), the peer logits are the peer's own forward of the step's images, and the
meters hold what those calls' ``hist`` say.  Both networks train, the peer inside the one flat parameter.  The student's and
the peer's gradients are the float64 pull-backs of ``d sup + weight * d cross`` through identically initialised networks.
Under ``two_stage`` / ``disable_bn`` the peer's running statistics move by the labelled pass alone.  Further steps issue no
synchronising call.  Two seeded two-epoch ``SemiTrainer`` runs end bit-identical, ``last.pth`` holds the peer, a resumed
trainer has it bit for bit and its next step equals the uninterrupted one.  Without the section a ``SemiTrainer`` is what it
was."""
import io
import random

import pytest
import torch

from tests import _cps_oracle as CO
from tests.test_gpu_semi_reg_hooks import _check_step_grads, _setup, _snapshot
from tests.test_gpu_semi_step import _batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CPS = {"weight": 0.5}
BN_KEY = "_Conv1.conv.1.running_mean"


def _spy(monkeypatch):
    """record the arguments and results of the hook's own calls of ``functional.cross_pseudo_ce``"""
    from spcl_amd import functional as F_hip
    calls = []
    real = F_hip.cross_pseudo_ce

    def spy(a_logits, b_logits, tau=None, weight=1.0, out=None):
        assert a_logits.requires_grad and b_logits.requires_grad  # both networks are trained through the call
        loss = real(a_logits, b_logits, tau, weight, out=out)
        calls.append(dict(a=a_logits.detach().clone(), b=b_logits.detach().clone(), tau=tau, weight=weight,
                          loss=loss.detach().clone(), out=out))
        return loss

    monkeypatch.setattr(F_hip, "cross_pseudo_ce", spy)
    return calls, real


def _clone_net(net):
    """a network of its own with ``net``'s parameters and running statistics, in training mode and f32 like the student"""
    from spcl_amd.semi_seg.arch import UNet
    twin = UNet(input_dim=1, num_classes=4, max_channel=128)
    twin.load_state_dict({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
    twin.to(DEV).train().set_compute_dtype(torch.float32)
    return twin


def _images(ep, lab, unl, seed):
    """the three image batches of ``ep.step(lab, unl, seed)`` and the label map, on the device"""
    from spcl_amd import functional as F_hip
    flags = ep.flip_flags(seed, len(unl[0][0]))
    utf = F_hip.flip_batch(unl[0][1].to(DEV).contiguous(), flags)
    return lab[0][0].to(DEV), unl[0][0].to(DEV), utf, lab[0][2].to(DEV).squeeze(1)


def test_one_step_returns_the_peer_loss_plus_the_weighted_cross_terms(monkeypatch):
    from spcl_amd import functional as F_hip
    from spcl_amd.semi_seg.hooks import CrossPseudoTrainerHook
    sd, model, hook, ep, flat = _setup("CrossPseudoParameters", CPS)
    assert isinstance(hook, CrossPseudoTrainerHook) and hook.tau.is_cuda
    assert all(p.is_cuda for p in hook.peer.parameters())
    calls, real = _spy(monkeypatch)
    lab, unl = _batch(2, 64, 1), _batch(2, 64, 2)
    limg, uimg, utf, target = _images(ep, lab, unl, 1234)
    with torch.no_grad():  # the peer's own forward of the step's images, on a twin (the peer's statistics stay as they are)
        want_peer = _clone_net(hook.peer)(torch.cat([limg, uimg, utf], dim=0))
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(lab, unl, seed=1234)
    torch.cuda.synchronize()
    assert len(calls) == 3
    total, agree, kept = None, 0, 0
    for k, c in enumerate(calls):
        assert c["weight"] == 2 / 6 and c["tau"] is None  # plain CPS passes no thresholds
        assert c["a"].shape == c["b"].shape == (2, 4, 64, 64)
        assert torch.equal(c["b"], want_peer[2 * k:2 * k + 2])
        out = []
        again = real(c["a"], c["b"], None, c["weight"], out=out)
        assert torch.equal(again, c["loss"])
        for x, y in zip(out, c["out"]):
            assert torch.equal(x, y)
        total = again if total is None else total + again
        agree += int(out[1][16])
        kept += int(out[1][8:16].sum())
    assert not torch.equal(calls[0]["a"], calls[1]["a"]) and not torch.equal(calls[1]["a"], calls[2]["a"])
    peer_sup, _ = F_hip.sup_loss_kl_onehot(want_peer[:2], target, 1e-16)
    assert torch.equal(reg.detach(), peer_sup + 0.5 * total)
    pixels = 3 * 2 * 64 * 64
    got = ep.meters.statistics()["cps"]
    print(f"cps step: sup {float(sup):.6f}, peer sup {float(peer_sup):.6f}, cross {float(total):.6f}, agree {agree} and kept "
          f"{kept} / 2 of {pixels}")
    assert got["loss"]["mean"] == pytest.approx(float(total), rel=1e-6)
    assert got["peer_sup_loss"]["mean"] == pytest.approx(float(peer_sup), rel=1e-6)
    assert got["agree"]["mean"] == pytest.approx(agree / pixels, rel=1e-6)
    assert got["kept"]["mean"] == pytest.approx(kept / (2 * pixels), rel=1e-6) and kept == 2 * pixels
    assert 0 <= agree <= pixels and bool(torch.isfinite(reg)) and float(peer_sup) > 0.0 and float(total) > 0.0
    ep.close_hooks()


def test_both_networks_train_inside_one_flat_parameter():
    sd, model, hook, ep, flat = _setup("CrossPseudoParameters", CPS)
    peer = hook.peer
    inside = {id(p) for p in flat.params}
    assert all(id(p) in inside for p in peer.parameters()) and all(id(p) in inside for p in model.parameters())
    assert flat.numel == sum(p.numel() for p in model.parameters()) + sum(p.numel() for p in peer.parameters())
    before_m, before_p = _snapshot(model), _snapshot(peer)
    assert any(not torch.equal(before_m[k], before_p[k]) for k in before_m)
    with ep.meters.focus_on(ep.meter_focus):
        ep.step(_batch(2, 64, 1), _batch(2, 64, 2), seed=1234)
    torch.cuda.synchronize()
    after_m, after_p = _snapshot(model), _snapshot(peer)
    assert any(not torch.equal(after_m[k], before_m[k]) for k in before_m)
    assert any(not torch.equal(after_p[k], before_p[k]) for k in before_p)
    assert peer.training
    ep.close_hooks()


def _pullback(net, images, target, other, weight, student_side):
    """gradients of ``sup + weight * sum_m (2 / 6) * cross_m`` w.r.t. ``net``'s parameters: its supervised loss on the device
    and the float64 gradient of the cross terms w.r.t. its three class maps pulled back through it.  ``other``: the other
    network's f32 logits [6, 4, 64, 64] (they carry labels, no gradient)."""
    from spcl_amd import functional as F_hip
    logits = net(torch.cat(images, dim=0))
    sup, _ = F_hip.sup_loss_kl_onehot(logits[:2], target, 1e-16)
    mine = logits.detach().cpu()
    d = torch.empty_like(mine, dtype=torch.float64)
    every = torch.ones(2, 64, 64, dtype=torch.bool)
    cross = 0.0
    for k in range(3):
        x, o = mine[2 * k:2 * k + 2], other[2 * k:2 * k + 2].cpu()
        x64 = x.double().requires_grad_(True)
        yx, yo = CO.conf_and_label(x)[1], CO.conf_and_label(o)[1]
        if student_side:
            term = CO.loss(x64, o.double(), yx, yo, every, every, 2 / 6)
        else:
            term = CO.loss(o.double(), x64, yo, yx, every, every, 2 / 6)
        term.backward()
        d[2 * k:2 * k + 2] = weight * x64.grad
        cross += float(term.detach())
    params = dict(net.named_parameters())
    grads = torch.autograd.grad([sup, logits], list(params.values()), grad_outputs=[torch.ones_like(sup), d.float().to(DEV)])
    return float(sup), cross, dict(zip(params, grads))


def test_step_gradients_of_both_networks_vs_float64_pullback():
    sd, model, hook, ep, flat = _setup("CrossPseudoParameters", CPS)
    lab, unl = _batch(2, 64, 1), _batch(2, 64, 2)
    *images, target = _images(ep, lab, unl, 1234)
    student_twin, peer_twin = _clone_net(model), _clone_net(hook.peer)
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(lab, unl, seed=1234)
    torch.cuda.synchronize()
    with torch.no_grad():  # (training mode: batch statistics, the same at every pass)
        s_logits = student_twin(torch.cat(images, dim=0))
        p_logits = peer_twin(torch.cat(images, dim=0))
    osup, cross, ref = _pullback(student_twin, images, target, p_logits, 0.5, True)
    psup, cross_p, ref_p = _pullback(peer_twin, images, target, s_logits, 0.5, False)
    assert abs(float(sup) - osup) <= 1e-4 * abs(osup), (float(sup), osup)
    assert cross == pytest.approx(cross_p, rel=1e-12)
    want = psup + 0.5 * cross
    assert abs(float(reg) - want) <= 1e-4 * abs(want), (float(reg), want)
    _check_step_grads(model, flat, ref)  # d sup + weight * da, at the 5e-3 bar of the sibling hooks
    _check_step_grads(hook.peer, flat, ref_p)  # d peer_sup + weight * db
    ep.close_hooks()


def test_two_stage_with_disable_bn_moves_the_peer_statistics_by_the_labelled_pass_alone():
    sd, model, hook, ep, flat = _setup("CrossPseudoParameters", CPS)
    ep._two_stage, ep._disable_bn = True, True
    lab, unl = _batch(2, 64, 1), _batch(2, 64, 2)
    limg, uimg, utf, _ = _images(ep, lab, unl, 1234)
    start = {k: v.detach().cpu().clone() for k, v in hook.peer.state_dict().items() if "running" in k}
    labelled_only, all_three = _clone_net(hook.peer), _clone_net(hook.peer)
    with torch.no_grad():
        labelled_only(limg)
        all_three(torch.cat([limg, uimg, utf], dim=0))
    with ep.meters.focus_on(ep.meter_focus):
        ep.step(lab, unl, seed=1234)
    torch.cuda.synchronize()
    ref = {k: v.cpu() for k, v in labelled_only.state_dict().items() if "running" in k}
    for k, v in hook.peer.state_dict().items():  # every BatchNorm of the peer, not the first alone
        if "running" in k:
            assert torch.allclose(v.cpu(), ref[k], rtol=1e-4, atol=1e-6), k
    got = hook.peer.state_dict()[BN_KEY].cpu()
    assert not torch.equal(got, start[BN_KEY])
    assert not torch.allclose(got, all_three.state_dict()[BN_KEY].cpu(), rtol=1e-4, atol=1e-6)
    # the model's own: by its labelled pass alone too (what the epocher did before the hook existed)
    from tests.test_gpu_semi_step import UNetStats
    assert torch.allclose(model.state_dict()[BN_KEY].cpu(), UNetStats.after_labelled_pass(sd, lab), rtol=1e-4, atol=1e-6)
    ep.close_hooks()


@pytest.mark.parametrize("params", [CPS, {"weight": 0.5, "threshold": [0.2, 0.3, 0.3, 0.3], "on": ["unlabeled", "unlabeled_tf"]}])
def test_further_steps_issue_no_host_synchronisation(params):
    sd, model, hook, ep, flat = _setup("CrossPseudoParameters", params)
    with ep.meters.focus_on(ep.meter_focus):
        ep.step(_batch(2, 64, 1), _batch(2, 64, 2), seed=1)
        torch.cuda.synchronize()
        batches = [(_batch(2, 64, 10 + k), _batch(2, 64, 20 + k)) for k in range(2)]
        moved = [tuple(((tuple(t.pin_memory() for t in b[0]),) + b[1:]) for b in pair) for pair in batches]
        for k, (lab, unl) in enumerate(moved):
            torch.cuda.set_sync_debug_mode("error")
            try:
                ep.step(lab, unl, seed=2 + k)
            finally:
                torch.cuda.set_sync_debug_mode(0)
            torch.cuda.synchronize()
    got = ep.meters.statistics()["cps"]
    assert 0.0 <= got["agree"]["mean"] <= 1.0 and 0.0 < got["kept"]["mean"] <= 1.0  # (class 0 clears its 0.2 always)
    ep.close_hooks()


def test_thresholds_and_on_reach_the_calls(monkeypatch):
    params = {"weight": 0.5, "threshold": [0.2, 0.3, 0.3, 0.3], "on": ["unlabeled_tf", "labeled"]}
    sd, model, hook, ep, flat = _setup("CrossPseudoParameters", params)
    calls, _ = _spy(monkeypatch)
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(_batch(2, 64, 1), _batch(2, 64, 2), seed=1234)
    torch.cuda.synchronize()
    assert len(calls) == 2 and all(c["weight"] == 2 / 4 and c["tau"] is hook.tau for c in calls)
    assert torch.equal(hook.tau.cpu(), torch.tensor([0.2, 0.3, 0.3, 0.3]))
    kept = sum(int(c["out"][1][8:16].sum()) for c in calls)
    assert ep.meters.statistics()["cps"]["kept"]["mean"] == pytest.approx(kept / (2 * 2 * 2 * 64 * 64), rel=1e-6)
    ep.close_hooks()


def test_under_the_real_mixup_epocher_the_call_says_what_is_missing():
    """``MixUpEpocher.step`` hands its hooks the labelled pair and ``label_logits`` only: a RuntimeError that names the
    epocher, not a TypeError about a keyword"""
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.epochers.mixup import MixUpEpocher
    sd, model, hook, _, _ = _setup("CrossPseudoParameters", CPS)
    ep = MixUpEpocher(model=model, optimizer=torch.optim.SGD(model.parameters(), lr=0.0), labeled_loader=[],
                      unlabeled_loader=None, sup_criterion=KL_div(), num_batches=1, device=DEV)
    ep.add_hooks([hook()])
    ep.init()
    with pytest.raises(RuntimeError, match="MixUpEpocher.*image batches"):
        with ep.meters.focus_on(ep.meter_focus):
            ep.step(_batch(2, 64, 1), seed=7)
    torch.cuda.synchronize()
    ep.close_hooks()


# ------------------------------------------------------------------------------------------------------------ trainer
def _trainer(cfg, save_dir=None, seed=3):
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.trainers.semi import SemiTrainer
    torch.manual_seed(seed)
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    lab = [_batch(2, 64, 30 + k) for k in range(3)]
    unl = [_batch(2, 64, 40 + k) for k in range(3)]
    val = [((b[0][0], b[0][2]), b[1], b[2]) for b in lab]
    tr = SemiTrainer(model=model, labeled_loader=lab, unlabeled_loader=unl, val_loader=val, test_loader=None,
                     criterion=KL_div(), save_dir=save_dir, max_epoch=2, num_batches=3, device=DEV, two_stage=True,
                     disable_bn=True, config=cfg)
    tr.register_hooks(*create_hook_from_config(model, cfg))
    tr.init()
    return tr, model, lab, unl


def _cfg(**sections):
    return dict({"Optim": {"name": "RAdam", "lr": 1e-3, "weight_decay": 1e-5}, "Data": {"name": "acdc"},
                 "Trainer": {"max_epoch": 2}}, **sections)


def _state(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def test_two_seeded_trainer_runs_are_identical_and_the_checkpoint_holds_the_peer(tmp_path):
    ends = []
    for run in range(2):
        tr, model, _, _ = _trainer(_cfg(CrossPseudoParameters=CPS), save_dir=str(tmp_path) if run == 0 else None)
        random.seed(7)
        hist = tr.start_training()
        torch.cuda.synchronize()
        assert len(hist) == 2 and "cps" in str(hist[-1]["tra"])
        for name in ("loss", "peer_sup_loss", "agree", "kept"):
            assert name in str(hist[-1]["tra"]), name
        ends.append((_state(model), _state(tr.__hooks__[0].peer)))
    (ma, pa), (mb, pb) = ends
    assert all(torch.equal(ma[k], mb[k]) for k in ma) and all(torch.equal(pa[k], pb[k]) for k in pa)
    assert any(not torch.equal(ma[k], pa[k]) for k in ma if "running" not in k and "num_batches" not in k)
    saved = torch.load(tmp_path / "last.pth", map_location="cpu")
    assert sorted(k for k in saved["__hooks__"] if k != "0.tau") == sorted("0._peer." + k for k in ma)
    assert all(torch.equal(saved["__hooks__"]["0._peer." + k], pa[k]) for k in pa)
    # a resumed trainer (other initial weights, another peer seed) has the trained peer bit for bit
    tr2, model2, _, _ = _trainer(_cfg(CrossPseudoParameters=dict(CPS, peer_seed=5)), seed=4)
    assert any(not torch.equal(v, pa[k]) for k, v in _state(tr2.__hooks__[0].peer).items())
    tr2.resume_from_path(str(tmp_path / "last.pth"))
    got = _state(tr2.__hooks__[0].peer)
    assert all(torch.equal(got[k], pa[k]) for k in pa)
    assert all(p.is_cuda for p in tr2.__hooks__[0].peer.parameters())


def test_trainer_round_trip_restores_the_peer_and_the_next_step():
    tr, model, lab, unl = _trainer(_cfg(CrossPseudoParameters=CPS))
    hook = tr.__hooks__[0]
    ep = tr._create_tra_epoch()
    with ep.meters.focus_on(ep.meter_focus):
        for k in range(2):
            ep.step(lab[k], unl[k], seed=100 + k)
        torch.cuda.synchronize()
        blob = io.BytesIO()
        torch.save(tr.state_dict(), blob)
        peer2 = _state(hook.peer)
        ep.step(lab[2], unl[2], seed=102)
    torch.cuda.synchronize()
    ep.close_hooks()
    want_m, want_p = _state(model), _state(hook.peer)
    assert any(not torch.equal(want_p[k], peer2[k]) for k in peer2)

    blob.seek(0)
    saved = torch.load(blob, map_location="cpu")
    tr2, model2, _, _ = _trainer(_cfg(CrossPseudoParameters=dict(CPS, peer_seed=5)), seed=4)  # (other initial weights)
    tr2.load_state_dict(saved)
    hook2 = tr2.__hooks__[0]
    got = _state(hook2.peer)
    assert all(torch.equal(got[k], peer2[k]) for k in peer2)
    ep2 = tr2._create_tra_epoch()
    with ep2.meters.focus_on(ep2.meter_focus):
        ep2.step(lab[2], unl[2], seed=102)
    torch.cuda.synchronize()
    ep2.close_hooks()
    got_m, got_p = _state(model2), _state(hook2.peer)
    assert all(torch.equal(got_m[k], want_m[k]) for k in want_m)
    assert all(torch.equal(got_p[k], want_p[k]) for k in want_p)


def test_without_the_section_the_trainer_is_what_it_was():
    from spcl_amd.semi_seg.hooks import CrossPseudoTrainerHook
    none, model, _, _ = _trainer(_cfg())
    with_cps, model_c, _, _ = _trainer(_cfg(CrossPseudoParameters=CPS))
    assert [type(h) for h in none.__hooks__] == []
    assert [type(h) for h in with_cps.__hooks__] == [CrossPseudoTrainerHook]
    n_model = sum(p.numel() for p in model.parameters())
    assert none._flat.numel == n_model and with_cps._flat.numel == 2 * n_model
    assert none.__hooks__.state_dict() == {}

    def meter_names(tr):
        ep = tr._create_tra_epoch()
        names = {g: sorted(ms) for g, ms in ep.meters._groups.items()}
        ep.close_hooks()
        return names

    base = meter_names(none)
    assert sorted(base) == ["semi"] and base["semi"] == ["lr", "reg_loss", "sup_dice", "sup_loss"]
    assert meter_names(with_cps) == dict(base, cps=["agree", "kept", "loss", "peer_sup_loss"])
