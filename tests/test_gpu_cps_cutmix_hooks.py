"""GPU: the CutMix term of the cross-pseudo-supervision hook (semi_seg/hooks/cps.py, ``"cutmix"`` in ``on``) on the tiny UNet of
tests/test_gpu_cps_hooks.py (``max_channel`` 128, 2 + 2 slices of 64 x 64).

One ``SemiSupervisedEpocher.step`` returns ``peer_sup + weight *`` the weighted terms; the spied calls carry ``n_seg / n_total``,
the boxes of ``draw``, the mixed batch and teachers without gradient; ``draw`` advances by one per step.  With ``on: [cutmix]``
``cross_pseudo_ce`` is never called.  The step gradients of both networks are the float64 pull-backs through identically
initialised networks, the path through the mixed forward included.  Under ``two_stage`` / ``disable_bn`` both networks'
running statistics move by the labelled pass alone.  Further steps issue no synchronising call.  Two seeded trainer runs end
bit-identical; a checkpoint round trip restores ``draw`` and reproduces the next step bit for bit.  One unlabelled slice is a
RuntimeError.  Without ``"cutmix"`` none of the three new functionals is called and state-dict keys and meters are what they
were."""
import io
import random

import pytest
import torch

from tests import _cps_oracle as CO
from tests import _cutmix_oracle as O
from tests.test_gpu_cps_hooks import BN_KEY, _cfg, _clone_net, _images, _state, _trainer
from tests.test_gpu_semi_reg_hooks import _check_step_grads, _setup
from tests.test_gpu_semi_step import _batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = {"weight": 0.5, "on": ["labeled", "unlabeled", "unlabeled_tf", "cutmix"], "cutmix": {"prop_range": [0.25, 0.5], "seed": 23}}
ONLY = {"weight": 0.5, "on": ["cutmix"], "cutmix": {"seed": 23}}
NEW = ("cutmix_boxes", "cutmix_images", "cross_pseudo_ce_mixed")


def _spy(monkeypatch):
    """record the hook's own calls of the four functionals; -> (calls by name, the real functions)"""
    from spcl_amd import functional as F_hip
    calls = {name: [] for name in NEW + ("cross_pseudo_ce",)}
    real = {name: getattr(F_hip, name) for name in calls}

    def boxes(seed, N, H, W, prop_range=(0.25, 0.5), device=None):
        word = seed.clone() if isinstance(seed, torch.Tensor) else seed
        got = real["cutmix_boxes"](seed, N, H, W, prop_range, device)
        calls["cutmix_boxes"].append(dict(seed=word, N=N, H=H, W=W, prop_range=tuple(prop_range), out=got))
        return got

    def images(x, bx, roll=1):
        got = real["cutmix_images"](x, bx, roll)
        calls["cutmix_images"].append(dict(x=x, boxes=bx, roll=roll, out=got))
        return got

    def mixed(s_a, s_b, t_a, t_b, boxes=None, roll=1, tau=None, weight=1.0, out=None):
        assert s_a.requires_grad and s_b.requires_grad  # both networks are trained through the mixed forward
        assert not t_a.requires_grad and not t_b.requires_grad  # the teachers are constants
        loss = real["cross_pseudo_ce_mixed"](s_a, s_b, t_a, t_b, boxes, roll, tau, weight, out=out)
        calls["cross_pseudo_ce_mixed"].append(dict(s_a=s_a.detach().clone(), s_b=s_b.detach().clone(), t_a=t_a.clone(),
                                                   t_b=t_b.clone(), boxes=boxes, roll=roll, tau=tau, weight=weight,
                                                   loss=loss.detach().clone(), out=out))
        return loss

    def plain(a_logits, b_logits, tau=None, weight=1.0, out=None):
        loss = real["cross_pseudo_ce"](a_logits, b_logits, tau, weight, out=out)
        calls["cross_pseudo_ce"].append(dict(a=a_logits.detach().clone(), b=b_logits.detach().clone(), tau=tau, weight=weight,
                                             loss=loss.detach().clone(), out=out))
        return loss

    for name, fn in zip(NEW + ("cross_pseudo_ce",), (boxes, images, mixed, plain)):
        monkeypatch.setattr(F_hip, name, fn)
    return calls, real


@pytest.mark.parametrize("params", [ALL, ONLY], ids=["all-four", "cutmix-only"])
def test_one_step_returns_the_peer_loss_plus_the_weighted_terms(monkeypatch, params):
    from spcl_amd import functional as F_hip
    sd, model, hook, ep, flat = _setup("CrossPseudoParameters", params)
    assert hook.cutmix and hook.draw.is_cuda and hook.draw.tolist() == [23]
    calls, real = _spy(monkeypatch)
    lab, unl = _batch(2, 64, 1), _batch(2, 64, 2)
    limg, uimg, utf, target = _images(ep, lab, unl, 1234)
    want_boxes = O.boxes(23, 2, 64, 64, (0.25, 0.5))
    want_mixed = O.mix_images(uimg, want_boxes, 1)
    with torch.no_grad():  # the two networks' own forwards of the step's images, on twins (training mode: batch statistics)
        want_peer = _clone_net(hook.peer)(torch.cat([limg, uimg, utf], dim=0))
        want_peer_mixed = _clone_net(hook.peer)(want_mixed)
        want_model = _clone_net(model)(torch.cat([limg, uimg, utf], dim=0))
        want_model_mixed = _clone_net(model)(want_mixed)
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(lab, unl, seed=1234)
    torch.cuda.synchronize()
    n_on = len(params["on"])
    assert len(calls["cross_pseudo_ce"]) == n_on - 1  # on: [cutmix] alone never calls the unmixed criterion
    assert [len(calls[k]) for k in NEW] == [1, 1, 1]
    b, i, m = calls["cutmix_boxes"][0], calls["cutmix_images"][0], calls["cross_pseudo_ce_mixed"][0]
    assert b["seed"].tolist() == [23] and (b["N"], b["H"], b["W"]) == (2, 64, 64) and b["prop_range"] == (0.25, 0.5)
    assert torch.equal(b["out"].cpu(), want_boxes)
    assert hook.draw.tolist() == [24]  # advanced by one
    assert i["x"].shape == (2, 1, 64, 64) and torch.equal(i["x"], uimg) and i["boxes"] is b["out"] and i["roll"] == 1
    assert torch.equal(i["out"], want_mixed)
    assert m["boxes"] is b["out"] and m["roll"] == 1 and m["tau"] is None and m["weight"] == 2 / (2 * n_on)
    assert torch.equal(m["t_a"], want_model[2:4]) and torch.equal(m["t_b"], want_peer[2:4])  # the pass the step has made
    assert torch.equal(m["s_a"], want_model_mixed) and torch.equal(m["s_b"], want_peer_mixed)
    total, agree, kept = None, 0, 0
    for c in calls["cross_pseudo_ce"]:
        assert c["weight"] == 2 / (2 * n_on) and c["tau"] is None
        out = []
        again = real["cross_pseudo_ce"](c["a"], c["b"], None, c["weight"], out=out)
        assert torch.equal(again, c["loss"])
        total = again if total is None else total + again
        agree += int(out[1][16])
        kept += int(out[1][8:16].sum())
    out = []
    again = real["cross_pseudo_ce_mixed"](m["s_a"], m["s_b"], m["t_a"], m["t_b"], m["boxes"], 1, None, m["weight"], out=out)
    assert torch.equal(again, m["loss"])
    for x, y in zip(out, m["out"]):
        assert torch.equal(x, y)
    total = again if total is None else total + again
    agree += int(out[1][16])
    kept += int(out[1][8:16].sum())
    inside = int(out[1][17])
    assert inside == int(O.inside(want_boxes, 64, 64).sum())
    peer_sup, _ = F_hip.sup_loss_kl_onehot(want_peer[:2], target, 1e-16)
    assert torch.equal(reg.detach(), peer_sup + 0.5 * total)
    pixels = n_on * 2 * 64 * 64
    got = ep.meters.statistics()["cps"]
    print(f"cps cutmix step ({params['on']}): sup {float(sup):.6f}, peer sup {float(peer_sup):.6f}, cross {float(total):.6f}, "
          f"mixed term {float(again):.6f}, agree {agree} and kept {kept} / 2 of {pixels}, inside {inside}")
    assert got["loss"]["mean"] == pytest.approx(float(total), rel=1e-6)
    assert got["peer_sup_loss"]["mean"] == pytest.approx(float(peer_sup), rel=1e-6)
    assert got["agree"]["mean"] == pytest.approx(agree / pixels, rel=1e-6)
    assert got["kept"]["mean"] == pytest.approx(kept / (2 * pixels), rel=1e-6) and kept == 2 * pixels
    assert got["mixed"]["mean"] == pytest.approx(inside / (2 * 64 * 64), rel=1e-6) and 0.2 < got["mixed"]["mean"] < 0.55
    assert bool(torch.isfinite(reg)) and float(again) > 0.0
    ep.close_hooks()


def _pullback(net, images, mixed, target, other, other_mixed, bx, on, weight, student_side):
    """gradients of ``sup + weight * sum_m share * term_m`` w.r.t. ``net``'s parameters: its supervised loss on the device, and
    the float64 gradients of the terms w.r.t. its class maps -- the three unmixed ones and the one of the mixed batch -- pulled
    back through its two forwards.  ``other`` / ``other_mixed``: the other network's f32 logits (labels, no gradient)."""
    from spcl_amd import functional as F_hip
    logits = net(torch.cat(images, dim=0))
    logits_mixed = net(mixed)
    sup, _ = F_hip.sup_loss_kl_onehot(logits[:2], target, 1e-16)
    mine, mine_mixed = logits.detach().cpu(), logits_mixed.detach().cpu()
    other, other_mixed = other.cpu(), other_mixed.cpu()
    share = 2 / (2 * len(on))
    every = torch.ones(2, 64, 64, dtype=torch.bool)
    d, d_mixed = torch.zeros_like(mine, dtype=torch.float64), None
    cross = 0.0
    for k, name in enumerate(("labeled", "unlabeled", "unlabeled_tf")):
        if name not in on:
            continue
        x, o = mine[2 * k:2 * k + 2], other[2 * k:2 * k + 2]
        x64 = x.double().requires_grad_(True)
        yx, yo = CO.conf_and_label(x)[1], CO.conf_and_label(o)[1]
        term = CO.loss(x64, o.double(), yx, yo, every, every, share) if student_side else \
            CO.loss(o.double(), x64, yo, yx, every, every, share)
        term.backward()
        d[2 * k:2 * k + 2] = weight * x64.grad
        cross += float(term.detach())
    # the mixed term: the teachers are the two networks' UNMIXED unlabelled maps, gathered through the boxes
    t_mine, t_other = mine[2:4], other[2:4]
    x64 = mine_mixed.double().requires_grad_(True)
    if student_side:
        _, yA, _, yB = O.teachers(t_mine, t_other, bx, 1)
        term = O.loss(x64, other_mixed.double(), yA, yB, every, every, share)
    else:
        _, yA, _, yB = O.teachers(t_other, t_mine, bx, 1)
        term = O.loss(other_mixed.double(), x64, yA, yB, every, every, share)
    term.backward()
    d_mixed = weight * x64.grad
    cross += float(term.detach())
    params = dict(net.named_parameters())
    grads = torch.autograd.grad([sup, logits, logits_mixed], list(params.values()),
                                grad_outputs=[torch.ones_like(sup), d.float().to(DEV), d_mixed.float().to(DEV)])
    return float(sup), cross, dict(zip(params, grads))


@pytest.mark.parametrize("params", [ALL, ONLY], ids=["all-four", "cutmix-only"])
def test_step_gradients_of_both_networks_vs_float64_pullback(params):
    sd, model, hook, ep, flat = _setup("CrossPseudoParameters", params)
    lab, unl = _batch(2, 64, 1), _batch(2, 64, 2)
    *images, target = _images(ep, lab, unl, 1234)
    bx = O.boxes(23, 2, 64, 64)
    mixed = O.mix_images(images[1], bx, 1)
    student_twin, peer_twin = _clone_net(model), _clone_net(hook.peer)
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(lab, unl, seed=1234)
    torch.cuda.synchronize()
    with torch.no_grad():  # (training mode: batch statistics, the same at every pass)
        s_logits, s_mixed = student_twin(torch.cat(images, dim=0)), student_twin(mixed)
        p_logits, p_mixed = peer_twin(torch.cat(images, dim=0)), peer_twin(mixed)
    on = params["on"]
    osup, cross, ref = _pullback(student_twin, images, mixed, target, p_logits, p_mixed, bx, on, 0.5, True)
    psup, cross_p, ref_p = _pullback(peer_twin, images, mixed, target, s_logits, s_mixed, bx, on, 0.5, False)
    assert abs(float(sup) - osup) <= 1e-4 * abs(osup), (float(sup), osup)
    assert cross == pytest.approx(cross_p, rel=1e-12)
    want = psup + 0.5 * cross
    assert abs(float(reg) - want) <= 1e-4 * abs(want), (float(reg), want)
    _check_step_grads(model, flat, ref)  # d sup + weight * (the unmixed terms + the mixed term), at the siblings' 5e-3 bar
    _check_step_grads(hook.peer, flat, ref_p)
    ep.close_hooks()


def test_two_stage_with_disable_bn_moves_both_networks_statistics_by_the_labelled_pass_alone():
    sd, model, hook, ep, flat = _setup("CrossPseudoParameters", ALL)
    ep._two_stage, ep._disable_bn = True, True
    lab, unl = _batch(2, 64, 1), _batch(2, 64, 2)
    limg, uimg, utf, _ = _images(ep, lab, unl, 1234)
    refs = []
    for net in (model, hook.peer):
        twin = _clone_net(net)
        with torch.no_grad():
            twin(limg)
        refs.append({k: v.cpu() for k, v in twin.state_dict().items() if "running" in k})
    start = {k: v.detach().cpu().clone() for k, v in hook.peer.state_dict().items() if "running" in k}
    with ep.meters.focus_on(ep.meter_focus):
        ep.step(lab, unl, seed=1234)
    torch.cuda.synchronize()
    for net, ref in zip((model, hook.peer), refs):  # every BatchNorm of both networks: the mixed forwards left no trace
        for k, v in net.state_dict().items():
            if "running" in k:
                assert torch.allclose(v.cpu(), ref[k], rtol=1e-4, atol=1e-6), k
    assert not torch.equal(hook.peer.state_dict()[BN_KEY].cpu(), start[BN_KEY])
    from tests.test_gpu_semi_step import UNetStats
    assert torch.allclose(model.state_dict()[BN_KEY].cpu(), UNetStats.after_labelled_pass(sd, lab), rtol=1e-4, atol=1e-6)
    ep.close_hooks()


def test_without_two_stage_the_mixed_forwards_do_move_the_statistics():
    """the counterpart: a plain pass is a plain pass (what ``_forward_pass`` does for the unlabelled batches there)"""
    sd, model, hook, ep, flat = _setup("CrossPseudoParameters", ONLY)
    lab, unl = _batch(2, 64, 1), _batch(2, 64, 2)
    limg, uimg, utf, _ = _images(ep, lab, unl, 1234)
    twin = _clone_net(hook.peer)
    with torch.no_grad():
        twin(torch.cat([limg, uimg, utf], dim=0))
    with ep.meters.focus_on(ep.meter_focus):
        ep.step(lab, unl, seed=1234)
    torch.cuda.synchronize()
    assert not torch.allclose(hook.peer.state_dict()[BN_KEY].cpu(), twin.state_dict()[BN_KEY].cpu(), rtol=1e-4, atol=1e-6)
    with torch.no_grad():
        twin(O.mix_images(uimg, O.boxes(23, 2, 64, 64), 1))
    assert torch.allclose(hook.peer.state_dict()[BN_KEY].cpu(), twin.state_dict()[BN_KEY].cpu(), rtol=1e-4, atol=1e-6)
    ep.close_hooks()


@pytest.mark.parametrize("params", [ALL, {"weight": 0.5, "threshold": [0.2, 0.3, 0.3, 0.3], "on": ["cutmix"]}],
                         ids=["all-four", "cutmix-only-tau"])
def test_further_steps_issue_no_host_synchronisation(params):
    sd, model, hook, ep, flat = _setup("CrossPseudoParameters", params)
    first = hook.draw.tolist()[0]
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
    assert hook.draw.tolist() == [first + 3]
    got = ep.meters.statistics()["cps"]
    assert 0.0 <= got["agree"]["mean"] <= 1.0 and 0.0 < got["kept"]["mean"] <= 1.0 and 0.2 < got["mixed"]["mean"] < 0.55
    ep.close_hooks()


def test_one_unlabelled_slice_is_refused():
    sd, model, hook, ep, flat = _setup("CrossPseudoParameters", ONLY)
    with pytest.raises(RuntimeError, match="fewer than two"):
        with ep.meters.focus_on(ep.meter_focus):
            ep.step(_batch(2, 64, 1), _batch(1, 64, 2), seed=7)
    torch.cuda.synchronize()
    assert hook.draw.tolist() == [23]  # refused before a box was drawn
    ep.close_hooks()


def test_without_cutmix_nothing_new_is_called_and_keys_and_meters_are_the_parents(monkeypatch):
    sd, model, hook, ep, flat = _setup("CrossPseudoParameters", {"weight": 0.5})
    calls, _ = _spy(monkeypatch)
    with ep.meters.focus_on(ep.meter_focus):
        ep.step(_batch(2, 64, 1), _batch(2, 64, 2), seed=1234)
    torch.cuda.synchronize()
    assert [len(calls[k]) for k in NEW] == [0, 0, 0] and len(calls["cross_pseudo_ce"]) == 3
    assert sorted(k for k in hook.state_dict() if not k.startswith("_peer.")) == ["tau"]
    assert sorted(ep.meters.statistics()["cps"]) == ["agree", "kept", "loss", "peer_sup_loss"]
    assert hook().graph_key() == ("_CrossPseudoEpocherHook", 0.5, ("labeled", "unlabeled", "unlabeled_tf"), "plain")
    ep.close_hooks()


# ------------------------------------------------------------------------------------------------------------ trainer
def test_two_seeded_trainer_runs_are_identical_and_the_checkpoint_holds_the_seed_word(tmp_path):
    ends = []
    for run in range(2):
        tr, model, _, _ = _trainer(_cfg(CrossPseudoParameters=ALL), save_dir=str(tmp_path) if run == 0 else None)
        random.seed(7)
        hist = tr.start_training()
        torch.cuda.synchronize()
        assert len(hist) == 2
        for name in ("loss", "peer_sup_loss", "agree", "kept", "mixed"):
            assert name in str(hist[-1]["tra"]), name
        hook = tr.__hooks__[0]
        assert hook.draw.tolist() == [23 + 6]  # two epochs of three steps
        ends.append((_state(model), _state(hook.peer)))
    (ma, pa), (mb, pb) = ends
    assert all(torch.equal(ma[k], mb[k]) for k in ma) and all(torch.equal(pa[k], pb[k]) for k in pa)
    saved = torch.load(tmp_path / "last.pth", map_location="cpu")
    assert sorted(k for k in saved["__hooks__"] if not k.startswith("0._peer.")) == ["0.draw", "0.tau"]
    assert saved["__hooks__"]["0.draw"].tolist() == [29]


def test_trainer_round_trip_restores_the_seed_word_and_the_next_step():
    tr, model, lab, unl = _trainer(_cfg(CrossPseudoParameters=ALL))
    hook = tr.__hooks__[0]
    ep = tr._create_tra_epoch()
    with ep.meters.focus_on(ep.meter_focus):
        for k in range(2):
            ep.step(lab[k], unl[k], seed=100 + k)
        torch.cuda.synchronize()
        blob = io.BytesIO()
        torch.save(tr.state_dict(), blob)
        assert hook.draw.tolist() == [25]
        ep.step(lab[2], unl[2], seed=102)
    torch.cuda.synchronize()
    ep.close_hooks()
    want_m, want_p = _state(model), _state(hook.peer)

    blob.seek(0)
    saved = torch.load(blob, map_location="cpu")
    other = dict(ALL, peer_seed=5, cutmix={"seed": 1000})  # (other initial weights, another peer, another first seed word)
    tr2, model2, _, _ = _trainer(_cfg(CrossPseudoParameters=other), seed=4)
    hook2 = tr2.__hooks__[0]
    assert hook2.draw.tolist() == [1000]
    tr2.load_state_dict(saved)
    assert hook2.draw.tolist() == [25]
    ep2 = tr2._create_tra_epoch()
    with ep2.meters.focus_on(ep2.meter_focus):
        ep2.step(lab[2], unl[2], seed=102)
    torch.cuda.synchronize()
    ep2.close_hooks()
    assert hook2.draw.tolist() == [26]
    got_m, got_p = _state(model2), _state(hook2.peer)
    assert all(torch.equal(got_m[k], want_m[k]) for k in want_m)
    assert all(torch.equal(got_p[k], want_p[k]) for k in want_p)
