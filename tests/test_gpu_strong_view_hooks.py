"""GPU: the strong-view hook (semi_seg/hooks/strongview.py) under ``SemiSupervisedEpocher.step`` on the tiny UNet of
tests/test_gpu_cps_hooks.py (``max_channel`` 128, 2 + 2 slices of 64 x 64).

With every gate shut two steps are what two steps without the hook are, bit for bit, alone and beside the pseudo-labelling
hook.  With the defaults the ``unlabeled_image_tf`` the other hooks receive is ``functional.strong_view`` of the cf image under
that step's ``draw``, which advances by one per step; a run saved after step 2 and resumed gives step 3's bits.  Beside
``PseudoLabelParameters`` (``teacher: self``) the loss is finite, the student's gradient non-zero and ``ops`` is filled; beside
``CrossPseudoParameters`` the peer's ``unlabeled_tf`` map is computed on the strong image."""
import io

import pytest
import torch

from tests.test_gpu_cps_hooks import _cfg, _clone_net, _state, _trainer
from tests.test_gpu_semi_reg_hooks import _unet
from tests.test_gpu_semi_step import _batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPS = ("gamma", "contrast", "brightness", "blur", "noise")
OFF = dict({name: {"p": 0.0} for name in OPS}, seed=5)
PSEUDO = {"weight": 1.0, "threshold": 0.3, "teacher": "self"}


def _setup(sections, lr=0.05):
    """the model of ``_unet`` and a ``SemiSupervisedEpocher`` with the hooks of ``sections``, stepped by plain SGD on the flat
    parameter -> (model, trainer hooks by section, epocher, flat)"""
    from spcl_amd import ddp
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    _, model = _unet()
    hooks = create_hook_from_config(model, dict({"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 2}}, **sections))
    for h in hooks:
        h.to(DEV)
    flat = ddp.FlatParams([p for p in model.parameters() if p.requires_grad] +
                          [p for h in hooks for p in h.parameters() if p.requires_grad])
    opt = torch.optim.SGD([flat.param], lr=lr)
    ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=[], unlabeled_loader=[], sup_criterion=KL_div(),
                               num_batches=1, device=DEV, flat_params=flat)
    ep.add_hooks([h() for h in hooks])
    return model, {type(h).__name__: h for h in hooks}, ep, flat


def _two_steps(sections):
    model, hooks, ep, flat = _setup(sections)
    losses = []
    with ep.meters.focus_on(ep.meter_focus):
        for k in range(2):
            sup, reg = ep.step(_batch(2, 64, 1 + 2 * k), _batch(2, 64, 2 + 2 * k), seed=1234 + k)
            losses += [sup.detach().clone(), reg.detach().clone()]
    torch.cuda.synchronize()
    ep.close_hooks()
    return losses, _state(model), hooks, ep


@pytest.mark.parametrize("beside", [{}, {"PseudoLabelParameters": PSEUDO}], ids=["alone", "beside-pseudolabel"])
def test_with_every_gate_shut_two_steps_are_what_they_were(beside):
    base_losses, base_state, _, base_ep = _two_steps(dict(beside))
    losses, state, hooks, ep = _two_steps(dict(beside, StrongViewParameters=OFF))
    assert hooks["StrongViewTrainerHook"].draw.tolist() == [7]
    for a, b in zip(base_losses, losses):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    assert all(torch.equal(state[k], base_state[k]) for k in base_state) and sorted(state) == sorted(base_state)
    if not beside:  # a step whose only hook is this one keeps the zero reg_loss it had
        assert float(losses[1]) == 0.0 and float(losses[3]) == 0.0
    assert ep.meters.statistics()["strongview"]["ops"]["mean"] == 0.0
    want, got = base_ep.meters.statistics(), ep.meters.statistics()
    assert sorted(got) == sorted(list(want) + ["strongview"])


class _Probe:
    """an epocher hook that keeps what the epocher hands to hooks"""
    meters = None

    def __init__(self):
        self.seen = []

    def set_epocher(self, epocher):
        pass

    def before_forward_pass(self, **kwargs):
        self.seen.append(("forward", kwargs["unlabeled_image_tf"]))

    def after_forward_pass(self, **kwargs):
        pass

    before_regularization = after_regularization = after_forward_pass

    def __call__(self, *, unlabeled_image_tf, unlabeled_logits_tf, unlabeled_logits, flip_flags, **kwargs):
        self.seen.append(("call", unlabeled_image_tf, unlabeled_logits_tf.detach(), unlabeled_logits.detach(), flip_flags))
        return unlabeled_logits.sum() * 0.0

    def close(self):
        pass


def test_hooks_receive_the_strong_view_of_that_steps_draw_and_draw_advances():
    from spcl_amd import functional as F_hip
    model, hooks, ep, flat = _setup({"StrongViewParameters": {"seed": 40}})
    owner = hooks["StrongViewTrainerHook"]
    probe = _Probe()
    ep.add_hook(probe)
    assert owner.draw.is_cuda and owner.draw.tolist() == [40]
    counts = []
    with ep.meters.focus_on(ep.meter_focus):
        for k in range(3):
            lab, unl = _batch(2, 64, 10 + k), _batch(2, 64, 20 + k)
            ep.step(lab, unl, seed=300 + k)
            torch.cuda.synchronize()
            assert owner.draw.tolist() == [41 + k]
            flags = ep.flip_flags(300 + k, 2)
            table = []
            want = F_hip.strong_view(unl[0][1].to(DEV), flags, 40 + k, owner.config, out=table)
            (_, fwd), (_, tf, logits_tf, logits, got_flags) = probe.seen[-2:]
            assert fwd is tf and torch.equal(tf, want) and torch.equal(got_flags, flags)
            plain = F_hip.flip_batch(unl[0][1].to(DEV).contiguous(), flags)
            assert not torch.equal(tf, plain)
            assert float(tf.min()) >= 0.0 and float(tf.max()) <= 1.0
            # intensity ops move no pixel: the flipped logits are still the plain flip of the weak view's logits
            assert torch.equal(logits_tf, F_hip.flip_batch(logits, flags))
            counts.append(float(table[0][:, 8].mean()))
    ep.close_hooks()
    stats = ep.meters.statistics()["strongview"]["ops"]["mean"]
    print(f"strong view: applied ops per slice over three steps {counts}, meter {stats:.4f}")
    assert stats == pytest.approx(sum(counts) / 3, rel=1e-6) and stats > 0.0


def test_a_run_saved_after_step_two_and_resumed_gives_step_threes_bits():
    cfg = _cfg(PseudoLabelParameters=PSEUDO, StrongViewParameters={"seed": 9})
    tr, model, lab, unl = _trainer(cfg)
    hook = tr.__hooks__[1]
    assert type(hook).__name__ == "StrongViewTrainerHook"
    ep = tr._create_tra_epoch()
    with ep.meters.focus_on(ep.meter_focus):
        for k in range(2):
            ep.step(lab[k], unl[k], seed=100 + k)
        torch.cuda.synchronize()
        assert hook.draw.tolist() == [11]
        blob = io.BytesIO()
        torch.save(tr.state_dict(), blob)
        ep.step(lab[2], unl[2], seed=102)
    torch.cuda.synchronize()
    ep.close_hooks()
    want = _state(model)
    assert hook.draw.tolist() == [12]

    blob.seek(0)
    saved = torch.load(blob, map_location="cpu")
    assert saved["__hooks__"]["1.draw"].tolist() == [11]
    tr2, model2, _, _ = _trainer(_cfg(PseudoLabelParameters=PSEUDO, StrongViewParameters={"seed": 77}), seed=4)
    tr2.load_state_dict(saved)
    hook2 = tr2.__hooks__[1]
    assert hook2.draw.tolist() == [11]
    ep2 = tr2._create_tra_epoch()
    with ep2.meters.focus_on(ep2.meter_focus):
        ep2.step(lab[2], unl[2], seed=102)
    torch.cuda.synchronize()
    ep2.close_hooks()
    got = _state(model2)
    assert all(torch.equal(got[k], want[k]) for k in want) and hook2.draw.tolist() == [12]
    # ... and the draw matters: the same step under another word ends elsewhere
    tr3, model3, _, _ = _trainer(_cfg(PseudoLabelParameters=PSEUDO, StrongViewParameters={"seed": 77}), seed=4)
    tr3.load_state_dict(saved)
    tr3.__hooks__[1].draw.fill_(500)
    ep3 = tr3._create_tra_epoch()
    with ep3.meters.focus_on(ep3.meter_focus):
        ep3.step(lab[2], unl[2], seed=102)
    torch.cuda.synchronize()
    ep3.close_hooks()
    other = _state(model3)
    assert any(not torch.equal(other[k], want[k]) for k in want)


def test_beside_self_taught_pseudo_labels_the_student_learns_from_the_strong_view():
    sections = {"PseudoLabelParameters": PSEUDO,
                "StrongViewParameters": dict({name: {"p": 1.0} for name in OPS}, seed=3)}
    model, hooks, ep, flat = _setup(sections)
    before = _state(model)
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(_batch(2, 64, 1), _batch(2, 64, 2), seed=1234)
    torch.cuda.synchronize()
    ep.close_hooks()
    sup, reg = sup.detach(), reg.detach()
    assert bool(torch.isfinite(sup)) and bool(torch.isfinite(reg)) and float(reg) > 0.0
    views = {id(p): v for p, v in zip(flat.params, flat.views)}
    grads = [views[id(p)] for p in model.parameters()]
    assert all(bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0.0 for g in grads)
    after = _state(model)
    assert any(not torch.equal(after[k], before[k]) for k in before if "running" not in k and "num_batches" not in k)
    stats = ep.meters.statistics()
    assert stats["strongview"]["ops"]["mean"] == 5.0  # every gate open
    assert stats["pseudolabel"]["mask_ratio"]["mean"] > 0.0
    # with the plain flip the self-taught student repeats itself: the strong view changes the loss
    model_w, _, ep_w, _ = _setup({"PseudoLabelParameters": PSEUDO})
    with ep_w.meters.focus_on(ep_w.meter_focus):
        _, reg_w = ep_w.step(_batch(2, 64, 1), _batch(2, 64, 2), seed=1234)
    torch.cuda.synchronize()
    ep_w.close_hooks()
    reg_w = reg_w.detach()
    print(f"pseudo-label loss on the weak pair {float(reg_w):.6f}, on the strong view {float(reg):.6f}")
    assert float(reg_w) != float(reg)


def test_beside_cross_pseudo_supervision_the_peer_reads_the_strong_image(monkeypatch):
    from spcl_amd import functional as F_hip
    sections = {"CrossPseudoParameters": {"weight": 0.5, "on": ["unlabeled_tf"]},
                "StrongViewParameters": dict({name: {"p": 1.0} for name in OPS}, seed=21)}
    model, hooks, ep, flat = _setup(sections)
    cps, owner = hooks["CrossPseudoTrainerHook"], hooks["StrongViewTrainerHook"]
    calls = []
    real = F_hip.cross_pseudo_ce

    def spy(a_logits, b_logits, tau=None, weight=1.0, out=None):
        calls.append((a_logits.detach().clone(), b_logits.detach().clone()))
        return real(a_logits, b_logits, tau, weight, out=out)

    monkeypatch.setattr(F_hip, "cross_pseudo_ce", spy)
    lab, unl = _batch(2, 64, 1), _batch(2, 64, 2)
    flags = ep.flip_flags(1234, 2)
    strong = F_hip.strong_view(unl[0][1].to(DEV), flags, 21, owner.config)
    weak = F_hip.flip_batch(unl[0][1].to(DEV).contiguous(), flags)
    assert not torch.equal(strong, weak)
    images = [lab[0][0].to(DEV), unl[0][0].to(DEV)]
    with torch.no_grad():  # twins in training mode: batch statistics, the same at every pass
        want_peer = _clone_net(cps.peer)(torch.cat(images + [strong], dim=0))[4:6]
        want_model = _clone_net(model)(torch.cat(images + [strong], dim=0))[4:6]
        weak_peer = _clone_net(cps.peer)(torch.cat(images + [weak], dim=0))[4:6]
    with ep.meters.focus_on(ep.meter_focus):
        ep.step(lab, unl, seed=1234)
    torch.cuda.synchronize()
    ep.close_hooks()
    assert len(calls) == 1 and owner.draw.tolist() == [22]
    a, b = calls[0]
    assert torch.equal(a, want_model) and torch.equal(b, want_peer) and not torch.equal(b, weak_peer)
