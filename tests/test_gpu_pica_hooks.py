"""GPU: the PICA baseline above the kernels -- the classes ``PUILoss`` / ``PUISegLoss`` called with probabilities against the
reference's recorded results (tests/golden/g13_pica.npz), ``from_logits`` against the class call, ``PICATrainHook`` on real
tapped UNet features against the float64 restatement (tests/_pica_oracle.py), one ``SemiTrainer`` epoch built from
``PICAConsistencyParams``, and a captured criterion call replayed to the eager bits.

Bars of the fixture checks: loss max(4 x the recorded float32-vs-float64 gap of the reference, 2^-22) relative; gradient w.r.t.
``y`` max(1e-5, 4 x the recorded gap) relative L2.  The classes take probabilities through their logarithm (the kernels apply
a softmax), so the gradient a probability map receives is the recorded one without its component along (1, ..., 1) at each
pixel, ``g - sum_k g_k p_k`` -- the part a map confined to the simplex can follow; the recorded gradient is projected the same
way before the comparison."""
import math
import os
import re

import pytest
import torch

from tests import _iic_oracle as R
from tests import _pica_oracle as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_pica.npz")


def _criterion(kind, pad, lamda, **kw):
    from spcl_amd.contrastyou.losses.pica_loss import PUILoss, PUISegLoss
    return PUILoss(lamda=lamda, **kw) if kind == "pui" else PUISegLoss(lamda=lamda, padding=pad, **kw)


@pytest.mark.parametrize("case", P.GOLDEN_CASES, ids=[P.case_key(*c) for c in P.GOLDEN_CASES])
def test_classes_on_probabilities_vs_the_references_recorded_results(case):
    kind, N, K, H, W, pad, lamda = case
    key = P.case_key(*case)
    _, z = P.load_golden(GOLDEN)
    x, y = z[key + "/x"], z[key + "/y"]
    crit = _criterion(kind, pad, lamda, check_inputs=True)
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    loss = crit(xd.flatten(1), yd.flatten(1)) if kind == "pui" else crit(xd, yd)
    loss.backward()
    torch.cuda.synchronize()
    bar_loss = max(4.0 * float(z[key + "/gap_loss"]), 2.0 ** -22)
    bar_gy = max(1e-5, 4.0 * float(z[key + "/gap_gy"]))
    want_gy = z[key + "/gy"].double()
    want_gy = want_gy - (want_gy * y.double()).sum(1, keepdim=True)
    got_l, got_g = P.rel(loss.detach().cpu(), z[key + "/loss"]), P.rel_l2(yd.grad.cpu(), want_gy)
    print(f"{key}: loss {float(loss):.9g} vs {float(z[key + '/loss']):.9g}: {got_l:.2e} (bar {bar_loss:.2e}); "
          f"gy {got_g:.2e} (bar {bar_gy:.2e}); ce {float(crit.last_ce):.9g}")
    assert got_l <= bar_loss, (got_l, bar_loss)
    assert got_g <= bar_gy, (got_g, bar_gy)
    ce64 = P.run_case(x, y, kind, pad, lamda, torch.float64)[1]
    assert P.rel(crit.last_ce.cpu(), ce64) <= 1e-5, (float(crit.last_ce), float(ce64))
    assert xd.grad is not None and bool(torch.isfinite(xd.grad).all())


@pytest.mark.parametrize("kind,pad", [("pui", 0), ("seg", 1)])
def test_from_logits_equals_the_class_call_on_softmax(kind, pad):
    N, K, H, W = (6, 10, 1, 1) if kind == "pui" else (2, 10, 9, 7)
    g = torch.Generator().manual_seed(5)
    lx, ly = torch.randn(N, K, H, W, generator=g).to(DEV), torch.randn(N, K, H, W, generator=g).to(DEV)
    crit = _criterion(kind, pad, 2.0)
    a = crit.from_logits(lx, ly, num_subheads=1, num_clusters=K)
    ce_a = crit.last_ce.clone()
    px, py = lx.softmax(1), ly.softmax(1)
    b = crit(px.flatten(1), py.flatten(1)) if kind == "pui" else crit(px, py)
    # the same function of the same probabilities up to their float32 rounding: the bars of the kernel tests
    assert P.rel(a.cpu(), b.cpu()) <= 1e-5 and P.rel(ce_a.cpu(), crit.last_ce.cpu()) <= 1e-5, (float(a), float(b))


def test_pica_hooks_vs_float64():
    from spcl_amd.contrastyou.meters import MeterInterface
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.hooks import create_pica_hooks
    torch.manual_seed(3)
    n, lamda = 2, 2.0
    model = UNet(input_dim=1, num_classes=4, max_channel=128).to(DEV).train().set_compute_dtype(torch.float32)
    hook = create_pica_hooks(model=model, feature_names=["Conv5", "Up_conv3"], weights=[0.1, 0.05], paddings=[1], lamda=lamda)
    hook.to(DEV)
    img = torch.rand(2 * n, 1, 48, 48, device=DEV)
    flags = torch.tensor([1, 2], dtype=torch.uint8, device=DEV)
    members = list(hook._hooks)
    assert all(h.learnable_modules == [h._projector] for h in members)
    ehooks = [h() for h in members]
    meters = MeterInterface(default_focus="semi")
    for eh in ehooks:
        eh.meters = meters
        eh.configure_meters(meters)
        eh.before_forward_pass()
    model(img)
    for eh in ehooks:
        eh.after_forward_pass()
    for th, eh in zip(members, ehooks):
        feat = eh._extractor.feature()[-2 * n:].detach()
        loss = eh(unlabeled_image=img[:n], unlabeled_image_tf=img[n:], affine_transformer=None, seed=0, flip_flags=flags)
        params = list(th._projector.parameters())
        grads = torch.autograd.grad(loss, params)
        torch.cuda.synchronize()
        f64 = feat.double().cpu()
        p64 = [p.detach().double().cpu().requires_grad_(True) for p in params]
        S = len(th._projector._headers)
        dense = th._feature_name != "Conv5"
        zs = []
        for s in range(S):
            w, b = p64[2 * s], p64[2 * s + 1]
            zs.append(torch.nn.functional.conv2d(f64, w, b) if dense else
                      (f64.mean(dim=(2, 3)) @ w.t() + b)[:, :, None, None])
        z = torch.cat(zs, 1)
        K = z.shape[1] // S
        ref, ref_ce = P.pica_hook_loss(z[:n], z[n:], S, K, th._criterion.padding if dense else 0, dense, [1, 2], lamda)
        gref = torch.autograd.grad(ref * th._weight, p64)
        ref, ref_ce = float(ref.detach()), float(ref_ce.detach())
        stats = meters.statistics()[th._hook_name]
        pui, pui_ce = stats["pui"]["mean"], stats["pui_ce"]["mean"]
        errs = [P.rel_l2(g, r) for g, r in zip(grads, gref)]
        print(f"{th._hook_name}: loss {float(loss):.9g} vs {ref * th._weight:.9g}; pui {pui:.9g}, pui_ce {pui_ce:.9g} vs "
              f"{ref_ce:.9g}; head gradients {max(errs):.2e}")
        assert P.rel(loss.detach().cpu(), ref * th._weight) <= 1e-5, (th._hook_name, float(loss), ref * th._weight)
        assert P.rel(pui, ref) <= 1e-5 and P.rel(pui_ce, ref_ce) <= 1e-5, (th._hook_name, pui, ref, pui_ce, ref_ce)
        if dense:  # the balance term is the constant of the shape
            M = n * feat.shape[2] * feat.shape[3]
            assert abs((ref - ref_ce) - lamda * (math.log(M) - M / K * math.log(K))) <= 1e-9 * abs(ref)
        assert max(errs) <= 1e-4, (th._hook_name, errs)
    for th, eh in zip(members, ehooks):
        tapped = getattr(model, "_" + th._feature_name)
        assert len(tapped._forward_hooks) == 1
        eh.close()
        assert len(tapped._forward_hooks) == 0


def test_semi_trainer_epoch_with_pica_consistency_params(tmp_path):
    from tests.test_gpu_semi_step import _batch
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.trainers.semi import SemiTrainer as ST
    torch.manual_seed(3)
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    lab = [_batch(2, 64, 30 + k) for k in range(3)]
    unl = [_batch(2, 64, 40 + k) for k in range(3)]
    val = [((b[0][0], b[0][2]), b[1], b[2]) for b in lab[:1]]
    cfg = {"Optim": {"name": "RAdam", "lr": 1e-5, "weight_decay": 1e-5}, "Data": {"name": "acdc"},
           "Trainer": {"max_epoch": 1},
           "PICAConsistencyParams": {"feature_names": ["Conv5", "Up_conv3"], "pica_weights": [0.1, 0.05], "dense_paddings": [1],
                                     "consistency_weight": 1.0, "lamda": 2.0}}
    tr = ST(model=model, labeled_loader=lab, unlabeled_loader=unl, val_loader=val, test_loader=None, criterion=KL_div(),
            save_dir=str(tmp_path), max_epoch=1, num_batches=3, device=DEV, two_stage=True, disable_bn=True, config=cfg)
    tr.register_hooks(*create_hook_from_config(model, cfg))
    tr.init()
    hist = tr.start_training()
    assert len(hist) == 1
    text = str(hist[-1]["tra"])
    print(text)
    for name in ("sup_loss", "reg_loss", "pica/conv5", "pica/up_conv3", "pui", "pui_ce", "consistency"):
        assert name in text, (name, text)
    assert "nan" not in text.lower() and "inf" not in text.lower(), text
    values = [float(v) for v in re.findall(r"-?\d+\.\d+(?:e[-+]?\d+)?", text)]
    assert values and all(math.isfinite(v) for v in values)


@pytest.mark.parametrize("kind", ["pui", "seg"])
def test_captured_criterion_call_replays_to_the_eager_bits(kind):
    """the criteria make no host synchronisation: forward and backward are captured in a graph and replayed"""
    S, K = 5, 20
    N, H, W = (5, 1, 1) if kind == "pui" else (2, 12, 10)
    g = torch.Generator().manual_seed(9)
    lx = torch.randn(N, S * K, H, W, generator=g).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ly = torch.randn(N, S * K, H, W, generator=g).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    flags = None if kind == "pui" else torch.tensor([1, 2], dtype=torch.uint8, device=DEV)
    crit = _criterion(kind, 1, 2.0)

    def call():
        loss = crit.from_logits(lx, ly, num_subheads=S, num_clusters=K, scale=1.0 / S, flags=flags)
        return (loss.detach().clone(), crit.last_ce.clone()) + tuple(t.clone() for t in torch.autograd.grad(loss, (lx, ly)))

    eager = call()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = call()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, eager):
        assert torch.equal(a, b)
