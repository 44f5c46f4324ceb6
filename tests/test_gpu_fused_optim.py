"""The fused Adam / AdamW / SGD steps (csrc/optim.hip, optim.py): parity with ``torch.optim`` on the CPU, the protocol they share
with ``FusedRAdam`` (``grad_scale``, ``scalar_adds``, staged steps, ``state_dict``), the epochers' step replayed from a hipGraph
with them, and ``build_optimizer``'s choice of class.

The parity bar is the RAdam kernel's (tests/test_gpu_kernels.py::test_fused_radam_matches_torch_radam): rtol 2e-6, atol 2e-7
on the parameter after every one of 9 steps.  torch's own f32 step stays within a third of that bar of its float64 twin on
these configurations, so two correct f32 implementations fit inside it."""
import ctypes
import io
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64          # floats on either side of the parameter (a multiple of 4: the parameter stays 16-byte aligned)
SENTINEL = -77.25
BIG = 2048 * 256 * 4 + 1027  # beyond one pass of the capped grid (2048 x 256 threads x 4 floats), plus a tail of 3

CONFIGS = {
    "adam-wd": ("Adam", dict(weight_decay=1e-2)),
    "adam-decoupled": ("Adam", dict(weight_decay=1e-2, decoupled_weight_decay=True)),
    "adamw": ("AdamW", dict(weight_decay=1e-2)),
    "sgd": ("SGD", dict()),
    "sgd-momentum": ("SGD", dict(momentum=0.9)),
    "sgd-dampening": ("SGD", dict(momentum=0.9, dampening=0.1)),
    "sgd-nesterov-wd": ("SGD", dict(momentum=0.9, nesterov=True, weight_decay=1e-2)),
}


def _fused(name):
    from spcl_amd import optim
    return {"Adam": optim.FusedAdam, "AdamW": optim.FusedAdamW, "SGD": optim.FusedSGD}[name]


def _guarded(p0):
    """a CUDA parameter holding ``p0`` inside a larger buffer of sentinels; returns (parameter, check)"""
    n = p0.numel()
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    buf[GUARD:GUARD + n] = p0.cuda()
    p = torch.nn.Parameter(buf[GUARD:GUARD + n])
    assert p.data_ptr() % 16 == 0 and p.is_contiguous()

    def check():
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())
    return p, check


@pytest.mark.parametrize("n", [1, 7, 10007, BIG])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_fused_step_matches_torch_optim(config, n):
    name, kw = CONFIGS[config]
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=g)
    ref_p = torch.nn.Parameter(p0.clone())
    hip_p, check_guard = _guarded(p0)
    ref = getattr(torch.optim, name)([ref_p], lr=2e-3, foreach=False, **kw)
    hip = _fused(name)([hip_p], lr=2e-3, **kw)
    for it in range(9):
        grad = torch.randn(n, generator=g) * (1.0 + it)
        if it == 6:
            for o in (ref, hip):
                o.param_groups[0]["lr"] = 5e-4
        ref_p.grad = grad.clone()
        hip_p.grad = grad.cuda()
        ref.step()
        hip.step()
        got, want = hip_p.detach().cpu().numpy(), ref_p.detach().numpy()
        if it in (0, 8):
            print(f"{config} n={n} step {it + 1}: max |diff| / (atol + rtol |ref|) = "
                  f"{float(np.max(np.abs(got - want) / (2e-7 + 2e-6 * np.abs(want)))):.3f}")
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-7, err_msg=f"step {it + 1}")
    check_guard()
    st = hip.state[hip_p]
    assert st["step"].dtype == torch.int64 and int(st["step"]) == 9
    rst = ref.state[ref_p]

    def moment_close(key):
        # a signed running sum (terms cancel): each of the 9 steps rounds it once, by at most half an ulp of its current
        # magnitude, in either implementation -- 9 ulps of the largest entry bound the distance of the two
        want = rst[key].numpy()
        np.testing.assert_allclose(st[key].cpu().numpy(), want, rtol=1e-5, atol=9 * 2.0 ** -23 * float(np.abs(want).max()))

    if name == "SGD":
        if kw.get("momentum", 0.0) == 0.0:
            assert "momentum_buffer" not in st  # plain SGD allocates (and touches) no buffer
        else:
            moment_close("momentum_buffer")
    else:
        np.testing.assert_allclose(st["exp_avg_sq"].cpu().numpy(), rst["exp_avg_sq"].numpy(), rtol=1e-5)  # (a sum of squares)
        moment_close("exp_avg")


# ---- the protocol shared with FusedRAdam: one representative of each kernel family and template branch
FAMILIES = {
    "adam": ("Adam", dict(weight_decay=1e-2)),
    "adamw": ("AdamW", dict(weight_decay=1e-2)),
    "sgd-plain": ("SGD", dict(weight_decay=1e-2)),
    "sgd-nesterov": ("SGD", dict(momentum=0.9, nesterov=True, weight_decay=1e-2)),
}
N_SMALL = 4 * 256 * 3 + 3  # three workgroups of vectors and a tail


def _make(family, p0, lr=2e-3):
    name, kw = FAMILIES[family]
    p = torch.nn.Parameter(p0.clone().cuda())
    return p, _fused(name)([p], lr=lr, **kw)


def _grads(steps, n, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=g) * (1.0 + k)).cuda() for k in range(steps)]


def _tensors(opt, p):
    st = opt.state[p]
    return {"param": p.detach()} | {k: v for k, v in st.items() if torch.is_tensor(v) and k not in ("coef", "lr_dev")}


def _assert_same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("family", list(FAMILIES))
def test_grad_scale_identity_and_power_of_two(family):
    p0 = torch.randn(N_SMALL, generator=torch.Generator().manual_seed(2))
    grads = _grads(4, N_SMALL)
    (pa, a), (pb, b), (pc, c) = _make(family, p0), _make(family, p0), _make(family, p0)
    for g in grads:
        pa.grad, pb.grad, pc.grad = g.clone(), g.clone(), 4.0 * g
        a.step()
        b.step(grad_scale=1.0)
        c.step(grad_scale=0.25)  # (power-of-two scaling is exact)
    _assert_same_bits(_tensors(a, pa), _tensors(b, pb))
    _assert_same_bits(_tensors(a, pa), _tensors(c, pc))
    assert not torch.equal(pa.detach().cpu(), p0)
    with pytest.raises(RuntimeError, match="grad_scale"):
        a.step(grad_scale=1.5)


def _adds(dsts, srcs, counts):
    k = len(dsts)
    return ((ctypes.c_void_p * k)(*[t.data_ptr() for t in srcs]), (ctypes.c_void_p * k)(*[t.data_ptr() for t in dsts]),
            (ctypes.c_float * k)(*counts), k)


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_scalar_adds_ride_in_the_step(family, staged):
    from spcl_amd.stepgraph import StepStage
    p0 = torch.randn(N_SMALL, generator=torch.Generator().manual_seed(3))
    p, opt = _make(family, p0)
    q, plain = _make(family, p0)
    srcs = [torch.tensor([v], device="cuda") for v in (0.25, -1.5, 3.0)]
    dsts = [torch.tensor([s, c], device="cuda") for s, c in ((1.5, 2.0), (0.0, 0.0), (-8.0, 5.0))]
    counts = [3.0, 1.0, 2.0]
    want = [[float(d[0]) + cn * float(s), float(d[1]) + cn] for d, s, cn in zip(dsts, srcs, counts)]
    g = _grads(1, N_SMALL)[0]
    p.grad, q.grad = g.clone(), g.clone()
    stage = StepStage("cuda") if staged else None
    if staged:
        stage.begin({})
    opt.step(scalar_adds=_adds(dsts, srcs, counts), stage=stage)
    if staged:
        stage.end()
    plain.step()
    assert [d.tolist() for d in dsts] == want
    _assert_same_bits(_tensors(opt, p), _tensors(plain, q))  # the adds change nothing of the update
    # a step with no gradient still performs the adds (and nothing else)
    before = p.detach().clone()
    p.grad = None
    opt.step(scalar_adds=_adds(dsts, srcs, counts))
    want2 = [[w[0] + cn * float(s), w[1] + cn] for w, s, cn in zip(want, srcs, counts)]
    assert [d.tolist() for d in dsts] == want2
    assert torch.equal(p.detach(), before) and int(opt.state[p]["step"]) == 1
    # a destination named twice is refused, by name
    p.grad = g.clone()
    with pytest.raises(RuntimeError, match="twice"):
        opt.step(scalar_adds=_adds([dsts[0], dsts[0]], srcs[:2], counts[:2]))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_staged_steps_equal_eager_steps(family):
    """six steps whose four floats come from the host (``stage=``: adam_coefficients / sgd_coefficients through the stage's
    upload, no coefficient launch) against six eager steps: the same bits, the device counter follows"""
    from spcl_amd.stepgraph import StepStage
    p0 = torch.randn(N_SMALL, generator=torch.Generator().manual_seed(4))
    grads = _grads(7, N_SMALL)
    (pe, eager), (ps, staged) = _make(family, p0), _make(family, p0)
    stage = StepStage("cuda")
    for k, g in enumerate(grads[:6]):
        if k == 4:
            for o in (eager, staged):
                o.param_groups[0]["lr"] = 5e-4
        pe.grad, ps.grad = g.clone(), g.clone()
        eager.step()
        stage.begin({})
        staged.step(stage=stage)
        stage.end()
    _assert_same_bits(_tensors(eager, pe), _tensors(staged, ps))
    assert int(staged.state[ps]["step"]) == 6 and staged._step_host[id(ps)] == 6
    # the host mirror dropped: the next staged step reads the device's counter back
    staged.forget_staged_steps()
    assert not staged._step_host
    pe.grad, ps.grad = grads[6].clone(), grads[6].clone()
    eager.step()
    stage.begin({})
    staged.step(stage=stage)
    stage.end()
    assert staged._step_host[id(ps)] == 7 and int(staged.state[ps]["step"]) == 7
    _assert_same_bits(_tensors(eager, pe), _tensors(staged, ps))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_state_dict_round_trip(family):
    p0 = torch.randn(N_SMALL, generator=torch.Generator().manual_seed(6))
    grads = _grads(4, N_SMALL)
    pa, a = _make(family, p0)
    for g in grads[:3]:
        pa.grad = g.clone()
        a.step()
    blob = io.BytesIO()
    torch.save(a.state_dict(), blob)
    blob.seek(0)
    pb, b = _make(family, pa.detach().cpu())
    b.load_state_dict(torch.load(blob, map_location="cpu"))
    st = b.state[pb]
    assert st["step"].dtype == torch.int64 and st["step"].is_cuda and int(st["step"]) == 3
    name, kw = FAMILIES[family]
    keys = {"step", "lr_dev", "lr_host", "coef"} | ({"exp_avg", "exp_avg_sq"} if name != "SGD" else
                                                     ({"momentum_buffer"} if kw.get("momentum") else set()))
    assert set(st) == keys == set(a.state[pa])
    for k in keys - {"step", "lr_host"}:
        assert st[k].dtype == torch.float32 and st[k].is_cuda, k
    pa.grad, pb.grad = grads[3].clone(), grads[3].clone()
    a.step()
    b.step()
    _assert_same_bits(_tensors(a, pa), _tensors(b, pb))


def test_entry_points_refuse_bad_arguments():
    from spcl_amd import native as n
    p = torch.zeros(16, device="cuda")
    g, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    step = torch.zeros((), dtype=torch.int64, device="cuda")
    lr, coef = torch.full((), 1e-3, device="cuda"), torch.zeros(4, device="cuda")

    def adam(**o):
        a = dict(p=n.ptr(p), g=n.ptr(g), gs=1.0, m=n.ptr(m), v=n.ptr(v), n=16, b1=0.9, k=0)
        a.update(o)
        n.call("spcl_adam_step_scaled", a["p"], a["g"], a["gs"], a["m"], a["v"], a["n"], n.ptr(step), n.ptr(lr), a["b1"], 0.999,
               1e-8, 0.0, 0, n.ptr(coef), a["k"], None, None, None, n.stream())

    def sgd(**o):
        a = dict(buf=None, mom=0.0, damp=0.0, nest=0, p=n.ptr(p))
        a.update(o)
        n.call("spcl_sgd_step_scaled", a["p"], n.ptr(g), 1.0, a["buf"], 16, n.ptr(step), n.ptr(lr), a["mom"], a["damp"], 0.0,
               a["nest"], n.ptr(coef), 0, None, None, None, n.stream())

    for bad, word in ((dict(p=None), "null"), (dict(n=0), "empty"), (dict(gs=0.0), "grad_scale"), (dict(b1=1.0), "betas"),
                      (dict(k=9), "scalar adds"), (dict(p=ctypes.c_void_p(p.data_ptr() + 4)), "aligned")):
        with pytest.raises(RuntimeError, match=word):
            adam(**bad)
    for bad, word in ((dict(p=None), "null"), (dict(mom=0.9), "momentum_buffer"), (dict(buf=n.ptr(m)), "momentum_buffer"),
                      (dict(mom=-0.5), "momentum"), (dict(nest=1), "Nesterov"),
                      (dict(nest=1, mom=0.9, damp=0.1, buf=n.ptr(m)), "Nesterov")):
        with pytest.raises(RuntimeError, match=word):
            sgd(**bad)
    torch.cuda.synchronize()
    assert int(step) == 0 and not p.any()  # a refused call launches nothing


# ---- the epochers' step through the hipGraph (the recipe of tests/test_gpu_step_graph.py::_setup)
def _pretrain_setup(graph, make_opt):
    import spcl_amd  # noqa
    from spcl_amd import ddp
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.epochers import PretrainEncoderEpocher
    from spcl_amd.semi_seg.hooks import create_sp_infonce_hooks
    torch.manual_seed(3)
    net = UNet(input_dim=1, num_classes=4, max_channel=128).cuda()
    net.set_compute_dtype(torch.float32)
    hook = create_sp_infonce_hooks(model=net, feature_names="Conv5", weights=1.0, contrast_ons="partition", begin_values=9.0,
                                   end_values=9.0, mode="soft", max_epoch=10, p=0.5, correct_grad=True, data_name="acdc",
                                   sync_checks=False).cuda()
    for name in net.decoder_names:
        getattr(net, "_" + name).requires_grad_(False)
    flat = ddp.FlatParams([p for p in net.parameters() if p.requires_grad] + list(hook.parameters()))
    opt = make_opt(flat.param)
    ep = PretrainEncoderEpocher(model=net, optimizer=opt, chain_dataloader=iter([]), num_batches=100, device="cuda",
                                inference_until="Conv5", flat_params=flat, graph=graph)
    ep.add_hooks([hook()])
    net.train()
    return net, flat, opt, ep


@pytest.mark.parametrize("which", ["adam", "sgd-nesterov"])
def test_pretrain_graphed_steps_equal_eager_steps(which):
    """the step counter and SGD's first-step branch live on the device: seven steps, five of them replays of ONE capture
    (taken at step 3), equal seven eager steps bit for bit"""
    from spcl_amd.optim import FusedAdam, FusedSGD
    from tests.test_gpu_step_graph import _batches, _run
    make = {"adam": lambda p: FusedAdam([p], lr=2e-3, weight_decay=1e-5),
            "sgd-nesterov": lambda p: FusedSGD([p], lr=2e-3, momentum=0.9, nesterov=True, weight_decay=1e-5)}[which]
    steps, bs = 7, 12
    res = {}
    for graph in (False, True):
        net, flat, opt, ep = _pretrain_setup(graph, make)
        assert flat.fold_mean is True
        curve = _run(ep, _batches(steps, bs, 32))
        sg = ep._step_graph
        if graph:
            assert sg is not None and sg.captured and not sg.failed and sg.replays == steps - 2, (sg.replays,)
        else:
            assert sg is None
        res[graph] = (curve, flat.data.clone(), {k: v.clone() for k, v in net.state_dict().items()},
                      int(opt.state[flat.param]["step"]), ep.meters.statistics())
    assert res[False][0] == res[True][0], (res[False][0], res[True][0])
    assert len(set(res[False][0])) == steps
    assert torch.equal(res[False][1], res[True][1])
    for k, v in res[False][2].items():
        assert torch.equal(v, res[True][2][k]), k
    assert res[False][3] == res[True][3] == steps
    a, b = res[False][4]["semi"]["reg_loss"]["mean"], res[True][4]["semi"]["reg_loss"]["mean"]
    np.testing.assert_allclose(a, b, rtol=1e-6)  # (the meter's add rode in the optimizer's launch, eager and replayed)


def test_finetune_graphed_steps_equal_eager_steps_with_adamw():
    from spcl_amd import ddp
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.optim import FusedAdamW
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.epochers import FineTuneEpocher
    steps, bs, size = 7, 6, 32
    g = torch.Generator().manual_seed(8)
    batches = []
    for k in range(steps):
        img = torch.rand(bs, 1, size, size, generator=g).cuda()
        tgt = torch.randint(0, 4, (bs, 1, size, size), generator=g).cuda()
        groups = [f"patient{(i + k) % 3:03d}_00" for i in range(bs)]
        batches.append(((img, img, tgt, tgt), [f"f{i}" for i in range(bs)], (["0"] * bs, groups)))
    res = {}
    for graph in (False, True):
        torch.manual_seed(4)
        net = UNet(input_dim=1, num_classes=4, max_channel=128).cuda()
        flat = ddp.FlatParams([p for p in net.parameters() if p.requires_grad])
        opt = FusedAdamW([flat.param], lr=1e-3, weight_decay=1e-2)
        ep = FineTuneEpocher(model=net, optimizer=opt, labeled_loader=iter([]), sup_criterion=KL_div(), num_batches=steps,
                             device="cuda", flat_params=flat, graph=graph)
        net.train()
        curve = []
        with ep.meters.focus_on(ep.meter_focus):
            for b in batches:
                curve.append(float(ep.step(b).detach()))
        sg = ep._step_graph
        if graph:
            assert sg is not None and sg.captured and not sg.failed and sg.replays == steps - 2
        else:
            assert sg is None
        res[graph] = (curve, flat.data.clone(), {k: v.clone() for k, v in net.state_dict().items()},
                      int(opt.state[flat.param]["step"]), ep.meters.statistics()["semi"])
    assert res[False][0] == res[True][0]
    assert len(set(res[False][0])) == steps
    assert torch.equal(res[False][1], res[True][1])
    for k, v in res[False][2].items():
        assert torch.equal(v, res[True][2][k]), k
    assert res[False][3] == res[True][3] == steps
    assert res[False][4]["sup_dice"] == res[True][4]["sup_dice"]
    np.testing.assert_allclose(res[False][4]["sup_loss"]["mean"], res[True][4]["sup_loss"]["mean"], rtol=1e-6)


# ---- wiring
def test_build_optimizer_returns_the_fused_classes_on_the_gpu():
    from spcl_amd import ddp, optim
    from spcl_amd.semi_seg.trainers.pretrain import build_optimizer
    flat = ddp.FlatParams([torch.nn.Parameter(torch.zeros(40, device="cuda"))])
    cfg = {"lr": 1e-5, "weight_decay": 1e-5}
    for name, cls in (("Adam", optim.FusedAdam), ("AdamW", optim.FusedAdamW), ("SGD", optim.FusedSGD),
                      ("RAdam", optim.FusedRAdam)):
        opt = build_optimizer(name, flat.param, dict(cfg))
        assert type(opt) is cls and optim.is_fused(opt)
        assert opt.defaults["lr"] == 1e-5 and opt.defaults["weight_decay"] == 1e-5
    assert build_optimizer("AdamW", flat.param, {"lr": 1e-5}).defaults["weight_decay"] == 1e-2  # torch's AdamW default
    assert build_optimizer("Adam", flat.param, dict(cfg, amsgrad=False, foreach=None)).defaults["lr"] == 1e-5
    opt = build_optimizer("SGD", flat.param, dict(cfg, momentum=0.9, nesterov=True))
    assert type(opt) is optim.FusedSGD and opt.defaults["nesterov"] is True
    # what the fused steps do not implement falls back to torch.optim, as does every other name
    for name, extra in (("Adam", {"amsgrad": True}), ("AdamW", {"maximize": True}), ("SGD", {"foreach": True}),
                        ("Adagrad", {})):
        opt = build_optimizer(name, flat.param, dict(cfg, **extra))
        assert type(opt) is getattr(torch.optim, name) and not optim.is_fused(opt)


def test_semi_trainer_from_an_adamw_config(tmp_path):
    from spcl_amd import optim
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.trainers.semi import SemiTrainer
    from tests.test_gpu_semi_step import _batch
    cfg = {"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 2}, "EntropyMinParameters": {"weight": 0.5},
           "Optim": {"name": "AdamW", "lr": 1e-5, "weight_decay": 1e-5}}
    lab = [_batch(2, 64, 30 + k) for k in range(3)]
    unl = [_batch(2, 64, 40 + k) for k in range(3)]
    torch.manual_seed(9)
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    tr = SemiTrainer(model=model, labeled_loader=lab, unlabeled_loader=unl, val_loader=[], test_loader=None,
                     criterion=KL_div(), save_dir=str(tmp_path), max_epoch=2, num_batches=3, device="cuda", config=cfg)
    tr.register_hooks(*create_hook_from_config(model, cfg))
    tr.init()
    assert type(tr._optimizer) is optim.FusedAdamW
    assert tr._optimizer.defaults["lr"] == 1e-5 and tr._optimizer.defaults["weight_decay"] == 1e-5
    before = tr._flat.data.clone()
    random.seed(5)
    stats = tr._create_tra_epoch().run()
    assert tr._flat.fold_mean is True
    assert int(tr._optimizer.state[tr._flat.param]["step"]) == 3
    assert not torch.equal(tr._flat.data, before) and bool(torch.isfinite(tr._flat.data).all())
    flat = str(stats)
    assert "sup_loss" in flat and "reg_loss" in flat
