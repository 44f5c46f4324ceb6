"""GPU: SupConLoss2 / 3 / 4 (contrastyou/losses/contrast_loss.py on csrc/supcon_weighted.hip) against the reference's recorded
results, against float64 autograd of the (P, E) restatement (tests/_weighted_supcon_oracle.py) and against the existing
kernels where they compute the same thing.  Bars, those tests/test_gpu_loss.py holds supcon.hip to: loss rtol 1e-4 /
atol 1e-5, gradients rtol 1e-3 / atol 1e-5."""
import numpy as np
import pytest
import torch

from tests import _weighted_supcon_oracle as O

pytestmark = pytest.mark.gpu

# n, d: single pair | odd d | 2n = 62, just under the one-workgroup limit | 2n = 64, the boundary | first shape on the row
# kernels | d just above one tile | row kernels, vector loads | large
SHAPES = [(1, 4), (3, 5), (31, 128), (32, 128), (33, 128), (70, 257), (300, 64), (1024, 128)]
GOLDEN_SHAPES = [(3, 5), (6, 32), (33, 128)]


def _mirror():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses import contrast_loss
    return contrast_loss


def _cuda(inp):
    return {k: v.cuda() for k, v in inp.items()}


def _run(source, dev_inp, out_mode, **ctor):
    """-> (criterion, loss, dz1, dz2) of the mirror on fresh leaves"""
    a = dev_inp["z1"].clone().requires_grad_(True)
    b = dev_inp["z2"].clone().requires_grad_(True)
    crit, loss = O.call_of(source, dict(dev_inp, z1_arg=a, z2_arg=b), _mirror(), out_mode, **ctor)
    loss.backward()
    return crit, loss.detach(), a.grad, b.grad


def _close(got, want, rtol, what):
    g, w = got.detach().double().cpu().numpy(), np.asarray(want, dtype=np.float64)
    print(f"{what}: max |diff| {np.abs(g - w).max():.3e} (max |want| {np.abs(w).max():.3e})")
    np.testing.assert_allclose(g, w, rtol=rtol, atol=1e-5, err_msg=what)


@pytest.mark.parametrize("out_mode", [True, False], ids=["out", "in"])
@pytest.mark.parametrize("n,d", SHAPES)
def test_loss_and_gradients_match_float64_autograd(n, d, out_mode):
    inp = O.make_inputs(n, d)
    dev = _cuda(inp)
    for source in O.SOURCES:
        want = O.loss_and_grads(inp["z1"], inp["z2"], *O.pe_of(source, inp), out_mode=out_mode)
        _, loss, dz1, dz2 = _run(source, dev, out_mode)
        what = f"n{n}_d{d}/{source}/{'out' if out_mode else 'in'}"
        _close(loss, want[0], 1e-4, what + " loss")
        _close(dz1, want[1], 1e-3, what + " dz1")
        _close(dz2, want[2], 1e-3, what + " dz2")


def test_single_pair_closed_forms():
    """n = 1: out mode is 0 (to the loss bar); in mode is -mean_i(log(w_i) / w_i)"""
    inp = O.make_inputs(1, 4)
    dev = _cuda(inp)
    _close(_run("blocks3", dev, True)[1], 0.0, 1e-4, "n = 1, out mode")
    w = inp["w12"].double().reshape(())
    _close(_run("blocks3", dev, False)[1], float(-torch.log(w) / w), 1e-4, "n = 1, in mode")


@pytest.mark.parametrize("n,d", GOLDEN_SHAPES)
def test_loss_and_gradients_match_the_reference(golden, n, d):
    g = golden("g11_weighted_supcon.npz")
    dev = {k: torch.tensor(g[f"n{n}_d{d}/{k}"]).cuda() for k in ("z1", "z2", "target", "mask", "pos_weight", "w11", "w22", "w12")}
    for source in O.SOURCES:
        for out_mode in (True, False):
            key = f"n{n}_d{d}/{source}/{'out' if out_mode else 'in'}"
            _, loss, dz1, dz2 = _run(source, dev, out_mode)
            _close(loss, g[key + "/loss"], 1e-4, key + " loss")
            _close(dz1, g[key + "/dz1"], 1e-3, key + " dz1")
            _close(dz2, g[key + "/dz2"], 1e-3, key + " dz2")


@pytest.mark.parametrize("n,d", [(30, 128), (300, 128)])
def test_out_mode_equals_suploss1_of_the_existing_kernels(n, d):
    """an independent second implementation of what semi_seg/epochers/legacy.py computes: same bars"""
    from spcl_amd.contrastyou.losses.contrast_loss3 import SupConLoss1
    dev = _cuda(O.make_inputs(n, d))
    for source, kw in (("target", {"target": dev["target"]}), ("simclr", {})):
        a = dev["z1"].clone().requires_grad_(True)
        b = dev["z2"].clone().requires_grad_(True)
        want = SupConLoss1()(a, b, **kw)
        want.backward()
        _, loss, dz1, dz2 = _run(source, dev, True)
        _close(loss, want.detach().cpu(), 1e-4, f"n{n} {source} loss")
        _close(dz1, a.grad.cpu(), 1e-3, f"n{n} {source} dz1")
        _close(dz2, b.grad.cpu(), 1e-3, f"n{n} {source} dz2")


@pytest.mark.parametrize("n,d", [(6, 32), (40, 64)])
def test_same_pairs_give_the_same_bits_through_every_class(n, d):
    """SupConLoss3 with a 0/1 weight == SupConLoss2 with that mask; SupConLoss4 with one matrix in all three slots ==
    SupConLoss3: the same kernel on the same (P, E)"""
    M = _mirror()
    dev = _cuda(O.make_inputs(n, d))
    hard = (dev["mask"] == 1).float()
    for out_mode in (True, False):
        res = []
        for make in (lambda a, b: M.SupConLoss2(out_mode=out_mode)(a, b, mask=hard),
                     lambda a, b: M.SupConLoss3(out_mode=out_mode)(a, b, pos_weight=hard),
                     lambda a, b: M.SupConLoss3(out_mode=out_mode)(a, b, pos_weight=dev["pos_weight"]),
                     lambda a, b: M.SupConLoss4(out_mode=out_mode)(proj_feat1=a, proj_feat2=b, one2one_weight=dev["pos_weight"],
                                                                   two2two_weight=dev["pos_weight"],
                                                                   one2two_weight=dev["pos_weight"])):
            a = dev["z1"].clone().requires_grad_(True)
            b = dev["z2"].clone().requires_grad_(True)
            loss = make(a, b)
            loss.backward()
            res.append((loss.detach(), a.grad, b.grad))
        for x, y in ((res[0], res[1]), (res[2], res[3])):
            assert all(torch.equal(p, q) for p, q in zip(x, y))


@pytest.mark.parametrize("n,d", [(6, 32), (40, 64)])
def test_nan_contract(n, d):
    M = _mirror()
    dev = _cuda(O.make_inputs(n, d))
    w = dev["pos_weight"].clone()
    w[2, :] = 0  # rows 2 and n + 2 of the pair matrix have no positive weight
    with pytest.raises(RuntimeError):
        M.SupConLoss3()(dev["z1"], dev["z2"], pos_weight=w)
    crit = M.SupConLoss3(sync_checks=False)
    loss = crit(dev["z1"], dev["z2"], pos_weight=w)  # nothing raises, nothing is read back
    assert loss.is_cuda
    with pytest.raises(RuntimeError):
        crit.check()
    crit(dev["z1"], dev["z2"], pos_weight=dev["pos_weight"])
    crit.check()
    # block (1,1) is installed only beside one2two_weight: the rows of view 1 are left without any pair
    with pytest.raises(RuntimeError):
        M.SupConLoss4()(proj_feat1=dev["z1"], proj_feat2=dev["z2"], one2one_weight=w, two2two_weight=dev["w22"])


@pytest.mark.parametrize("n,d", [(6, 32), (40, 64)])
def test_norm_contract(n, d):
    M = _mirror()
    dev = _cuda(O.make_inputs(n, d))
    with pytest.raises(AssertionError, match="need to be normalized"):
        M.SupConLoss2()(2 * dev["z1"], dev["z2"], target=dev["target"])
    with pytest.raises(AssertionError, match="need to be normalized"):
        M.SupConLoss3(out_mode=False)(dev["z1"], 2 * dev["z2"], pos_weight=dev["pos_weight"])


@pytest.mark.parametrize("n,d", [(3, 5), (8, 32)])
def test_taps(n, d):
    """the values the reference stores BEFORE it removes the diagonal"""
    inp = O.make_inputs(n, d)
    dev = _cuda(inp)
    sim_exp, sim_logits = O.taps(inp["z1"], inp["z2"])
    for source in O.SOURCES:
        crit = _run(source, dev, True)[0]
        P, E = O.pe_of(source, inp)
        np.testing.assert_allclose(crit.sim_logits.cpu().double().numpy(), sim_logits.numpy(), rtol=0, atol=2e-5)
        np.testing.assert_allclose(crit.sim_exp.cpu().double().numpy(), sim_exp.numpy(), rtol=1e-4, atol=0)
        if source in ("target", "simclr", "mask"):
            assert torch.equal(crit.pos_mask.cpu().double(), P) and torch.equal(crit.neg_mask.cpu().double(), E - P)
        else:
            assert torch.equal(crit.pos_weight.cpu(), P.float())  # (the weights are float32 inputs: exact)
        if source.startswith("blocks"):
            assert torch.equal(crit.enable_mask.cpu().double(), E)
    se, sl = _mirror().exp_sim_temperature(dev["z1"], dev["z2"], 0.07)
    np.testing.assert_allclose(sl.cpu().double().numpy(), sim_logits.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(se.cpu().double().numpy(), sim_exp.numpy(), rtol=1e-4, atol=0)


@pytest.mark.parametrize("n,d", [(30, 128), (70, 257)])
def test_mechanics(n, d):
    """two runs give identical bits; a non-unit upstream gradient scales dz; the registered unit gradient is the forward's
    block; the weights receive no gradient; stacked halves of one projection give the bits of two separate tensors"""
    from spcl_amd import functional as F_hip
    M = _mirror()
    dev = _cuda(O.make_inputs(n, d))
    for out_mode in (True, False):
        first, again = _run("blocks3", dev, out_mode), _run("blocks3", dev, out_mode)
        assert all(torch.equal(p, q) for p, q in zip(first[1:], again[1:]))

        unit = F_hip.register_unit_gradient(torch.ones((), device="cuda"))
        for grad, factor in ((torch.full((), 0.5, device="cuda"), 0.5), (unit, 1.0)):
            a = dev["z1"].clone().requires_grad_(True)
            b = dev["z2"].clone().requires_grad_(True)
            w = dev["pos_weight"].clone().requires_grad_(True)
            M.SupConLoss3(out_mode=out_mode)(a, b, pos_weight=w).backward(gradient=grad)
            assert w.grad is None
            ref = _run("pos_weight", dev, out_mode)
            assert torch.equal(a.grad, ref[2] * factor) and torch.equal(b.grad, ref[3] * factor)
        del unit

        z = torch.cat([dev["z1"], dev["z2"]]).requires_grad_(True)
        h = z * 1.0
        loss = M.SupConLoss3(out_mode=out_mode)(*torch.chunk(h, 2), pos_weight=dev["pos_weight"])
        assert F_hip.stacked_halves(*torch.chunk(h, 2)) is h
        loss.backward()
        ref = _run("pos_weight", dev, out_mode)
        assert torch.equal(loss.detach(), ref[1]) and torch.equal(z.grad, torch.cat([ref[2], ref[3]]))


def test_captured_forward_and_backward_replays_to_the_eager_bits():
    M = _mirror()
    dev = _cuda(O.make_inputs(30, 128))
    eager = {m: _run("pos_weight", dev, m)[1:] for m in (True, False)}
    a = dev["z1"].clone().requires_grad_(True)
    b = dev["z2"].clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for out_mode in (True, False):
        crit = M.SupConLoss3(out_mode=out_mode)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            loss = crit(a, b, pos_weight=dev["pos_weight"])
            da, db = torch.autograd.grad(loss, (a, b))
        g.replay()
        torch.cuda.synchronize()
        crit.check()  # (a captured call is checked after its replay)
        assert torch.equal(loss.detach(), eager[out_mode][0])
        assert torch.equal(da, eager[out_mode][1]) and torch.equal(db, eager[out_mode][2])
