"""GPU: ``MineEstimator`` as a whole (semi_seg/mi_estimator/mine.py over functional.mine_loss).

f32, the convolutions on the exact-f32 products: one call with backward against the float64 restatement of
tests/_mine_oracle.py at (n, C, H, W) = (1, 16, 5, 7), (3, 16, 5, 7), (2, 32, 14, 14), (3, 8, 9, 6) -- loss, both halves of the
feature gradient, every parameter gradient and the running statistics within ``bound`` (4 x the error of torch's own f32 CPU
evaluation, at least the 2e-5 bar of tests/test_gpu_decoder.py for results that went through a convolution); convolution-bias
gradients exactly zero; ``num_batches_tracked`` up by 2.  Condition, asserted on the oracle: in both passes the gap between the
two largest positive activations of every (sample, channel) is >= 1e-3, four orders above the f32 error of an activation
(~3e-7), so no argmax can differ between the device and the oracle.  The seeds below were chosen so that the condition holds in
train and in eval mode (searched on the CPU, on the oracle alone).
A channel that is nowhere positive: maximum 0, and nothing passes its ReLU -- gradients as the oracle's.
bf16: the loss within the 2 % bar of tests/test_gpu_decoder.py; every gradient of the fused path within rel-L2 3e-2 of the
composition of the existing ops on the same device (that file's bf16 noise floor), 2e-5 in f32.
Eval mode matches the oracle's; a state dict made by the oracle loads with ``strict=True``."""
import copy

import pytest
import torch

from tests import _mine_oracle as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# ((n, C, H, W), seed of the inputs, seed of the state)
CASES = [((1, 16, 5, 7), 301, 401), ((3, 16, 5, 7), 312, 412), ((2, 32, 14, 14), 322, 422), ((3, 8, 9, 6), 334, 434)]
MIN_GAP = 1e-3


@pytest.fixture
def compute():
    """set the compute dtype (and, for f32, the exact-f32 convolution products) for one test"""
    import spcl_amd  # noqa: F401
    from spcl_amd import config, native
    before = config.get_compute_dtype()

    def use(dtype):
        config.set_compute_dtype(dtype)
        native.call("spcl_conv_set_f32_split", 0 if dtype == torch.float32 else 1)
    try:
        yield use
    finally:
        config.set_compute_dtype(before)
        native.call("spcl_conv_set_f32_split", 1)


def _estimator(C, sd0, train=True):
    from spcl_amd.semi_seg.mi_estimator import MineEstimator
    est = MineEstimator(layer_name="Conv5", input_dim=C)
    est.load_state_dict({"_projector." + k: v for k, v in sd0.items()}, strict=True)  # (a state dict made by the oracle)
    return est.to(DEV).train(train)


def _call(est, feat, flags):
    x = feat.to(DEV).requires_grad_(True)
    fl = torch.tensor(flags, dtype=torch.uint8, device=DEV)
    loss = est.from_feature(x, fl)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), x.grad


def _check_against_oracle(est, loss, dfeat, feat, flags, sd0, training):
    n = feat.shape[0] // 2
    r64 = M.run(feat, flags, sd0, torch.float64, training)
    r32 = M.run(feat, flags, sd0, torch.float32, training)
    gap = min(M.top2_gap(r64["taps"]["act_joint"]), M.top2_gap(r64["taps"]["act_marg"]))
    assert gap >= MIN_GAP, gap
    tol = M.bound(r32["loss"], r64["loss"])
    print(f"loss {float(loss):.9g} vs {float(r64['loss']):.9g} (bound {tol:.1e}), smallest top-2 gap {gap:.2e}")
    assert abs(float(loss) - float(r64["loss"])) <= tol * abs(float(r64["loss"]))
    for name, sl in (("feat2 half", slice(0, n)), ("feat1 half", slice(n, 2 * n))):
        err, tol = M.rel_l2(dfeat[sl], r64["dfeat"][sl]), M.bound(r32["dfeat"][sl], r64["dfeat"][sl])
        print(f"d{name}: {err:.2e} (bound {tol:.1e})")
        assert err <= tol, name
    params = dict(est._projector.named_parameters())
    assert sorted(params) == sorted(r64["grads"])
    for k, p in params.items():
        if k in ("0.bias", "3.bias"):
            if training:  # exact zeros, not None: the bias cancels in the batch normalisation
                assert p.grad is not None and bool((p.grad == 0).all()), k
            continue
        assert p.grad is not None, k
        err, tol = M.rel_l2(p.grad, r64["grads"][k]), M.bound(r32["grads"][k], r64["grads"][k])
        print(f"d{k}: {err:.2e} (bound {tol:.1e})")
        assert err <= tol, k
    state = {k[len("_projector."):]: v for k, v in est.state_dict().items()}
    for k, v in r64["state"].items():
        if "running" in k:
            assert M.rel_l2(state[k], v) <= M.bound(r32["state"][k], v), k
        elif "num_batches" in k:
            assert int(state[k]) == int(v) == (2 if training else 0), k


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_whole_call_vs_float64(case, compute):
    compute(torch.float32)
    (n, C, H, W), seed, sseed = case
    feat, flags = M.make_inputs(n, C, H, W, seed)
    sd0 = M.init_state(C, sseed)
    est = _estimator(C, sd0)
    loss, dfeat = _call(est, feat, flags)
    _check_against_oracle(est, loss, dfeat, feat, flags, sd0, True)


def test_eval_mode_vs_float64(compute):
    """running statistics, the convolution biases folded into the BatchNorm shift (constants there: no gradient)"""
    compute(torch.float32)
    (n, C, H, W), seed, sseed = CASES[1]
    feat, flags = M.make_inputs(n, C, H, W, seed)
    sd0 = M.init_state(C, sseed)
    est = _estimator(C, sd0, train=False)
    loss, dfeat = _call(est, feat, flags)
    _check_against_oracle(est, loss, dfeat, feat, flags, sd0, False)


def test_a_channel_that_is_nowhere_positive_passes_no_gradient(compute):
    compute(torch.float32)
    (n, C, H, W), seed, sseed = CASES[1]
    feat, flags = M.make_inputs(n, C, H, W, seed)
    sd0 = M.init_state(C, sseed)
    sd0["4.weight"][0], sd0["4.bias"][0] = 0.0, -1.0  # BatchNorm output -1 everywhere: the ReLU output is 0, the maximum 0
    est = _estimator(C, sd0)
    out = {}
    x = feat.to(DEV).requires_grad_(True)
    loss = est.from_feature(x, torch.tensor(flags, dtype=torch.uint8, device=DEV), out=out)
    loss.backward()
    assert bool((out["maxima"][:, :, 0] == 0).all()) and bool((out["argmax"][:, :, 0] == 0).all())
    assert bool((est._projector[3].weight.grad[0] == 0).all())
    assert float(est._projector[4].weight.grad[0]) == 0.0 and float(est._projector[4].bias.grad[0]) == 0.0
    _check_against_oracle(est, loss.detach(), x.grad, feat, flags, sd0, True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=lambda c: "x".join(map(str, c[0])))
def test_fused_path_vs_the_composition_of_existing_ops(case, dtype, compute):
    compute(dtype)
    (n, C, H, W), seed, sseed = case
    feat, flags = M.make_inputs(n, C, H, W, seed)
    sd0 = M.init_state(C, sseed)
    fused = _estimator(C, sd0)
    composed = copy.deepcopy(fused)
    loss, dfeat = _call(fused, feat, flags)
    x = feat.to(DEV).requires_grad_(True)
    closs = M.composed_on_device(composed, x, torch.tensor(flags, dtype=torch.uint8, device=DEV))
    closs.backward()
    ref = M.run(feat, flags, sd0, torch.float64)
    rel = abs(float(loss) - float(ref["loss"])) / abs(float(ref["loss"]))
    print(f"{dtype}: loss {float(loss):.7g}, composed {float(closs.detach()):.7g}, float64 {float(ref['loss']):.7g} ({rel:.2e})")
    assert rel <= (2e-2 if dtype == torch.bfloat16 else 2e-5)
    tol = 3e-2 if dtype == torch.bfloat16 else 2e-5
    assert M.rel_l2(dfeat, x.grad) <= tol
    for (k, p), q in zip(fused._projector.named_parameters(), composed._projector.parameters()):
        if k in ("0.bias", "3.bias"):
            assert bool((p.grad == 0).all()), k
            continue
        assert M.rel_l2(p.grad, q.grad) <= tol, k
    for (k, v), w in zip(fused.state_dict().items(), composed.state_dict().values()):
        assert torch.equal(v, w), k  # same kernels, same statistics


def test_module_forward_takes_the_two_halves(compute):
    compute(torch.float32)
    (n, C, H, W), seed, sseed = CASES[0]
    feat, _ = M.make_inputs(n, C, H, W, seed)
    sd0 = M.init_state(C, sseed)
    a, b = _estimator(C, sd0), _estimator(C, sd0)
    x = feat.to(DEV)
    assert torch.equal(a(x[n:], x[:n]), b.from_feature(x, None))
    with pytest.raises(ValueError, match="expected"):
        a.from_feature(torch.zeros(2, C + 2, H, W, device=DEV))
