"""GPU: the MINE baseline's hook (semi_seg/hooks/mine.py behind ``create_mine_hooks`` / ``MineParameters``).

One ``SemiSupervisedEpocher.step`` on the small UNet and synthetic batches of tests/test_gpu_semi_reg_hooks.py with one hook
(Conv5) and with two (Conv5, Up_conv3): ``reg_loss`` and the meter ``mi`` against the float64 restatement of
tests/_mine_oracle.py evaluated on the step's own extracted features and flip flags with the estimators' state from before the
step; the estimators' parameters lie in the trainer's flat parameter, receive a gradient and move with the optimizer step;
their running statistics were updated twice; ``feature_until_from_hooks`` names the deepest feature."""
import pytest
import torch

from oracle import spcl_oracle as O
from tests import _mine_oracle as M
from tests.test_gpu_semi_reg_hooks import _setup
from tests.test_gpu_semi_step import _batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("features,weights", [(["Conv5"], [0.1]), (["Conv5", "Up_conv3"], [0.1, 0.05])],
                         ids=["one_hook", "two_hooks"])
def test_semi_step_with_mine_hooks_vs_float64(features, weights):
    from spcl_amd import native
    from spcl_amd.semi_seg.hooks import feature_until_from_hooks
    native.call("spcl_conv_set_f32_split", 0)
    try:
        _body(features, weights, feature_until_from_hooks)
    finally:
        native.call("spcl_conv_set_f32_split", 1)


def _body(features, weights, feature_until_from_hooks):
    seed, n = 1234, 2
    sd, model, hook, ep, flat = _setup("MineParameters", {"feature_names": features, "weights": weights})
    assert feature_until_from_hooks(hook) == features[-1]
    members = list(hook._hooks)
    assert [h._hook_name for h in members] == [f"mine/{f.lower()}" for f in features]
    est_params = [p for h in members for p in h._estimator.parameters()]
    inside = {id(p) for p in flat.params}
    assert est_params and all(id(p) in inside for p in est_params)
    assert flat.numel == sum(p.numel() for p in model.parameters()) + sum(p.numel() for p in est_params)
    before = [{k: v.detach().cpu().clone() for k, v in h._estimator._projector.state_dict().items()} for h in members]
    lab, unl = _batch(n, 64, 1), _batch(n, 64, 2)
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(lab, unl, seed=seed)
    torch.cuda.synchronize()
    flags = [int(d[0]) | (int(d[1]) << 1) for d in O.random_flip_decisions(seed, n)]
    total, slack, stats = 0.0, 0.0, ep.meters.statistics()
    for h, w, sd0 in zip(members, weights, before):
        feat = h._extractor.feature()[-2 * n:].detach().double().cpu()
        assert feat.shape[1] == model.get_channel_dim(h._feature_name)
        state = M.cast(sd0, torch.float64)
        l64 = float(M.estimator_loss(feat, flags, state))
        l32 = M.estimator_loss(feat.float(), flags, M.cast(sd0, torch.float32))
        tol = M.bound(l32, torch.tensor(l64))
        got = stats[h._hook_name]["mi"]["mean"]
        print(f"{h._hook_name}: mi {got:.9g} vs {-l64:.9g} (bound {tol:.1e})")
        assert abs(got + l64) <= tol * abs(l64), (h._hook_name, got, -l64)
        total += w * l64
        slack += w * tol * abs(l64)
        # the statistics network trained: a gradient for every parameter (zeros for the convolution biases), the
        # optimizer moved the weights, both passes updated the running statistics
        after = h._estimator._projector.state_dict()
        views = {id(p): v for p, v in zip(flat.params, flat.views)}
        for k, p in h._estimator._projector.named_parameters():
            g = views[id(p)]
            if k in ("0.bias", "3.bias"):
                assert bool((g == 0).all()) and torch.equal(p.detach().cpu(), sd0[k]), k
            else:
                assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
                assert not torch.equal(p.detach().cpu(), sd0[k]), k
        for bn in ("1", "4"):
            assert int(after[bn + ".num_batches_tracked"]) == 2
            assert M.rel_l2(after[bn + ".running_mean"], state[bn + ".running_mean"]) <= M.FLOOR_CONV, bn
            assert M.rel_l2(after[bn + ".running_var"], state[bn + ".running_var"]) <= M.FLOOR_CONV, bn
    print(f"reg_loss {float(reg.detach()):.9g} vs {total:.9g}")
    assert abs(float(reg.detach()) - total) <= slack + 1e-6 * abs(total)  # each term within its bound; the f32 products and sum
    assert bool(torch.isfinite(sup))
    ep.close_hooks()
