"""GPU: ``IICEstimator`` (semi_seg/mi_estimator/discrete_mi_estimator.py) with linear and mlp heads on an encoder and on a decoder
feature against the float64 restatement (tests/_iic_estimator_oracle.py heads, then tests/_iic_oracle.py ``iid_loss`` or the
patch-wise criterion per subhead), its fused form against ``forward``, and one semi-supervised step with the hooks that
``IICRegParameters`` builds.

Bars.  Loss: 1e-5 relative (the bar of the criteria's own tests), or the float32 oracle's own error ``e32`` where that is
larger.  Gradients of the feature and of the parameters: relative L2 within ``max(2e-5, e32)`` (tests/test_gpu_decoder.py's
bar for the heads' products).  Each test prints ``e32`` next to the figure it bounds."""
import pytest
import torch

from tests import _iic_estimator_oracle as E
from tests import _iic_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, K = 3, 5
FLAGS = [1, 2, 3]


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _estimator(layer, C, normalize, T, pad=1, patch=8, seed=21, head_type="linear"):
    from spcl_amd.semi_seg.mi_estimator.discrete_mi_estimator import IICEstimator
    torch.manual_seed(seed)
    est = IICEstimator()
    est.init_projector(layer_name=layer, input_dim=C, head_type=head_type, num_subhead=S, num_cluster=K, normalize=normalize,
                       temperature=T)
    est.init_criterion(padding=pad, patch_size=patch)
    return est


def _oracle(feature, sd, dense, normalize, T, flags, pad, patch, dtype, S=S, K=K, head_type="linear"):
    """loss and its gradients w.r.t. the feature [2n, ...] and the head's parameters, computed in ``dtype``"""
    f = feature.detach().clone().to(dtype).requires_grad_(True)
    sd = {k[len("_projector."):]: v.detach().clone().to(dtype).requires_grad_(True) for k, v in sd.items()}
    n = f.shape[0] // 2
    if dense:
        lg = E.dense_cluster_head_logits(f, sd, S, head_type, normalize, T)
        loss, _ = E.patch_heads_loss(lg[n:], lg[:n], S, K, pad, patch, flags, 1.0 / S)
    else:
        lg = E.cluster_head_logits(f, sd, S, head_type, normalize, T)
        loss = sum(R.iid_loss(lg[n:, s * K:(s + 1) * K].softmax(1), lg[:n, s * K:(s + 1) * K].softmax(1))[0]
                   for s in range(S)) / S
    loss.backward()
    return loss.detach(), f.grad, {k: v.grad for k, v in sd.items()}


@pytest.mark.parametrize("layer,shape", [("Conv5", (6, 16, 4, 4)), ("Up_conv3", (6, 8, 12, 10))], ids=["encoder", "decoder"])
@pytest.mark.parametrize("normalize,T", [(False, 1.0), (True, 1.0), (True, 0.5)], ids=["plain", "normalized", "normalized_T0.5"])
@pytest.mark.parametrize("head_type", ["linear", "mlp"])
def test_from_feature_vs_float64(layer, shape, head_type, normalize, T):
    dense = layer == "Up_conv3"
    est = _estimator(layer, shape[1], normalize, T, head_type=head_type)
    sd = {k: v.clone() for k, v in est.state_dict().items()}
    feat = torch.randn(*shape, generator=torch.Generator().manual_seed(22))
    l64, gf64, gp64 = _oracle(feat, sd, dense, normalize, T, FLAGS, 1, 8, torch.float64, head_type=head_type)
    l32, gf32, gp32 = _oracle(feat, sd, dense, normalize, T, FLAGS, 1, 8, torch.float32, head_type=head_type)
    e32l = abs(float(l32) - float(l64)) / abs(float(l64))
    e32f = _rel_l2(gf32, gf64)
    est.to(DEV)
    fg = feat.to(DEV).requires_grad_(True)
    loss = est.from_feature(fg, torch.tensor(FLAGS, dtype=torch.uint8, device=DEV))
    loss.backward()
    est.flush_check()
    torch.cuda.synchronize()
    el = abs(float(loss.detach()) - float(l64)) / abs(float(l64))
    ef = _rel_l2(fg.grad, gf64)
    print(f"loss {float(loss.detach()):.9g} vs {float(l64):.9g}: rel {el:.2e} (float32 oracle {e32l:.2e}); "
          f"d feature {ef:.2e} (float32 oracle {e32f:.2e})")
    assert el <= max(1e-5, e32l), (el, e32l)
    assert ef <= max(2e-5, e32f), (ef, e32f)
    for k, p in est._projector.named_parameters():
        e, e32 = _rel_l2(p.grad, gp64[k]), _rel_l2(gp32[k], gp64[k])
        print(f"  d {k} {e:.2e} (float32 oracle {e32:.2e})")
        assert e <= max(2e-5, e32), (k, e, e32)


@pytest.mark.parametrize("layer,shape", [("Conv5", (6, 16, 4, 4)), ("Up_conv3", (6, 8, 12, 10))], ids=["encoder", "decoder"])
def test_fused_form_equals_forward_on_the_flipped_feature(layer, shape):
    est = _estimator(layer, shape[1], True, 0.5, head_type="mlp").to(DEV)
    feat = torch.randn(*shape, generator=torch.Generator().manual_seed(23)).to(DEV)
    n = shape[0] // 2
    fl = torch.tensor(FLAGS, dtype=torch.uint8, device=DEV)
    with torch.no_grad():
        fused = est.from_feature(feat, fl)
        plain = est(feat[n:], R.flip(feat[:n], FLAGS))  # mi_estimator(unlabeled_tf_features, flip(unlabeled_features))
    est.flush_check()
    err = abs(float(fused) - float(plain)) / abs(float(plain))
    print(f"fused {float(fused):.9g}, forward {float(plain):.9g}: rel {err:.2e}")
    assert err <= 1e-6


def test_refusals():
    est = _estimator("Up_conv3", 8, False, 1.0).to(DEV)
    with pytest.raises(ValueError, match="expected"):
        est.from_feature(torch.zeros(5, 8, 4, 4, device=DEV))
    with pytest.raises(ValueError, match="one shape"):
        est(torch.zeros(2, 8, 4, 4, device=DEV), torch.zeros(2, 8, 4, 5, device=DEV))


PARAMS = {"feature_names": ["Conv5", "Up_conv3"], "feature_importance": [1, 3], "weight": 0.1,
          "EncoderParams": {"num_clusters": 20, "num_subheads": 5, "head_types": "linear", "normalize": False,
                            "temperature": 1.0},
          "DecoderParams": {"num_clusters": 20, "num_subheads": 5, "head_types": "linear", "normalize": True,
                            "temperature": 0.5},
          "LossParams": {"paddings": [1], "patch_sizes": 1024}, "enforce_matching": False}


def _step(seed=1234, n=2):
    from tests.test_gpu_semi_reg_hooks import _setup
    from tests.test_gpu_semi_step import _batch
    torch.manual_seed(77)
    sd, model, hook, ep, flat = _setup("IICRegParameters", PARAMS)
    members = list(hook._hooks)
    before = [{k: v.detach().cpu().clone() for k, v in h._estimator.state_dict().items()} for h in members]
    lab, unl = _batch(n, 64, 1), _batch(n, 64, 2)
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(lab, unl, seed=seed)
    torch.cuda.synchronize()
    return model, hook, ep, flat, members, before, sup, reg


def test_semi_step_with_the_hooks_of_IICRegParameters():
    from oracle import spcl_oracle as O
    from spcl_amd.semi_seg.hooks import feature_until_from_hooks
    seed, n = 1234, 2
    model, hook, ep, flat, members, before, sup, reg = _step(seed, n)
    assert feature_until_from_hooks(hook) == "Up_conv3"
    assert [h._hook_name for h in members] == ["iic/conv5", "iic/up_conv3"]
    weights = [0.1 * 1 / 4, 0.1 * 3 / 4]
    assert [h._weight for h in members] == pytest.approx(weights, rel=1e-12)
    est_params = [p for h in members for p in h._estimator.parameters()]
    inside = {id(p) for p in flat.params}
    assert est_params and all(id(p) in inside for p in est_params)
    views = {id(p): v for p, v in zip(flat.params, flat.views)}
    flags = [int(d[0]) | (int(d[1]) << 1) for d in O.random_flip_decisions(seed, n)]
    stats, total = ep.meters.statistics(), 0.0
    for h, w, sd0 in zip(members, weights, before):
        est = h._estimator
        feat = h._extractor.feature()[-2 * n:].detach().cpu()
        dense = not est.is_encoder
        args = (dense, est._normalize, est._t, flags, 1, 1024)
        sk = {"S": est._num_subhead, "K": est._num_clusters}
        l64, _, _ = _oracle(feat, sd0, *args, torch.float64, **sk)
        l32, _, _ = _oracle(feat, sd0, *args, torch.float32, **sk)
        e32 = abs(float(l32) - float(l64)) / abs(float(l64))
        got = stats[h._hook_name]["mi"]["mean"]
        err = abs(got + float(l64)) / abs(float(l64))
        print(f"{h._hook_name}: mi {got:.9g} vs {-float(l64):.9g}: rel {err:.2e} (float32 oracle {e32:.2e})")
        assert err <= max(1e-5, e32), (h._hook_name, got, -float(l64))
        total += w * -got
        for k, p in est.named_parameters():
            g = views[id(p)]
            assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
    print(f"reg_loss {float(reg.detach()):.9g} vs {total:.9g}")
    assert abs(float(reg.detach()) - total) <= 1e-6 * abs(total)  # reg = sum_i w_i loss_i and mi_i = -loss_i
    assert bool(torch.isfinite(sup))
    ep.close_hooks()


def test_a_second_identical_step_gives_the_same_bits():
    a = _step()
    b = _step()
    assert torch.equal(a[7].detach(), b[7].detach()) and torch.equal(a[6].detach(), b[6].detach())
    assert torch.equal(a[3].param.detach(), b[3].param.detach())
    sa, sb = a[2].meters.statistics(), b[2].meters.statistics()
    for h in a[4]:
        assert sa[h._hook_name]["mi"]["mean"] == sb[h._hook_name]["mi"]["mean"]
    a[2].close_hooks()
    b[2].close_hooks()


def test_forward_vs_the_references_recorded_losses():
    """every estimator case of tests/golden/g15_iic_estimator.npz: ``forward(feat_tf, flip(feat))`` of the reference's own
    ``IICEstimator`` in float32.  The fixture's loss lies ``eg`` from the float64 restatement (its own float32 error, measured
    here from the fixture), the kernels within ``max(1e-5, e32)``: the two may differ by the sum."""
    import os
    from spcl_amd.semi_seg.mi_estimator.discrete_mi_estimator import IICEstimator
    _, ests, z = E.load_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_iic_estimator.npz"))
    assert len(ests) == 8
    for key in ests:
        layer, ht, nz, T = E.parse_case(key)
        flags = [int(f) for f in z[key + "/flags"]]
        a, b = z[key + "/feat"], z[key + "/feat_tf"]
        sd = E.golden_state(z, key)
        head_sd = {k[len("_projector."):]: v for k, v in sd.items()}
        args = (layer != "Conv5", S, K, ht, nz, T, 1, 8)
        l64 = float(E.estimator_forward(b.double(), R.flip(a, flags).double(), {k: v.double() for k, v in head_sd.items()}, *args))
        l32 = float(E.estimator_forward(b, R.flip(a, flags), head_sd, *args))
        want = float(z[key + "/loss"])
        eg, e32 = abs(want - l64) / abs(l64), abs(l32 - l64) / abs(l64)
        est = IICEstimator()
        est.init_projector(layer_name=layer, input_dim=a.shape[1], head_type=ht, num_subhead=S, num_cluster=K, normalize=nz,
                           temperature=T)
        est.init_criterion(padding=1, patch_size=8)
        assert list(est.state_dict()) == z[key + "/keys"], key
        est.load_state_dict(sd, strict=True)
        est.to(DEV)
        with torch.no_grad():
            got = float(est(b.to(DEV), R.flip(a, flags).to(DEV)))
        est.flush_check()
        err = abs(got - want) / abs(l64)
        print(f"{key}: {got:.9g} vs recorded {want:.9g} (float64 {l64:.9g}): {err:.2e}; recorded vs float64 {eg:.2e}, "
              f"float32 restatement vs float64 {e32:.2e}")
        assert err <= max(1e-5, e32) + eg, (key, got, want)
