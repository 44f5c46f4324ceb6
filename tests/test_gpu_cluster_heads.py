"""GPU: the cluster heads' normalise / temperature kernel (csrc/projector.hip ``spcl_group_l2norm_temp_*``,
functional.group_l2norm_temp) and ``ClusterHead`` / ``DenseClusterHead`` at ``linear | mlp`` x ``normalize`` x ``T`` against the
float64 restatements of tests/_iic_estimator_oracle.py.

Bars.  Kernel: relative L2 1e-6 forward, 1e-5 backward (three f32 roundings put it near 2e-7).  Heads: forward 1e-5, gradients
of the feature and of every parameter 2e-5 relative L2, the bar of tests/test_gpu_decoder.py.  The linear / unnormalised /
T = 1 logits must be bit-equal to what the two launches the heads issued before (``functional.projector`` /
``functional.pixelwise_mlp`` on the stacked weights) return, restated here."""
import pytest
import torch

from tests import _iic_estimator_oracle as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ the kernel
def _kernel_case(shape, ld, S, K):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(*shape, ld, generator=g)
    x[..., 1, K:2 * K] = 0.0  # one all-zero group
    dz = torch.randn(*shape, ld, generator=g)
    return x, dz


@pytest.mark.parametrize("shape,ld", [((7,), 15), ((7,), 16), ((2, 9, 11), 15), ((2, 9, 11), 20)],
                         ids=["rows", "rows_pitch16", "map", "map_pitch20"])
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalized"])
@pytest.mark.parametrize("T", [1.0, 0.5])
def test_group_l2norm_temp_vs_float64(shape, ld, normalize, T):
    from spcl_amd import functional as F_hip
    S, K = 3, 5
    x, dz = _kernel_case(shape, ld, S, K)
    xin = x if len(shape) == 1 else x.permute(0, 3, 1, 2)  # a map is logical [N, ld, H, W] over channels-last storage
    xg = xin.to(DEV).requires_grad_(True)
    z = F_hip.group_l2norm_temp(xg, num_subheads=S, num_clusters=K, normalize=normalize, T=T)
    if not normalize and T == 1.0:
        assert z is xg  # nothing to do: no launch
        return
    zs = z if len(shape) == 1 else z.permute(0, 2, 3, 1)
    zs.backward(dz.to(DEV))
    torch.cuda.synchronize()
    x64 = x.double().requires_grad_(True)
    ref = E.group_l2norm_temp(x64, S, K, normalize, T)
    ref.backward(dz.double()[..., :S * K])
    gx = (xg.grad if len(shape) == 1 else xg.grad.permute(0, 2, 3, 1)).cpu()
    zs = zs.detach().cpu()
    zero = torch.zeros(x.shape[:-1], dtype=torch.bool)
    zero[..., 1] = True
    ef = _rel_l2(zs[..., :S * K], ref.detach())
    eb = _rel_l2(gx[..., :S * K][~zero], x64.grad[..., :S * K][~zero])
    ez = _rel_l2(gx[..., K:2 * K][zero], x64.grad[..., K:2 * K][zero])
    print(f"forward {ef:.2e}, backward {eb:.2e}, backward of the all-zero group {ez:.2e}")
    assert ef <= 1e-6 and eb <= 1e-5 and ez <= 1e-5, (ef, eb, ez)
    assert bool((zs[..., K:2 * K][zero] == 0).all()) and bool(torch.isfinite(gx).all())
    if ld > S * K:  # the columns no subhead owns: zeros out, zero gradient
        assert bool((zs[..., S * K:] == 0).all()) and bool((gx[..., S * K:] == 0).all())


def test_group_l2norm_temp_refuses_bad_arguments():
    from spcl_amd import functional as F_hip
    x = torch.zeros(4, 14, device=DEV)
    with pytest.raises(RuntimeError, match="ld = 14"):
        F_hip.group_l2norm_temp(x, num_subheads=3, num_clusters=5, normalize=True)
    with pytest.raises(RuntimeError, match="temperature"):
        F_hip.group_l2norm_temp(x, num_subheads=2, num_clusters=5, normalize=True, T=0.0)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.group_l2norm_temp(x.cpu(), num_subheads=2, num_clusters=5, normalize=True)


# ------------------------------------------------------------------------------------------------ the heads
S, K, C = 3, 5, 16


def _head(dense, head_type, normalize, T, seed=11):
    from spcl_amd.contrastyou.projectors.heads import ClusterHead, DenseClusterHead
    torch.manual_seed(seed)
    cls = DenseClusterHead if dense else ClusterHead
    return cls(input_dim=C, num_clusters=K, num_subheads=S, head_type=head_type, T=T, normalize=normalize)


def _feature():
    return torch.randn(4, C, 6, 5, generator=torch.Generator().manual_seed(12))


@pytest.mark.parametrize("dense", [False, True], ids=["ClusterHead", "DenseClusterHead"])
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalized"])
@pytest.mark.parametrize("T", [1.0, 0.5])
@pytest.mark.parametrize("head_type", ["linear", "mlp"])
def test_heads_vs_float64(dense, head_type, normalize, T):
    head = _head(dense, head_type, normalize, T)
    layers = [0 if dense else 2] + ([2 if dense else 4] if head_type == "mlp" else [])
    assert list(head.state_dict()) == [f"_headers.{s}.{i}.{n}" for s in range(S) for i in layers for n in ("weight", "bias")]
    sd64 = {k: v.double().requires_grad_(True) for k, v in head.state_dict().items()}
    feat = _feature()
    f64 = feat.double().requires_grad_(True)
    oracle = E.dense_cluster_head_logits if dense else E.cluster_head_logits
    ref = oracle(f64, sd64, S, head_type, normalize, T)
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    ref.backward(g)
    head.to(DEV)
    fg = feat.to(DEV).requires_grad_(True)
    lg = head.logits(fg)
    assert tuple(lg.shape) == ((4, S * K, 6, 5) if dense else (4, S * K, 1, 1))
    lg.backward(g.float().to(DEV).view(lg.shape))
    probs = head(fg.detach())
    torch.cuda.synchronize()
    ef = _rel_l2(lg.detach().reshape(ref.shape), ref.detach())
    ex = _rel_l2(fg.grad, f64.grad)
    print(f"logits {ef:.2e}, d feature {ex:.2e}")
    assert ef <= 1e-5 and ex <= 2e-5, (ef, ex)
    for k, p in head.named_parameters():
        e = _rel_l2(p.grad, sd64[k].grad)
        print(f"  d {k} {e:.2e}")
        assert e <= 2e-5, (k, e)
    assert len(probs) == S
    for s, p in enumerate(probs):
        want = ref.detach()[:, s * K:(s + 1) * K].softmax(1)
        assert _rel_l2(p.reshape(want.shape), want) <= 1e-5, s


@pytest.mark.parametrize("dense,subheads", [(False, 3), (False, 4), (True, 4)],
                         ids=["ClusterHead_15", "ClusterHead_20", "DenseClusterHead_20"])
def test_plain_linear_logits_keep_their_bits(dense, subheads):
    """linear / unnormalised / T = 1: the product over the stacked weights, as the heads issued it before normalisation and
    temperature were served -- restated here on the head's own parameters"""
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.projectors.heads import ClusterHead, DenseClusterHead
    torch.manual_seed(3)
    head = (DenseClusterHead if dense else ClusterHead)(input_dim=C, num_clusters=K, num_subheads=subheads, head_type="linear",
                                                        T=1, normalize=False).to(DEV)
    feat = _feature().to(DEV)
    idx = 0 if dense else 2
    w = torch.cat([h[idx].weight for h in head._headers], 0)
    b = torch.cat([h[idx].bias for h in head._headers], 0)
    with torch.no_grad():
        if dense:
            want = F_hip.pixelwise_mlp(feat, w, b)
        else:
            out = F_hip.projector(feat, w, b, None, None, False)
            want = out.view(out.shape[0], out.shape[1], 1, 1)
        got = head.logits(feat)
    assert got.shape == want.shape and torch.equal(got, want)



# ------------------------------------------------------------------------------------------------ the recorded reference
import os  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_iic_estimator.npz")


def test_heads_vs_the_references_recorded_probabilities():
    """every head case of tests/golden/g15_iic_estimator.npz (the reference's own ``ClusterHead`` / ``DenseClusterHead`` in
    float32): state-dict keys, the S probability maps and the feature gradient at the bars above"""
    from spcl_amd.contrastyou.projectors.heads import ClusterHead, DenseClusterHead
    heads, _, z = E.load_golden(GOLDEN)
    assert len(heads) == 16
    for key in heads:
        dense, ht, nz, T = E.parse_case(key)
        head = (DenseClusterHead if dense else ClusterHead)(input_dim=C, num_clusters=K, num_subheads=S, head_type=ht, T=T,
                                                            normalize=nz)
        assert list(head.state_dict()) == z[key + "/keys"], key
        head.load_state_dict(E.golden_state(z, key), strict=True)
        head.to(DEV)
        x = z[key + "/feat"].to(DEV).requires_grad_(True)
        probs = torch.stack(head(x), 0)
        want = z[key + "/probs"]
        (probs.reshape(want.shape) * z[key + "/up"].to(DEV)).sum().backward()
        ef, ex = _rel_l2(probs.detach().reshape(want.shape), want), _rel_l2(x.grad, z[key + "/dfeat"])
        print(f"{key}: probabilities {ef:.2e}, d feature {ex:.2e}")
        assert ef <= 1e-5 and ex <= 2e-5, (key, ef, ex)
