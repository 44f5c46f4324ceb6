"""GPU: the UDA-IIC hooks on real tapped UNet features (fp32 storage) against float64 restatements: each discrete-MI hook's
loss and its cluster head's parameter gradients, and the consistency hook's loss and logit gradient."""
import pytest
import torch

from tests import _iic_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("paddings", [[0, 0], [1, 3]])
def test_discrete_mi_hooks_vs_float64(paddings):
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.arch import UNet
    torch.manual_seed(3)
    n = 2
    model = UNet(input_dim=1, num_classes=4, max_channel=128).to(DEV).train().set_compute_dtype(torch.float32)
    cfg = {"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 2},
           "DiscreteMIConsistencyParams": {"feature_names": ["Conv5", "Up_conv3", "Up_conv2"], "mi_weights": [0.1, 0.05, 0.05],
                                           "dense_paddings": paddings, "consistency_weight": 1}}
    hook = create_hook_from_config(model, cfg)[0]
    hook.to(DEV)
    mi_hooks = hook._hooks[0]._hooks
    img = torch.rand(2 * n, 1, 48, 48, device=DEV)
    flags = torch.tensor([1, 2], dtype=torch.uint8, device=DEV)
    ehooks = [h() for h in mi_hooks]
    from spcl_amd.contrastyou.meters import MeterInterface
    meters = MeterInterface(default_focus="semi")
    for eh in ehooks:
        eh.meters = meters
        eh.configure_meters(meters)
        eh.before_forward_pass()
    model(img)
    for eh in ehooks:
        eh.after_forward_pass()
    for th, eh in zip(mi_hooks, ehooks):
        feat = eh._extractor.feature()[-2 * n:].detach()
        loss = eh(unlabeled_image=img[:n], unlabeled_image_tf=img[n:], affine_transformer=None, seed=0, flip_flags=flags)
        params = list(th._projector.parameters())
        grads = torch.autograd.grad(loss, params)
        torch.cuda.synchronize()
        # float64: heads of the reference (pool + Linear / 1x1 conv, softmax), criteria of the reference
        f64 = feat.double().cpu()
        p64 = [p.detach().double().cpu().requires_grad_(True) for p in params]
        S = len(th._projector._headers)
        terms = []
        for s in range(S):
            w, b = p64[2 * s], p64[2 * s + 1]
            if th._feature_name == "Conv5":
                z = f64.mean(dim=(2, 3)) @ w.t() + b
                pa, pb = z[:n].softmax(1), z[n:].softmax(1)
                terms.append(R.iid_loss(pa, pb)[0])
            else:
                z = torch.nn.functional.conv2d(f64, w, b)
                pa, pb = R.flip(z[:n], [1, 2]).softmax(1), z[n:].softmax(1)
                terms.append(R.iid_segmentation_loss(pa, pb, th._criterion.padding))
        ref = sum(terms) / S * th._weight
        gref = torch.autograd.grad(ref, p64)
        assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref)) + 1e-9, (th._hook_name, float(loss), float(ref))
        for g, r in zip(grads, gref):
            assert _rel_l2(g, r) <= 1e-4, (th._hook_name, _rel_l2(g, r))
    for eh in ehooks:
        eh.close()


def test_consistency_hook_vs_float64():
    from spcl_amd.semi_seg.hooks import create_consistency_hook
    from spcl_amd.contrastyou.meters import MeterInterface
    th = create_consistency_hook(weight=1.0)
    eh = th()
    meters = MeterInterface(default_focus="semi")
    eh.meters = meters
    eh.configure_meters(meters)
    g = torch.Generator().manual_seed(1)
    a = torch.randn(3, 4, 20, 24, generator=g)
    b = torch.randn(3, 4, 20, 24, generator=g)
    flags = [3, 0, 1]
    bd = b.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ad = a.to(DEV).contiguous(memory_format=torch.channels_last)
    loss = eh(unlabeled_tf_logits=bd, unlabeled_logits_tf=None, seed=0, affine_transformer=None, unlabeled_logits=ad,
              flip_flags=torch.tensor(flags, dtype=torch.uint8, device=DEV))
    loss.backward()
    b64 = b.double().requires_grad_(True)
    ref = R.consistency(a.double(), b64, 1.0, flags)
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * float(ref)
    assert _rel_l2(bd.grad, b64.grad) <= 1e-5
