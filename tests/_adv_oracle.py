"""Restatement of the adversarial baseline in torch.nn.functional on the CPU, in any floating dtype (float64: the reference
of the GPU tests; float32: the yardstick of their tolerance): the layers of the DCGAN discriminator one by one, the whole
network as an ``nn.Sequential``, and one adversarial step given the segmentation logits."""
import torch
import torch.nn.functional as F
from torch import nn

SLOPE = 0.2


def rel_l2(a, ref):
    a, ref = a.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((a - ref).norm() / ref.norm().clamp_min(1e-300))


def bound(f32_value, ref64):
    """the tolerance of a comparison that goes through a product or a long sum: 4 x the relative L2 error torch's own float32
    CPU evaluation of the same expression makes on the same inputs (the margin covers another summation order), at least 1e-6"""
    return max(4.0 * rel_l2(f32_value, ref64), 1e-6)


def transform(x, mode, scale=None, shift=None):
    """the input transform of a layer on a [N, C, H, W] map: 0 identity, 1 LeakyReLU(0.2), 2 LeakyReLU(0.2)(scale x + shift)"""
    if mode == 0:
        return x
    if mode == 2:
        x = x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    return F.leaky_relu(x, SLOPE)


def patch_rows(u):
    """[N, C, H, W] -> [N Ho Wo, 16 C] rows of the 4 x 4, stride 2, padding 1 windows, k = 16 c + 4 kh + kw (unfold's order);
    the padding is zero AFTER whatever produced ``u``"""
    cols = F.unfold(u, kernel_size=4, stride=2, padding=1)  # [N, 16 C, L]
    return cols.transpose(1, 2).reshape(-1, cols.shape[1])


def conv4s2(u, w):
    return F.conv2d(u, w, stride=2, padding=1)


def batch_norm(x, gamma, beta, running_mean=None, running_var=None, training=True, momentum=0.1, eps=1e-5):
    return F.batch_norm(x, running_mean, running_var, gamma, beta, training, momentum, eps)


def head_logits(u, w):
    """Conv2d(C, 1, 4, 1, 0) of the activated map ``u``"""
    return F.conv2d(u, w)


def softplus_bce(t, y):
    """BCE(sigmoid(t), y) for the constant y: softplus(-t) for 1, softplus(t) for 0; the mean"""
    z = -t if y else t
    return (z.clamp_min(0) + torch.log1p(torch.exp(-z.abs()))).mean()


def bce(d, y):
    return F.binary_cross_entropy(d, torch.full_like(d, float(y)))


def discriminator(input_dim, hidden_dim, dtype=torch.float64):
    h = hidden_dim
    net = nn.Sequential(
        nn.Conv2d(input_dim, h, 4, 2, 1, bias=False), nn.LeakyReLU(SLOPE),
        nn.Conv2d(h, 2 * h, 4, 2, 1, bias=False), nn.BatchNorm2d(2 * h), nn.LeakyReLU(SLOPE),
        nn.Conv2d(2 * h, 4 * h, 4, 2, 1, bias=False), nn.BatchNorm2d(4 * h), nn.LeakyReLU(SLOPE),
        nn.Conv2d(4 * h, 8 * h, 4, 2, 1, bias=False), nn.BatchNorm2d(8 * h), nn.LeakyReLU(SLOPE),
        nn.Conv2d(8 * h, 1, 4, 1, 0, bias=False), nn.Sigmoid())
    return net.to(dtype)


def load_into(net, state):
    """the HIP module's state_dict (keys ``_main.<i>.<name>``) into an ``nn.Sequential`` of this file"""
    net.load_state_dict({k.split(".", 1)[1]: v.detach().cpu().to(net[0].weight.dtype) if v.is_floating_point() else v.cpu()
                         for k, v in state.items()}, strict=True)
    return net


def adversarial_step(net, labeled_logits, unlabeled_logits, labeled_image, unlabeled_image, reg_weight, consider_image):
    """one iteration of the adversarial scheme from the segmentation logits on (float64 leaves): ``net`` in train mode sees
    the unlabelled class map (generator term, target 1), then the detached labelled (target 1) and unlabelled (target 0)
    maps.  Returns gen_loss, dis_loss, the gradient of ``reg_weight * gen_loss`` w.r.t. the unlabelled logits and the
    discriminator's gradients of ``reg_weight * dis_loss`` alone."""
    def inp(logits, image):
        p = logits.softmax(1)
        return torch.cat([image, p], 1) if consider_image else p

    ul = unlabeled_logits.detach().clone().requires_grad_(True)
    gen = bce(net(inp(ul, unlabeled_image)), 1.0)
    (reg_weight * gen).backward()
    net.zero_grad()
    dis = bce(net(inp(labeled_logits.detach(), labeled_image)), 1.0) + bce(net(inp(unlabeled_logits.detach(), unlabeled_image)), 0.0)
    (reg_weight * dis).backward()
    return gen.detach(), dis.detach(), ul.grad, {k: p.grad.clone() for k, p in net.named_parameters()}

