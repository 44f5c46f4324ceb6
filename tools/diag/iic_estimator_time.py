"""Time one call of ``IICEstimator`` with its backward on the features of 5 + 5 slices of the 224 x 224 UNet, S = 5 subheads of
K = 20 clusters, linear and mlp heads, two ways on the same device:

* (a) the HIP path: ``IICEstimator.from_feature`` (one product over the stacked subheads, the normalise / temperature launch
  when configured, csrc/iic_patch.hip's joint over the subheads -- or csrc/iic.hip's global joint on ``Conv5``);
* (b) the plain torch formulation of the reference: ``nn`` heads (``DenseClusterHead`` / ``ClusterHead`` as
  contrastyou/projectors/heads.py builds them, softmax included), torch's ``flip`` / ``cat``, then per subhead -- and, for the
  decoder, per patch -- ``F.conv2d`` and the tensor ops of ``IIDSegmentationLoss`` / ``IIDLoss``.

Decoder: ``Up_conv3`` (32 channels, 112 x 112), padding 1, patch sizes 1024 (one patch) and 32 (36 patches), plain and
normalised / T = 0.5 heads.  Encoder: ``Conv5`` (256 channels, 14 x 14).

Every figure is the mean of its repetitions after a warm-up; the measurement is repeated ``--rounds`` times in one process so
that the spread shows.  No pass / fail bar: both sides are recorded.

    python tools/diag/iic_estimator_time.py [--reps 20] [--rounds 3] [--out profiles/iic_estimator_time.txt]"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
DEV = "cuda:0"
N, S, K = 5, 5, 20
FLAGS = [0, 1, 2, 3, 1]


def _time(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _starts(h, patch):
    return list(range(0, h - patch, patch // 2)) + [max(h - patch, 0)]


def _iid_seg(px, py, padding):
    k = px.shape[1]
    p = F.conv2d(px.permute(1, 0, 2, 3), weight=py.permute(1, 0, 2, 3), padding=(padding, padding))
    p = p - p.min().detach() + 1e-16
    T = 2 * padding + 1
    p = p.permute(2, 3, 0, 1)
    p = p / p.sum(dim=3, keepdim=True).sum(dim=2, keepdim=True)
    p = (p + p.permute(0, 1, 3, 2)) / 2.0
    pi = p.sum(dim=2, keepdim=True).repeat(1, 1, k, 1)
    pj = p.sum(dim=3, keepdim=True).repeat(1, 1, 1, k)
    return (-p * (torch.log(p + 1e-16) - torch.log(pi + 1e-16) - torch.log(pj + 1e-16))).sum() / (T * T)


def _iid(x, y):
    k = x.shape[1]
    p = (x.unsqueeze(2) * y.unsqueeze(1)).sum(dim=0)
    p = (p + p.t()) / 2.0
    p = p / p.sum()
    pi = p.sum(dim=1).view(k, 1).expand(k, k)
    pj = p.sum(dim=0).view(1, k).expand(k, k)
    return (-p * (torch.log(p + 1e-10) - torch.log(pj + 1e-10) - torch.log(pi + 1e-10))).sum()


def _flip(x, flags):
    out = []
    for n, f in enumerate(flags):
        v = x[n]
        if f & 1:
            v = v.flip(-2)
        if f & 2:
            v = v.flip(-1)
        out.append(v)
    return torch.stack(out, 0)


class TorchEstimator(nn.Module):
    """the reference's estimator in stock torch modules (heads.py:42-75, discrete_mi_estimator.py:53-65)"""

    def __init__(self, C, dense, head_type, normalize, T, padding, patch):
        super().__init__()
        self.dense, self.normalize, self.T, self.padding, self.patch = dense, normalize, T, padding, patch

        def head():
            if head_type == "linear":
                return nn.Conv2d(C, K, 1) if dense else nn.Linear(C, K)
            if dense:
                return nn.Sequential(nn.Conv2d(C, 64, 1), nn.LeakyReLU(0.01), nn.Conv2d(64, K, 1))
            return nn.Sequential(nn.Linear(C, 128), nn.LeakyReLU(0.01), nn.Linear(128, K))

        self.heads = nn.ModuleList([head() for _ in range(S)])

    def probs(self, x):
        out = []
        for h in self.heads:
            o = h(x) if self.dense else h(x.mean((2, 3)))
            if self.normalize:
                o = F.normalize(o, p=2, dim=1)
            out.append((o / self.T).softmax(1))
        return out

    def forward(self, feat1, feat2):
        losses = []
        for p in self.probs(torch.cat([feat1, feat2], 0)):
            x, y = torch.chunk(p, 2, 0)
            if not self.dense:
                losses.append(_iid(x, y))
                continue
            H, W = x.shape[2:]
            per = [_iid_seg(x[:, :, a:a + self.patch, b:b + self.patch], y[:, :, a:a + self.patch, b:b + self.patch],
                            self.padding) for a in _starts(H, self.patch) for b in _starts(W, self.patch)]
            losses.append(sum(per) / len(per))
        return sum(losses) / len(losses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "iic_estimator_time.txt"))
    args = ap.parse_args()
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.mi_estimator import IICEstimator
    lines = [f"IICEstimator.from_feature + backward vs the reference's torch formulation, {N} + {N} slices, S = {S}, K = {K}, "
             f"f32; ms per call, {args.reps} repetitions, {args.rounds} rounds"]
    print(lines[0])
    shapes = [("Up_conv3", 32, 112, 1, 1024), ("Up_conv3", 32, 112, 1, 32), ("Conv5", 256, 14, 0, 0)]
    cases = [sh + (ht, nz, T) for sh in shapes for ht in ("linear", "mlp") for nz, T in ((False, 1.0), (True, 0.5))]
    fl = torch.tensor(FLAGS, dtype=torch.uint8, device=DEV)
    for layer, C, hw, pad, patch, head_type, normalize, T in cases:
        dense = layer != "Conv5"
        torch.manual_seed(1)
        est = IICEstimator()
        est.init_projector(layer_name=layer, input_dim=C, head_type=head_type, num_subhead=S, num_cluster=K,
                           normalize=normalize, temperature=T)
        est.init_criterion(padding=pad, patch_size=patch)
        est.to(DEV)
        ref = TorchEstimator(C, dense, head_type, normalize, T, pad, patch).to(DEV)
        feat = torch.randn(2 * N, C, hw, hw, device=DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)

        def hip():
            feat.grad = None
            est.zero_grad(set_to_none=True)
            est.from_feature(feat, fl).backward()

        def plain():
            feat.grad = None
            ref.zero_grad(set_to_none=True)
            ref(feat[N:], _flip(feat[:N], FLAGS)).backward()

        for r in range(args.rounds):
            a, b = _time(hip, args.reps), _time(plain, args.reps)
            line = (f"{layer:9s} {hw:3d}^2 C={C:3d} pad={pad} patch={patch:4d} {head_type:6s} normalize={int(normalize)} T={T}: "
                    f"HIP {a:8.3f} ms   torch {b:8.3f} ms   torch/HIP {b / a:6.2f}   (round {r + 1})")
            print(line, flush=True)
            lines.append(line)
        est.flush_check()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
