"""float64 restatement of the weighted supervised-contrastive criterion (SupConLoss2 / 3 / 4), written from its formula.

Over the 2n rows of z = cat(z1, z2), s_ij = z_i . z_j / t, a non-negative pair-weight matrix P[2n,2n] and a 0/1
denominator-enable matrix E[2n,2n], both with the diagonal forced to 0:

    D_i = sum_j E_ij exp(s_ij)        W_i = sum_j P_ij
    out mode: loss = -mean_i [ sum_j P_ij (s_ij - log D_i) / W_i ]
    in  mode: loss = -mean_i [ log( sum_j P_ij exp(s_ij) / D_i ) / W_i ]

and the five ways the three classes build (P, E).  Used by the CPU and the GPU tests; torch float64 throughout, so autograd
of ``criterion`` is the gradient reference."""
import torch

F64 = torch.float64


def _tile(m):
    return m.to(F64).repeat(2, 2)


def pe_target(target):
    """SupConLoss2(target=): P = [target_i == target_j] tiled 2 x 2, E = 1"""
    t = torch.as_tensor(target).to(F64)
    P = _tile((t[:, None] == t[None, :]))
    return P, torch.ones_like(P)


def pe_simclr(n):
    """SupConLoss2 without argument: P = eye(n) tiled 2 x 2, E = 1"""
    P = _tile(torch.eye(n))
    return P, torch.ones_like(P)


def pe_mask(mask):
    """SupConLoss2(mask=): P = [mask == 1], E = [mask == 0 or mask == 1], both tiled 2 x 2"""
    m = _tile(mask)
    P = (m == 1).to(F64)
    return P, ((m == 0) | (m == 1)).to(F64)


def pe_pos_weight(pos_weight):
    """SupConLoss3(pos_weight=): P = pos_weight tiled 2 x 2, E = 1"""
    P = _tile(pos_weight)
    return P, torch.ones_like(P)


def pe_blocks(n, one2one_weight=None, two2two_weight=None, one2two_weight=None):
    """SupConLoss4: block (1,1) = one2one_weight, installed only when one2two_weight is given; block (2,2) =
    two2two_weight; blocks (1,2) and (2,1) both = one2two_weight, not transposed; E = 1 exactly on the installed blocks"""
    P = torch.zeros(2 * n, 2 * n, dtype=F64)
    E = torch.zeros_like(P)
    if one2two_weight is not None:
        P[:n, :n] = one2one_weight.to(F64)
        P[:n, n:] = one2two_weight.to(F64)
        P[n:, :n] = one2two_weight.to(F64)
        E[:n, :n] = E[:n, n:] = E[n:, :n] = 1
    if two2two_weight is not None:
        P[n:, n:] = two2two_weight.to(F64)
        E[n:, n:] = 1
    return P, E


def logits(z1, z2, t):
    z = torch.cat([z1, z2]).to(F64)
    return z @ z.t() / t


def criterion(z1, z2, P, E, t=0.07, out_mode=True):
    """the loss (0-dim float64, differentiable in z1 / z2); P, E before the diagonal is removed"""
    s = logits(z1, z2, t)
    off = 1 - torch.eye(s.shape[0], dtype=F64)
    P, E = P.to(F64) * off, E.to(F64) * off
    l = s - s.max(dim=1, keepdim=True).values.detach()  # (a per-row constant: it cancels in both forms)
    x = torch.exp(l)
    D, W = (E * x).sum(1), P.sum(1)
    if out_mode:
        return -((P * l).sum(1) / W - torch.log(D)).mean()
    return -(torch.log((P * x).sum(1) / D) / W).mean()


def loss_and_grads(z1, z2, P, E, t=0.07, out_mode=True):
    a = z1.detach().to(F64).requires_grad_(True)
    b = z2.detach().to(F64).requires_grad_(True)
    loss = criterion(a, b, P, E, t, out_mode)
    ga, gb = torch.autograd.grad(loss, (a, b))
    return loss.detach(), ga, gb


def taps(z1, z2, t=0.07):
    """(sim_exp, sim_logits) as the classes store them: S / t - max(S / t) over the whole matrix, and its exponential"""
    s = logits(z1, z2, t)
    sl = s - s.max()
    return torch.exp(sl), sl


# ---- seeded inputs shared by the golden generator and the tests
SOURCES = ("target", "simclr", "mask", "pos_weight", "blocks3", "blocks_no22")


def unit_rows(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g, dtype=F64), dim=1).float()


def make_inputs(n, d, seed=0):
    """z1, z2 (unit rows, float32) and one input of every kind: target [n]; a mask over {0, 0.5, 1} in which every row
    keeps at least one 1 off the diagonal; four random non-symmetric weight matrices in (0.05, 1)"""
    g = torch.Generator().manual_seed(1000 + seed)
    inp = {"z1": unit_rows(n, d, 2 * seed + 11), "z2": unit_rows(n, d, 2 * seed + 12)}
    inp["target"] = (torch.arange(n) % max(2, n // 3 + 1))[torch.randperm(n, generator=g)].float()  # every class present
    mask = torch.randint(0, 3, (n, n), generator=g).float() / 2
    for i in range(n):  # a 1 off the diagonal of the tiled matrix: column (i + 1) mod n (for n = 1 the pair (i, i + n))
        mask[i, (i + 1) % n] = 1.0
    inp["mask"] = mask
    for k in ("pos_weight", "w11", "w22", "w12"):
        inp[k] = (0.05 + 0.95 * torch.rand(n, n, generator=g)).float()
    return inp


def pe_of(source, inp):
    n = inp["z1"].shape[0]
    if source == "target":
        return pe_target(inp["target"])
    if source == "simclr":
        return pe_simclr(n)
    if source == "mask":
        return pe_mask(inp["mask"])
    if source == "pos_weight":
        return pe_pos_weight(inp["pos_weight"])
    if source == "blocks3":
        return pe_blocks(n, inp["w11"], inp["w22"], inp["w12"])
    if source == "blocks_no22":
        return pe_blocks(n, inp["w11"], None, inp["w12"])
    raise KeyError(source)


def call_of(source, inp, module, out_mode, **ctor):
    """the class call of ``module`` (a ``contrast_loss`` module: the mirror's or the reference's) for one source -> loss"""
    z1, z2 = inp["z1_arg"], inp["z2_arg"]
    if source in ("target", "simclr", "mask"):
        crit = module.SupConLoss2(out_mode=out_mode, **ctor)
        kw = {"target": {"target": inp["target"]}, "simclr": {}, "mask": {"mask": inp["mask"]}}[source]
        return crit, crit(z1, z2, **kw)
    if source == "pos_weight":
        crit = module.SupConLoss3(out_mode=out_mode, **ctor)
        return crit, crit(z1, z2, pos_weight=inp["pos_weight"])
    crit = module.SupConLoss4(out_mode=out_mode, **ctor)
    return crit, crit(proj_feat1=z1, proj_feat2=z2, one2one_weight=inp["w11"],
                      two2two_weight=inp["w22"] if source == "blocks3" else None, one2two_weight=inp["w12"])
