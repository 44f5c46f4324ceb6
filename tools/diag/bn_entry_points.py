"""Launch plan and output bits of every launching entry point of csrc/bn.hip, one text line per case.

    python tools/diag/bn_entry_points.py --out FILE [--lib path/to/libspcl_hip.so]

Each case seeds its inputs, turns the library's launch recorder on, calls the entry point once and writes: the return code,
the launches (kernel instantiation : bytes : flops, no times) and the sha256 of every output buffer.  Two builds of the library
that lay out their launches the same way and compute the same bits give byte-identical files (C == CS everywhere: no padding
lanes are hashed).  The cases are the smallest that reach every branch of the host layer's dispatch."""
import argparse
import ctypes
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import spcl_amd  # noqa: E402,F401
from spcl_amd import native as n  # noqa: E402

DT = {0: torch.float32, 1: torch.bfloat16}
EVEN, ODD = (2, 6, 10, 32), (1, 5, 7, 16)
LINES = []


def rnd(seed, shape, dtype=torch.float32, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype).cuda()


def out(shape, dtype=torch.float32):
    return torch.full(shape, -7.0, dtype=dtype, device="cuda")


def sha(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()[:20]


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def run(name, fn, args, outs, extra=""):
    """one call under the launch recorder -> one line"""
    L = n.lib()
    n.call("spcl_profile_enable", 1)
    rc = getattr(L, fn)(*args)
    torch.cuda.synchronize()
    launches = []
    for i in range(n.call("spcl_profile_count")):
        buf, us, by, fl = ctypes.create_string_buffer(512), ctypes.c_float(), ctypes.c_double(), ctypes.c_double()
        n.call("spcl_profile_get", i, buf, 512, ctypes.byref(us), ctypes.byref(by), ctypes.byref(fl))
        launches.append(f"{buf.value.decode()}:{by.value:.0f}:{fl.value:.0f}")
    n.call("spcl_profile_enable", 0)
    hashes = " ".join(f"{k}={sha(v)}" for k, v in outs.items() if v is not None)
    LINES.append(f"{name} | {fn} rc={rc} | {' ; '.join(launches)} | {hashes}{extra() if callable(extra) else extra}")


def coef(seed, cs):
    """the forward's [4][CS]: mean, invstd, scale, shift (any values: the two builds must agree on them)"""
    g = torch.Generator().manual_seed(seed)
    mean, invstd = torch.randn(cs, generator=g) * 0.1, torch.rand(cs, generator=g) + 0.5
    gamma, beta = torch.rand(cs, generator=g) + 0.5, torch.randn(cs, generator=g) * 0.3
    return torch.stack([mean, invstd, gamma * invstd, beta - mean * gamma * invstd]).contiguous().cuda()


def block(cs, s1=None, s2=None):
    """an accumulator block (csrc/bn_acc.hpp) holding the sums s1, s2 [cs] in its first replica; zeroed without them"""
    acc = torch.zeros(n.call("spcl_bn_acc_elems", cs), dtype=torch.int64)
    if s1 is not None:
        rows = acc[:acc.numel() - 4].view(-1, cs, 4)
        for k, s in ((0, s1.double().cpu()), (2, s2.double().cpu())):
            hi = torch.round(s * 1024.0)
            rows[0, :, k], rows[0, :, k + 1] = hi.long(), torch.round((s - hi / 1024.0) * 2.0 ** 60).long()
    return acc.cuda()


class FwdBlock:
    """a spcl_bn_acc over the statistics of y, with the buffers its consumer writes"""

    def __init__(self, seed, y, cs):
        yf = y.double().cpu().reshape(-1, cs)
        self.acc = block(cs, yf.sum(0), (yf * yf).sum(0))
        self.gamma, self.beta = rnd(seed + 1, (cs,), shift=1.0, scale=0.2), rnd(seed + 2, (cs,), scale=0.3)
        self.rm, self.rv, self.nbt = out((cs,)), out((cs,)), torch.zeros((), dtype=torch.int64, device="cuda")
        self.st = out((4, cs))
        self.desc = n.BnAcc(self.acc.data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr(), self.rm.data_ptr(),
                            self.rv.data_ptr(), self.nbt.data_ptr(), self.st.data_ptr(), 0.1, 1e-5, float(yf.shape[0]), cs, cs)

    def outs(self):
        return {"st": self.st, "rm": self.rm, "rv": self.rv, "nbt": self.nbt}


def forward_cases():
    for shape in (EVEN, ODD):
        N, H, W, cs = shape
        for dtc in (0, 1):
            dt, tag = DT[dtc], f"{N}x{H}x{W}x{cs}.{'f32 bf16'.split()[dtc]}"
            y, st = rnd(1, shape, dt, 1.2, 0.1), coef(2, cs)
            for mode in ("act", "pool", "both", "ymax+act", "ymax"):
                for blk in (False, True):
                    act = out(shape, dt) if mode in ("act", "both", "ymax+act") else None
                    pool = out((N, H // 2, W // 2, cs), dt) if mode != "act" else None
                    ymax = out((N, H // 2, W // 2, cs), dt) if mode.startswith("ymax") else None
                    b = FwdBlock(3, y, cs) if blk else None
                    bn = ctypes.byref(b.desc) if blk else None
                    outs = {"act": act, "pool": pool, "ymax": ymax, **(b.outs() if blk else {})}
                    name = f"fwd.{mode}.{'block' if blk else 'coef'}.{tag}"
                    if ymax is not None:
                        run(name, "spcl_bnrelu_pool_forward_ymax", (p(y), dtc, N, H, W, cs, p(st[2]), p(st[3]), bn, p(act), p(pool),
                                                                    p(ymax), n.stream()), outs)
                    elif blk:
                        run(name, "spcl_bnrelu_pool_forward_acc", (p(y), dtc, N, H, W, cs, bn, p(act), p(pool), n.stream()), outs)
                    else:
                        run(name, "spcl_bnrelu_pool_forward", (p(y), dtc, N, H, W, cs, p(st[2]), p(st[3]), p(act), p(pool),
                                                               n.stream()), outs)
            wide, pool = out((N, H, W, 2 * cs), dt), out((N, H // 2, W // 2, cs), dt)
            run(f"fwd.strided.{tag}", "spcl_bnrelu_pool_forward_strided",
                (p(y), dtc, N, H, W, cs, p(st[2]), p(st[3]), p(wide[..., cs:]), 2 * cs, p(pool), n.stream()), {"act": wide, "pool": pool})
            run(f"fwd.strided.refused.{tag}", "spcl_bnrelu_pool_forward_strided",
                (p(y), dtc, N, H, W, cs, p(st[2]), p(st[3]), p(wide[..., cs:]), cs - 8, p(pool), n.stream()), {"act": wide})
            up = out((N, 2 * H, 2 * W, cs), dt)
            run(f"fwd.up2.{tag}", "spcl_bnrelu_up2_forward", (p(y), dtc, N, H, W, cs, p(st[2]), p(st[3]), p(up), n.stream()), {"up": up})
    N, H, W, cs = 3, 7, 9, 64
    for dtc in (0, 1):
        y, st = rnd(4, (N, H, W, cs), DT[dtc], 1.2, 0.1), coef(5, cs)
        for blk in (False, True):
            b = FwdBlock(6, y, cs) if blk else None
            act, gap = out((N, H, W, cs), DT[dtc]), out((N, cs))
            run(f"fwd.gap.{'block' if blk else 'coef'}.{dtc}", "spcl_bnrelu_gap_forward",
                (p(y), dtc, N, H, W, cs, cs, p(st[2]), p(st[3]), ctypes.byref(b.desc) if blk else None, p(act), p(gap), n.stream()),
                {"act": act, "gap": gap, **(b.outs() if blk else {})})
    run("fwd.baddtype", "spcl_bnrelu_pool_forward", (p(y), 7, N, H, W, cs, p(st[2]), p(st[3]), p(act), None, n.stream()), {})


class Bwd:
    """the buffers of one backward call on `shape`"""

    def __init__(self, seed, shape, dtc, image=False):
        self.shape, self.dtc, self.dt = shape, dtc, DT[dtc]
        N, H, W, cs = shape
        self.y, self.st = rnd(seed, shape, self.dt, 1.2, 0.1), coef(seed + 1, cs)
        nbytes = n.call("spcl_bnrelu_image_wgrad_workspace_bytes" if image else "spcl_bnrelu_bwd_workspace_bytes", N, H, W, cs)
        self.ws = torch.zeros(nbytes // 4, device="cuda")
        self.dg, self.db, self.dy = out((cs,)), out((cs,)), out(shape, self.dt)
        self.seed = seed

    def grad(self, k, shape, scale=1e-2):
        return rnd(self.seed + 10 + k, shape, self.dt, scale)

    def dims(self):
        N, H, W, cs = self.shape
        return (self.dtc, N, H, W, cs, cs)

    def coefs(self):
        return tuple(p(self.st[k]) for k in range(4))

    def tail(self):  # (ws, dgamma, dbeta) of the workspace forms
        return (p(self.ws), p(self.dg), p(self.db))

    def outs(self, **more):
        return {"dy": self.dy, "dgamma": self.dg, "dbeta": self.db, **more}


def tagof(shape, dtc):
    return "x".join(map(str, shape)) + "." + ("f32", "bf16")[dtc]


def backward_cases():
    for dtc in (0, 1):
        for shape in (EVEN, ODD):
            N, H, W, cs = shape
            tag, half = tagof(shape, dtc), (N, H // 2, W // 2, cs)
            # ---- through the workspace: linear, strided, pooled, at twice the resolution
            b = Bwd(20, shape, dtc)
            run(f"bwd.lin.{tag}", "spcl_bnrelu_pool_backward", (p(b.y), p(b.grad(0, shape)), None, *b.dims(), *b.coefs(), 1, *b.tail(),
                                                                p(b.dy), n.stream()), b.outs())
            b, wide = Bwd(21, shape, dtc), rnd(22, (N, H, W, 2 * cs), DT[dtc], 1e-2)
            run(f"bwd.strided.{tag}", "spcl_bnrelu_pool_backward_strided", (p(b.y), p(wide[..., cs:]), 2 * cs, None, *b.dims(), *b.coefs(),
                                                                            1, *b.tail(), p(b.dy), n.stream()), b.outs())
            b = Bwd(23, shape, dtc)
            run(f"bwd.pool.{tag}", "spcl_bnrelu_pool_backward", (p(b.y), None, p(b.grad(1, half)), *b.dims(), *b.coefs(), 1, *b.tail(),
                                                                 p(b.dy), n.stream()), b.outs())
            b = Bwd(24, shape, dtc)
            run(f"bwd.pool+act.{tag}", "spcl_bnrelu_pool_backward", (p(b.y), p(b.grad(0, shape)), p(b.grad(1, half)), *b.dims(),
                                                                     *b.coefs(), 0, *b.tail(), p(b.dy), n.stream()), b.outs())
            b = Bwd(25, shape, dtc)  # (a strided dact AND a pooled gradient: the general pooled kernel with the stride)
            run(f"bwd.pool+strided.{tag}", "spcl_bnrelu_pool_backward_strided",
                (p(b.y), p(wide[..., cs:]), 2 * cs, p(b.grad(1, half)), *b.dims(), *b.coefs(), 1, *b.tail(), p(b.dy), n.stream()), b.outs())
            b, gs = Bwd(26, shape, dtc), out(shape, DT[dtc])
            run(f"bwd.up2.{tag}", "spcl_bnrelu_backward_up2", (p(b.y), p(b.grad(2, (N, 2 * H, 2 * W, cs))), p(gs), *b.dims(), *b.coefs(), 1,
                                                               *b.tail(), p(b.dy), n.stream()), b.outs(scratch=gs))
            # ---- this call's reduction pass fills the block
            for form in ("lin", "strided", "pool", "pool+act", "up2"):
                b, acc = Bwd(30, shape, dtc), block(cs)
                dact = b.grad(0, shape) if form in ("lin", "pool+act") else wide[..., cs:] if form == "strided" else None
                dpool = b.grad(1, half) if form.startswith("pool") else None
                d_up, gs = (b.grad(2, (N, 2 * H, 2 * W, cs)), out(shape, DT[dtc])) if form == "up2" else (None, None)
                run(f"bwd.fill.{form}.{tag}", "spcl_bnrelu_backward_fill_acc",
                    (p(b.y), p(gs if form == "up2" else dact), 2 * cs if form == "strided" else 0, p(dpool), p(d_up), *b.dims(), p(b.st),
                     1, p(acc), p(b.dg), p(b.db), p(b.dy), n.stream()), b.outs(acc=acc, scratch=gs))
            # ---- the block is already filled
            if H % 2 == 0:
                for form in ("lin", "pool"):
                    b, acc = Bwd(40, shape, dtc), block(cs, rnd(41, (cs,), scale=0.5), rnd(42, (cs,), scale=0.5))
                    dact, dpool = (b.grad(0, shape), None) if form == "lin" else (None, b.grad(1, half))
                    run(f"bwd.filled.{form}.{tag}", "spcl_bnrelu_backward_acc",
                        (p(b.y), p(dact), p(dpool), None, *b.dims(), p(b.st), 1, p(acc), p(b.dg), p(b.db), p(b.dy), n.stream()),
                        b.outs(acc=acc))
            # ---- rows handed in: few (read directly), many (grouped, transposed); into a block
            for nrows in (9, 5000):
                rows = rnd(50 + nrows, (nrows, 2, cs), scale=0.05)
                b = Bwd(51, shape, dtc)
                run(f"bwd.rows{nrows}.lin.{tag}", "spcl_bnrelu_backward_rows",
                    (p(b.y), p(b.grad(0, shape)), None, p(rows), nrows, *b.dims(), *b.coefs(), 1, *b.tail(), p(b.dy), None, n.stream()),
                    b.outs())
                b = Bwd(52, shape, dtc)  # (bf16 only: f32 is refused)
                run(f"bwd.rows{nrows}.pool.{tag}", "spcl_bnrelu_pool_backward_rows",
                    (p(b.y), p(b.grad(1, half)), p(rows), nrows, *b.dims(), *b.coefs(), 1, *b.tail(), p(b.dy), n.stream()), b.outs())
            for nrows in (9, 700):
                rows = rnd(60 + nrows, (nrows, 2, cs), scale=0.05)
                for form in ("lin", "pool") if H % 2 == 0 else ("lin",):
                    b, acc = Bwd(61, shape, dtc), block(cs)
                    dact, dpool = (b.grad(0, shape), None) if form == "lin" else (None, b.grad(1, half))
                    run(f"bwd.rows{nrows}.block.{form}.{tag}", "spcl_bnrelu_backward_rows_acc",
                        (p(b.y), p(dact), p(dpool), p(rows), nrows, *b.dims(), p(b.st), 1, p(acc), p(b.dg), p(b.db), p(b.dy), n.stream()),
                        b.outs(acc=acc))
            # ---- the image block's weight gradient: with and without rows, with and without an armed tail capture
            for with_rows in (False, True):
                for armed in (False, True):
                    b = Bwd(70, shape, dtc, image=True)
                    img, dw, rows = rnd(71, (N, H, W)), out((cs, 9)), rnd(72, (9, 2, cs), scale=0.05)
                    slot = n.WgradTail()
                    if armed:
                        n.call("spcl_wgrad_tail_capture", ctypes.byref(slot))
                    if with_rows:
                        fn, args = "spcl_bnrelu_backward_rows", (p(b.y), p(b.grad(0, shape)), p(img), p(rows), 9, *b.dims(), *b.coefs(), 1,
                                                                 *b.tail(), None, p(dw), n.stream())
                    else:
                        fn, args = "spcl_bnrelu_backward_image_wgrad", (p(b.y), p(b.grad(0, shape)), p(img), *b.dims(), *b.coefs(), 1,
                                                                        *b.tail(), p(dw), n.stream())
                    run(f"bwd.imagewgrad.{'rows' if with_rows else 'reduce'}.{'tail' if armed else 'final'}.{tag}", fn, args,
                        {"dgamma": b.dg, "dbeta": b.db, "dw": dw, "ws": b.ws},
                        (lambda s=slot, ws=b.ws, dw=dw: f" tail=kind{s.kind},nsplit{s.nsplit},{s.nblk_ci},{s.nblk_co},{s.CIB},{s.COB},"
                         f"{s.Cin},{s.Cout},partial@ws+{(s.partial or 0) - ws.data_ptr()},dw{int(s.dw == dw.data_ptr())}")
                        if armed else "")
                    n.call("spcl_wgrad_tail_capture", None)
        # ---- one value per image and channel: 25 -> 4 splits, the 2048-row cap halving the split, one split; through the block
        for shape in ((64, 14, 14, 256), (1100, 4, 4, 256), (3, 7, 9, 64)):
            N, H, W, cs = shape
            b = Bwd(80, shape, dtc)
            run(f"bwd.bcast.{tagof(shape, dtc)}", "spcl_bnrelu_backward_bcast",
                (p(b.y), p(b.grad(3, (N, cs))), *b.dims(), *b.coefs(), 1, *b.tail(), p(b.dy), n.stream()), b.outs())
            b, acc = Bwd(81, shape, dtc), block(cs)
            run(f"bwd.bcast.block.{tagof(shape, dtc)}", "spcl_bnrelu_backward_acc",
                (p(b.y), None, None, p(b.grad(3, (N, cs))), *b.dims(), p(b.st), 1, p(acc), p(b.dg), p(b.db), p(b.dy), n.stream()),
                b.outs(acc=acc))
    # ---- image3: grouped rows, grouped rows with the autocorrelation fold, one row set per workgroup
    N, H, W, cs = 2, 28, 28, 16
    st, w = coef(90, cs), rnd(91, (cs, 9), scale=0.3)
    for name, nrows, nacorr in (("rows700", 700, 8), ("rows1500.fold", 1500, 40), ("wgrows", 300, 16)):
        ws = torch.zeros(n.call("spcl_bnrelu_image3_workspace_bytes", cs) // 4, device="cuda")
        rows = rnd(92, (11, cs, nrows) if name == "wgrows" else (nrows, 11, cs), scale=0.05)
        acorr, dg, db, dw = rnd(93, (nacorr, 64)), out((cs,)), out((cs,)), out((cs, 9))
        run(f"bwd.image3.{name}", "spcl_bnrelu_backward_wgrows_image3" if name == "wgrows" else "spcl_bnrelu_backward_rows_image3",
            (p(rows), nrows, p(acorr), nacorr, p(w), N, H, W, cs, cs, p(st[0]), p(st[1]), p(st[2]), 1, p(ws), p(dg), p(db), p(dw),
             n.stream()), {"dgamma": dg, "dbeta": db, "dw": dw})
    # ---- a streaming case at the grid caps: 2048 workgroups through the workspace, 768 with a block
    shape = (4, 224, 224, 16)
    b = Bwd(95, shape, 1)
    run("bwd.stream.lin", "spcl_bnrelu_pool_backward", (p(b.y), p(b.grad(0, shape)), None, *b.dims(), *b.coefs(), 1, *b.tail(), p(b.dy),
                                                        n.stream()), b.outs())
    b, acc = Bwd(95, shape, 1), block(16)
    run("bwd.stream.fill", "spcl_bnrelu_backward_fill_acc", (p(b.y), p(b.grad(0, shape)), 0, None, None, *b.dims(), p(b.st), 1, p(acc),
                                                             p(b.dg), p(b.db), p(b.dy), n.stream()), b.outs(acc=acc))
    y, acc, act = rnd(96, shape, torch.bfloat16, 1.2, 0.1), None, out(shape, torch.bfloat16)
    fb = FwdBlock(97, y, 16)
    run("fwd.stream.block", "spcl_bnrelu_pool_forward_acc", (p(y), 1, *shape, ctypes.byref(fb.desc), p(act), None, n.stream()),
        {"act": act, **fb.outs()})
    run("fwd.stream.coef", "spcl_bnrelu_pool_forward", (p(y), 1, *shape, p(b.st[2]), p(b.st[3]), p(act), None, n.stream()), {"act": act})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--lib", default=None, help="another build of libspcl_hip.so (same ABI version)")
    a = ap.parse_args()
    if a.lib:
        n.LIB_PATH = os.path.abspath(a.lib)
    forward_cases()
    backward_cases()
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    print(f"{len(LINES)} cases -> {a.out}")


if __name__ == "__main__":
    main()
