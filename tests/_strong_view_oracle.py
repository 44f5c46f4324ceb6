"""numpy restatement of the strong intensity view (include/spcl_hip.h, csrc/strong_view.hip).

The table's draws in float32 with the kernel's three roundings (difference, product, sum; the scaling by 2^-24 and the min
with ``hi`` are exact): bit-equal.  The mean, the image pipeline and the blur in float64; the flip; the integer noise."""
import numpy as np

COLS = 16
NEUTRAL = (1.0, 1.0, 1.0, 0.0, 0.0)
SQRT3_F32 = np.float32(1.7320508075688772)
M32 = np.uint64(0xFFFFFFFF)


def key(i, seed):
    """``pxs_key``: fmix32(((i + 1) * 0x9E3779B1 mod 2^32) ^ seed), element-wise on uint32 values held in uint64"""
    i = np.asarray(i, dtype=np.uint64)
    h = (((i + np.uint64(1)) * np.uint64(0x9E3779B1)) & M32) ^ np.uint64(int(seed) & 0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def draws(seed, N, p16, lo, hi):
    """-> (values float32 [N, 5], mask int64 [N], noise seed words uint32 [N])"""
    n = np.arange(N, dtype=np.uint64)
    r = np.stack([key(np.uint64(16) * n + np.uint64(j), seed) for j in range(11)], axis=1)  # [N, 11]
    values = np.empty((N, 5), dtype=np.float32)
    mask = np.zeros(N, dtype=np.int64)
    for k in range(5):
        on = (r[:, 2 * k] & np.uint64(0xFFFF)) < np.uint64(p16[k])
        f = (r[:, 2 * k + 1] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)  # (24 bits: exact)
        lo_k, hi_k = np.float32(lo[k]), np.float32(hi[k])
        d = np.float32(hi_k - lo_k)
        v = np.minimum(hi_k, (lo_k + (d * f).astype(np.float32)).astype(np.float32))
        values[:, k] = np.where(on, v, np.float32(NEUTRAL[k]))
        mask |= on.astype(np.int64) << k
    return values, mask, r[:, 10].astype(np.uint32)


def mean64(x):
    """the float64 mean of every sample of ``x`` [N, C, H, W]"""
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(x.shape[0], -1).mean(axis=1)


def table(x, seed, p16, lo, hi):
    """-> float32 [N, 16], the kernel's table with the mean rounded to float32 from the float64 mean"""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    values, mask, nseed = draws(seed, N, p16, lo, hi)
    t = np.zeros((N, COLS), dtype=np.float32)
    t[:, :5] = values
    t[:, 5] = mask.astype(np.float32)
    t[:, 6] = nseed.view(np.float32)
    t[:, 7] = mean64(x).astype(np.float32)
    t[:, 8] = np.array([bin(int(m)).count("1") for m in mask], dtype=np.float32)
    return t


def neutral_table(N, m=0.0):
    t = np.zeros((N, COLS), dtype=np.float32)
    t[:, :5] = np.array(NEUTRAL, dtype=np.float32)
    t[:, 7] = m
    return t


def flip(x, flags):
    """sample n flipped along H (bit 0 of flags[n]) and along W (bit 1)"""
    out = np.array(x, copy=True)
    for n, f in enumerate(flags):
        v = out[n]
        if int(f) & 1:
            v = v[:, ::-1, :]
        if int(f) & 2:
            v = v[:, :, ::-1]
        out[n] = v
    return out


def noise_z(nseed, C, H, W):
    """the Irwin-Hall integers of one sample, int64 [C, H, W]: four 16-bit uniforms minus 131070"""
    q = np.arange(C * H * W, dtype=np.uint64)
    k0, k1 = key(np.uint64(2) * q, nseed), key(np.uint64(2) * q + np.uint64(1), nseed)
    z = (k0 & np.uint64(0xFFFF)) + (k0 >> np.uint64(16)) + (k1 & np.uint64(0xFFFF)) + (k1 >> np.uint64(16))
    return (z.astype(np.int64) - 131070).reshape(C, H, W)


def binomial(a):
    """[1 4 6 4 1] / 16 along W then along H of [C, H, W] with replicated edges"""
    H, W = a.shape[1:]
    p = np.pad(a, ((0, 0), (0, 0), (2, 2)), mode="edge")
    a = ((p[:, :, 0:W] + p[:, :, 4:W + 4]) + 4.0 * (p[:, :, 1:W + 1] + p[:, :, 3:W + 3]) + 6.0 * p[:, :, 2:W + 2]) / 16.0
    p = np.pad(a, ((0, 0), (2, 2), (0, 0)), mode="edge")
    return ((p[:, 0:H] + p[:, 4:H + 4]) + 4.0 * (p[:, 1:H + 1] + p[:, 3:H + 3]) + 6.0 * p[:, 2:H + 2]) / 16.0


def apply(x, flags, t):
    """the float64 pipeline on the stored values ``x`` [N, C, H, W] under the float32 table ``t`` -> (pre, out): the values
    before the last clamp and after it.  An all-neutral row is a pure copy (pre == out == the flipped sample)."""
    x = flip(np.asarray(x, dtype=np.float64), flags)
    N, C, H, W = x.shape
    pre = np.empty_like(x)
    out = np.empty_like(x)
    for n in range(N):
        g, c, b, tt, s = (float(v) for v in t[n, :5])
        m = float(t[n, 7])
        if (g, c, b, tt, s) == NEUTRAL:
            pre[n] = out[n] = x[n]
            continue
        a = np.clip(x[n], 0.0, 1.0)
        if g != 1.0:
            a = np.power(a, g)
        a = ((a - m) * c + m) * b
        if tt != 0.0:
            a = a + tt * (binomial(a) - a)
        if s != 0.0:
            nseed = int(t[n, 6:7].view(np.uint32)[0])
            a = a + (s * float(SQRT3_F32)) * (noise_z(nseed, C, H, W).astype(np.float64) * 2.0 ** -16)
        pre[n] = a
        out[n] = np.clip(a, 0.0, 1.0)
    return pre, out
