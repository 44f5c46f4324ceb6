// The DCGAN discriminator of the adversarial baseline (semi_seg/arch/discr.py:17-36, driven by
// semi_seg/epochers/new_comparable.py:122-200): what the rows product of rows_mlp.hip cannot express.
//   patch rows      Conv2d(C, ., 4, 2, 1, bias=False) as rows[N Ho Wo][16 C] x Wr[Cout][16 C]^T, the previous layer's
//                   LeakyReLU(0.2) / BatchNorm2d + LeakyReLU(0.2) applied on the way in (discr.py:19-32)
//   rows BatchNorm  nn.BatchNorm2d in training mode over an [M][C] map, forward statistics and full backward (discr.py:23,27,31)
//   head            Conv2d(8 hidden, 1, 4, 1, 0) -> Sigmoid -> nn.BCELoss(., constant) (discr.py:34-35, new_comparable.py:124,
//                   162-163, 183-191)
// k order of a patch row (k = 16 c + 4 kh + kw: the [Cout][C][4][4] parameter is the weight matrix as it lies): include/spcl_hip.h.  Every sum has a fixed order; no floating-point atomics.
#include "common.hpp"

namespace spcl {

constexpr float kDiscrLeaky = 0.2f;

__device__ __forceinline__ float dc_leaky(float v) { return v > 0.f ? v : kDiscrLeaky * v; }
__device__ __forceinline__ float dc_slope(float v) { return v > 0.f ? 1.f : kDiscrLeaky; }  // (torch: the slope at 0 is the negative one)

// T of the header: mode 0 identity, 1 LeakyReLU(x), 2 LeakyReLU(scale x + shift)
__device__ __forceinline__ float dc_apply(float v, int mode, float sc, float sh) {
  if (mode == 0) return v;
  if (mode == 2) v = fmaf(sc, v, sh);
  return dc_leaky(v);
}
__device__ __forceinline__ float dc_deriv(float v, int mode, float sc, float sh) {
  if (mode == 0) return 1.f;
  if (mode == 2) v = fmaf(sc, v, sh);
  return dc_slope(v);
}

struct DcMap {  // a strided f32 map of `C` channels
  const float* p;
  int C;
  long sn, sc, sh, sw;
};

// ---- patch rows, any layout: one thread per element of rows (stores coalesced; the loads of a 4- or 5-channel class map hit
// the cache -- every input element is read four times)
__global__ __launch_bounds__(256) void patch_rows_fwd_kernel(DcMap a, DcMap b, int N, int H, int W, int Ho, int Wo, int mode,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             float* __restrict__ rows, long total) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int C = a.C + b.C, K = 16 * C;
  const long m = e / K;
  const int k = (int)(e - m * K), c = k >> 4, kh = (k >> 2) & 3, kw = k & 3;
  const int ow = (int)(m % Wo), oh = (int)((m / Wo) % Ho), n = (int)(m / ((long)Wo * Ho));
  const int ih = 2 * oh - 1 + kh, iw = 2 * ow - 1 + kw;
  float v = 0.f;  // a padded tap is 0, not T(0)
  if (ih >= 0 && ih < H && iw >= 0 && iw < W) {
    const float x = c < a.C ? a.p[n * a.sn + c * a.sc + ih * a.sh + iw * a.sw]
                            : b.p[n * b.sn + (c - a.C) * b.sc + ih * b.sh + iw * b.sw];
    v = dc_apply(x, mode, mode == 2 ? scale[c] : 0.f, mode == 2 ? shift[c] : 0.f);
  }
  rows[e] = v;
}

// ---- patch rows of a dense NHWC map, C % 4 == 0: one thread per four channels of one kernel row -- four 16-byte loads along c
// (kw = 0 .. 3), transposed in registers, four 16-byte stores along kw (one per channel)
__global__ __launch_bounds__(256) void patch_rows_fwd_vec_kernel(const float* __restrict__ x, int N, int H, int W, int C, int Ho,
                                                                 int Wo, int mode, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, float* __restrict__ rows,
                                                                 long total) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;  // ((m, c4), kh), kh fastest
  if (e >= total) return;
  const int cpr = C >> 2, kh = (int)(e & 3);
  const long mc = e >> 2, m = mc / cpr;
  const int c4 = (int)(mc - m * cpr);
  const int ow = (int)(m % Wo), oh = (int)((m / Wo) % Ho), n = (int)(m / ((long)Wo * Ho));
  const int ih = 2 * oh - 1 + kh, iw0 = 2 * ow - 1;
  f32x4 v[4];
#pragma unroll
  for (int kw = 0; kw < 4; ++kw) v[kw] = (f32x4){0.f, 0.f, 0.f, 0.f};  // a padded tap is 0, not T(0)
  if (ih >= 0 && ih < H) {
    f32x4 sc = {0.f, 0.f, 0.f, 0.f}, sh = sc;
    if (mode == 2) {
      sc = *(const f32x4*)(scale + 4 * c4);
      sh = *(const f32x4*)(shift + 4 * c4);
    }
#pragma unroll
    for (int kw = 0; kw < 4; ++kw) {
      const int iw = iw0 + kw;
      if (iw < 0 || iw >= W) continue;
      f32x4 t = *(const f32x4*)(x + (((long)n * H + ih) * W + iw) * C + 4 * c4);
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = dc_apply(t[i], mode, sc[i], sh[i]);
      v[kw] = t;
    }
  }
  float* o = rows + m * 16 * C + (long)(4 * c4) * 16 + 4 * kh;
#pragma unroll
  for (int i = 0; i < 4; ++i) *(f32x4*)(o + 16 * i) = (f32x4){v[0][i], v[1][i], v[2][i], v[3][i]};
}

// the output rows / taps that cover input row (or column) i: tap k0 and k0 + 2, output (i + 1 - k) / 2 when inside [0, no)
__device__ __forceinline__ int dc_cover(int i, int j, int no, int* o) {
  const int k = ((i + 1) & 1) + 2 * j, num = i + 1 - k;
  *o = num >> 1;
  return (num >= 0 && (num >> 1) < no) ? k : -1;
}

// ---- patch rows backward (gather), any channel count: one thread per element of dx [N][H][W][C - c_lo]
__global__ __launch_bounds__(256) void patch_rows_bwd_kernel(const float* __restrict__ drows, const float* __restrict__ x, int N,
                                                             int H, int W, int C, int c_lo, int Ho, int Wo, int mode,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             float* __restrict__ dx, long total) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int Cd = C - c_lo, K = 16 * C;
  const long pix = e / Cd;
  const int c = c_lo + (int)(e - pix * Cd);
  const int iw = (int)(pix % W), ih = (int)((pix / W) % H), n = (int)(pix / ((long)W * H));
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    int oh;
    const int kh = dc_cover(ih, a, Ho, &oh);
    if (kh < 0) continue;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      int ow;
      const int kw = dc_cover(iw, b, Wo, &ow);
      if (kw < 0) continue;
      acc += drows[(((long)n * Ho + oh) * Wo + ow) * K + c * 16 + kh * 4 + kw];
    }
  }
  if (mode != 0) acc *= dc_deriv(x[pix * C + c], mode, mode == 2 ? scale[c] : 0.f, mode == 2 ? shift[c] : 0.f);
  dx[e] = acc;
}

__global__ __launch_bounds__(256) void patch_rows_bwd_vec_kernel(const float* __restrict__ drows, const float* __restrict__ x,
                                                                 int N, int H, int W, int C, int Ho, int Wo, int mode,
                                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                                 float* __restrict__ dx, long total4) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total4) return;
  const int cpr = C >> 2, K = 16 * C;
  const long pix = e / cpr;
  const int c4 = (int)(e - pix * cpr);
  const int iw = (int)(pix % W), ih = (int)((pix / W) % H), n = (int)(pix / ((long)W * H));
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    int oh;
    const int kh = dc_cover(ih, a, Ho, &oh);
    if (kh < 0) continue;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      int ow;
      const int kw = dc_cover(iw, b, Wo, &ow);
      if (kw < 0) continue;
      const float* d = drows + (((long)n * Ho + oh) * Wo + ow) * K + (long)(4 * c4) * 16 + kh * 4 + kw;
      acc += (f32x4){d[0], d[16], d[32], d[48]};
    }
  }
  if (mode != 0) {
    const f32x4 v = *(const f32x4*)(x + pix * C + 4 * c4);
    f32x4 sc = {0.f, 0.f, 0.f, 0.f}, sh = sc;
    if (mode == 2) {
      sc = *(const f32x4*)(scale + 4 * c4);
      sh = *(const f32x4*)(shift + 4 * c4);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] *= dc_deriv(v[i], mode, sc[i], sh[i]);
  }
  *(f32x4*)(dx + e * 4) = acc;
}

// ---- BatchNorm over rows.  A workgroup owns a slab of rows: thread t reads four channels (chunk t % (C / 4)) of the rows
// t / (C / 4) + j * rp of its slab, the rp threads of one chunk are added in index order through shared memory, the slab's two
// sums go to part[slab][2][C]; the workgroup that takes the last ticket adds the slabs in index order in double and finishes.
// MODE 0 (forward): sums of (x - x[0][c]) and its square -> stats, running statistics.
// MODE 1 (backward): sums of du and du * xhat -> dbeta, dgamma.
// at most 64 slabs: the last workgroup's fold reads every partial (with 245 slabs of 64 rows -- the first version -- that fold
// alone took 100 us of the launch's 130 at the second layer's 15 680 x 128 map)
static int bn_slab_rows(int M, int C) {
  const int rp = 256 / (C >> 2);
  int r = cdiv(M, 64);
  if (r < 4 * rp) r = 4 * rp;
  return round_up(r, rp);
}

template <int MODE>
__global__ __launch_bounds__(256) void rows_bn_sums_kernel(const float* __restrict__ x, const float* __restrict__ du, int M, int C,
                                                           int slab_rows, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, float momentum,
                                                           float* __restrict__ running_mean, float* __restrict__ running_var,
                                                           float* __restrict__ stats, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, float* __restrict__ part,
                                                           unsigned int* __restrict__ ticket) {
  __shared__ f32x4 red[2][256];
  __shared__ unsigned int last;
  const int t = threadIdx.x, cpr = C >> 2, rp = 256 / cpr;
  const int lr = t / cpr, ch = t - lr * cpr;
  const int r0 = blockIdx.x * slab_rows, r1 = r0 + slab_rows < M ? r0 + slab_rows : M;
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = s1;
  if (lr < rp) {
    f32x4 k4, inv = s1;
    if (MODE == 0) {
      k4 = *(const f32x4*)(x + 4 * ch);
    } else {
      k4 = *(const f32x4*)(stats + 4 * ch);
      inv = *(const f32x4*)(stats + C + 4 * ch);
    }
    for (int r = r0 + lr; r < r1; r += rp) {
      const f32x4 v = *(const f32x4*)(x + (long)r * C + 4 * ch);
      if (MODE == 0) {
        const f32x4 d = v - k4;
        s1 += d;
        s2 += d * d;
      } else {
        const f32x4 g = *(const f32x4*)(du + (long)r * C + 4 * ch);
        s1 += g;
        s2 += g * ((v - k4) * inv);
      }
    }
  }
  red[0][t] = s1;
  red[1][t] = s2;
  __syncthreads();
  if (t < cpr) {
    f32x4 a = red[0][t], b = red[1][t];
    for (int j = 1; j < rp; ++j) {
      a += red[0][j * cpr + t];
      b += red[1][j * cpr + t];
    }
    *(f32x4*)(part + ((long)blockIdx.x * 2 + 0) * C + 4 * t) = a;
    *(f32x4*)(part + ((long)blockIdx.x * 2 + 1) * C + 4 * t) = b;
    __threadfence();
  }
  __syncthreads();
  if (t == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  __syncthreads();
  if (!last) return;  // (uniform over the workgroup)
  __threadfence();
  const volatile float* vp = part;
  for (int c = t; c < C; c += 256) {
    double a = 0.0, b = 0.0;
    unsigned int s = 0;
    for (; s + 8 <= gridDim.x; s += 8) {  // eight slabs' loads in flight, added in slab order
      float va[8], vb[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        va[j] = vp[((long)(s + j) * 2 + 0) * C + c];
        vb[j] = vp[((long)(s + j) * 2 + 1) * C + c];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a += (double)va[j];
        b += (double)vb[j];
      }
    }
    for (; s < gridDim.x; ++s) {
      a += (double)vp[((long)s * 2 + 0) * C + c];
      b += (double)vp[((long)s * 2 + 1) * C + c];
    }
    if (MODE == 0) {
      const double am = a / M, mean = (double)x[c] + am;
      double var = b / M - am * am;
      if (var < 0.0) var = 0.0;
      const double inv = 1.0 / sqrt(var + (double)eps), sc = (double)gamma[c] * inv;
      stats[c] = (float)mean;
      stats[C + c] = (float)inv;
      stats[2 * C + c] = (float)sc;
      stats[3 * C + c] = (float)((double)beta[c] - mean * sc);
      if (running_mean != nullptr) {
        running_mean[c] = (float)((1.0 - (double)momentum) * running_mean[c] + (double)momentum * mean);
        running_var[c] = (float)((1.0 - (double)momentum) * running_var[c] + (double)momentum * var * ((double)M / (M - 1)));
      }
    } else {
      dbeta[c] = (float)a;
      dgamma[c] = (float)b;
    }
  }
  if (t == 0) *ticket = 0u;
}

__global__ __launch_bounds__(256) void rows_bn_affine_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ rm, const float* __restrict__ rv, float eps,
                                                             int C, float* __restrict__ stats) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const double inv = 1.0 / sqrt((double)rv[c] + (double)eps), sc = (double)gamma[c] * inv;
  stats[c] = rm[c];
  stats[C + c] = (float)inv;
  stats[2 * C + c] = (float)sc;
  stats[3 * C + c] = (float)((double)beta[c] - (double)rm[c] * sc);
}

// dx = scale (du - dbeta / M - xhat dgamma / M); training == 0: dx = scale du
__global__ __launch_bounds__(256) void rows_bn_dx_kernel(const float* du, const float* __restrict__ x, int M, int C,
                                                         const float* __restrict__ stats, const float* __restrict__ dgamma,
                                                         const float* __restrict__ dbeta, int training, float* dx, long total4) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total4) return;
  const int cpr = C >> 2, ch = (int)(e % cpr);
  const f32x4 g = *(const f32x4*)(du + e * 4);
  const f32x4 sc = *(const f32x4*)(stats + 2 * C + 4 * ch);
  f32x4 o;
  if (training) {
    const f32x4 v = *(const f32x4*)(x + e * 4);
    const f32x4 mean = *(const f32x4*)(stats + 4 * ch), inv = *(const f32x4*)(stats + C + 4 * ch);
    const f32x4 dg = *(const f32x4*)(dgamma + 4 * ch), db = *(const f32x4*)(dbeta + 4 * ch);
    const float im = 1.f / (float)M;
    o = sc * (g - db * im - (v - mean) * inv * (dg * im));
  } else {
    o = sc * g;
  }
  *(f32x4*)(dx + e * 4) = o;
}

// ---- head
__device__ __forceinline__ float dc_block_sum(float v, float* sh) {  // 256 threads, fixed order; every thread gets the total
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// one workgroup per output position: t = <LeakyReLU(scale x + shift) patch, w>, d = sigmoid(t), the position's BCE term; the
// workgroup that takes the last ticket adds the terms in index order in double
__global__ __launch_bounds__(256) void discr_head_fwd_kernel(const float* __restrict__ x, int H, int W, int C, int Ho, int Wo,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             const float* __restrict__ w, int y, float* __restrict__ tout,
                                                             float* __restrict__ dout, float* __restrict__ loss,
                                                             float* __restrict__ dt, double* __restrict__ partial,
                                                             unsigned int* __restrict__ ticket) {
  __shared__ float sh[4];
  __shared__ unsigned int last;
  __shared__ double stage[256];
  const int t = threadIdx.x, m = blockIdx.x, M = gridDim.x, cpr = C >> 2;
  const int ow = m % Wo, oh = (m / Wo) % Ho, n = m / (Wo * Ho);
  float acc = 0.f;
  for (int i = t; i < 4 * cpr; i += 256) {  // (kh, c4), c4 fastest: four pixels of a kernel row, four channels each
    const int kh = i / cpr, c4 = i - kh * cpr;
    const f32x4 sc = *(const f32x4*)(scale + 4 * c4), sf = *(const f32x4*)(shift + 4 * c4);
    f32x4 wv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) wv[e] = *(const f32x4*)(w + (long)(4 * c4 + e) * 16 + 4 * kh);
#pragma unroll
    for (int kw = 0; kw < 4; ++kw) {
      const f32x4 v = *(const f32x4*)(x + (((long)n * H + oh + kh) * W + ow + kw) * C + 4 * c4);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = fmaf(dc_leaky(fmaf(sc[e], v[e], sf[e])), wv[e][kw], acc);
    }
  }
  const float tv = dc_block_sum(acc, sh);
  // sigmoid(t) and sigmoid(-t) from one exponential of -|t|: neither 1 - d nor d - 1 is ever formed by subtraction
  const float ex = expf(-fabsf(tv)), big = 1.f / (1.f + ex), small = ex / (1.f + ex);
  const float d = tv >= 0.f ? big : small, dneg = tv >= 0.f ? small : big;  // dneg = 1 - d
  if (t == 0) {
    tout[m] = tv;
    dout[m] = d;
  }
  if (y < 0) return;  // (uniform: a kernel argument)
  if (t == 0) {
    const float z = y ? -tv : tv;  // BCE(sigmoid(t), y) = softplus(-t) for y = 1, softplus(t) for y = 0
    partial[m] = (double)(fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))));
    if (dt != nullptr) dt[m] = (y ? -dneg : d) / (float)M;  // (d - y) / M
    __threadfence();
    last = atomicAdd(ticket, 1u) == (unsigned int)(M - 1);
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  double tot = 0.0;
  for (int base = 0; base < M; base += 256) {
    if (base + t < M) stage[t] = *((volatile double*)partial + base + t);
    __syncthreads();
    if (t == 0) {
      const int cnt = M - base < 256 ? M - base : 256;
      for (int i = 0; i < cnt; ++i) tot += stage[i];
    }
    __syncthreads();
  }
  if (t == 0) {
    loss[0] = (float)(tot / (double)M);
    *ticket = 0u;
  }
}

// du [N][H][W][C]: the <= 16 output positions that cover a pixel, taps in index order, times LeakyReLU'(scale x + shift)
__global__ __launch_bounds__(256) void discr_head_dx_kernel(const float* __restrict__ x, int H, int W, int C, int Ho, int Wo,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            const float* __restrict__ w, const float* __restrict__ dt,
                                                            const float* __restrict__ grad, float* __restrict__ du, long total4) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total4) return;
  const int cpr = C >> 2;
  const long pix = e / cpr;
  const int c4 = (int)(e - pix * cpr);
  const int iw = (int)(pix % W), ih = (int)((pix / W) % H), n = (int)(pix / ((long)W * H));
  const float gs = grad != nullptr ? grad[0] : 1.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  f32x4 wv[4][4];  // [channel][kh][kw]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int kh = 0; kh < 4; ++kh) wv[i][kh] = *(const f32x4*)(w + (long)(4 * c4 + i) * 16 + 4 * kh);
#pragma unroll
  for (int kh = 0; kh < 4; ++kh) {
    const int oh = ih - kh;
    if (oh < 0 || oh >= Ho) continue;
#pragma unroll
    for (int kw = 0; kw < 4; ++kw) {
      const int ow = iw - kw;
      if (ow < 0 || ow >= Wo) continue;
      const float g = dt[((long)n * Ho + oh) * Wo + ow] * gs;
      acc += g * (f32x4){wv[0][kh][kw], wv[1][kh][kw], wv[2][kh][kw], wv[3][kh][kw]};
    }
  }
  const f32x4 v = *(const f32x4*)(x + pix * C + 4 * c4);
  const f32x4 sc = *(const f32x4*)(scale + 4 * c4), sf = *(const f32x4*)(shift + 4 * c4);
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] *= dc_slope(fmaf(sc[i], v[i], sf[i]));
  *(f32x4*)(du + e * 4) = acc;
}

// dw partials: thread = four channels of one kernel row (16 sums), a slab of output positions walked in index order
__global__ __launch_bounds__(256) void discr_head_dw_kernel(const float* __restrict__ x, int H, int W, int C, int Ho, int Wo, int M,
                                                            int slab, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, const float* __restrict__ dt,
                                                            const float* __restrict__ grad, float* __restrict__ part) {
  const int i = blockIdx.x * 256 + threadIdx.x, cpr = C >> 2;
  if (i >= 4 * cpr) return;
  const int kh = i / cpr, c4 = i - kh * cpr;
  const float gs = grad != nullptr ? grad[0] : 1.f;
  const f32x4 sc = *(const f32x4*)(scale + 4 * c4), sf = *(const f32x4*)(shift + 4 * c4);
  const int m0 = blockIdx.y * slab, m1 = m0 + slab < M ? m0 + slab : M;
  f32x4 acc[4];  // [channel][kw]
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int m = m0; m < m1; ++m) {
    const int ow = m % Wo, oh = (m / Wo) % Ho, n = m / (Wo * Ho);
    const float g = dt[m] * gs;
#pragma unroll
    for (int kw = 0; kw < 4; ++kw) {
      const f32x4 v = *(const f32x4*)(x + (((long)n * H + oh + kh) * W + ow + kw) * C + 4 * c4);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e][kw] = fmaf(g, dc_leaky(fmaf(sc[e], v[e], sf[e])), acc[e][kw]);
    }
  }
  float* o = part + (long)blockIdx.y * 16 * C + (long)(4 * c4) * 16 + 4 * kh;
#pragma unroll
  for (int e = 0; e < 4; ++e) *(f32x4*)(o + 16 * e) = acc[e];
}

__global__ __launch_bounds__(256) void discr_fold_kernel(const float* __restrict__ part, int nslab, int K, float* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  float s = 0.f;
  for (int p = 0; p < nslab; ++p) s += part[(long)p * K + k];
  out[k] = s;
}

static int head_slab(int M) {  // output positions per slab of the weight gradient: at most 64 slabs
  const int r = cdiv(M, 64);
  return r < 32 ? 32 : r;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace spcl

using namespace spcl;

extern "C" int spcl_patch4s2_rows_forward(const float* a, int Ca, long a_sn, long a_sc, long a_sh, long a_sw, const float* b,
                                          int Cb, long b_sn, long b_sc, long b_sh, long b_sw, int N, int H, int W, int mode,
                                          const float* scale, const float* shift, float* rows, void* stream) {
  SPCL_CHECK_ARG(a && rows, "patch4s2_rows_forward: null pointer");
  SPCL_CHECK_ARG(Ca > 0 && Cb >= 0 && (Cb == 0) == (b == nullptr), "patch4s2_rows_forward: channels %d + %d", Ca, Cb);
  SPCL_CHECK_ARG(N > 0 && H >= 2 && W >= 2, "patch4s2_rows_forward: N > 0, H, W >= 2 (got %d, %d, %d)", N, H, W);
  SPCL_CHECK_ARG(mode >= 0 && mode <= 2, "patch4s2_rows_forward: mode %d", mode);
  SPCL_CHECK_ARG(mode != 2 || (scale && shift), "patch4s2_rows_forward: mode 2 needs scale and shift");
  SPCL_CHECK_ARG(a_sn >= 0 && a_sc >= 0 && a_sh >= 0 && a_sw >= 0 && b_sn >= 0 && b_sc >= 0 && b_sh >= 0 && b_sw >= 0,
                 "patch4s2_rows_forward: negative stride");
  const int C = Ca + Cb, Ho = H / 2, Wo = W / 2;
  const long M = (long)N * Ho * Wo, total = M * 16 * C;
  SPCL_CHECK_ARG((total + 255) / 256 < (1L << 31), "patch4s2_rows_forward: too large");
  hipStream_t st = (hipStream_t)stream;
  const bool dense = b == nullptr && C % 4 == 0 && a_sc == 1 && a_sw == C && a_sh == (long)W * C && a_sn == (long)H * W * C &&
                     aligned16(a) && aligned16(rows) && (mode != 2 || (aligned16(scale) && aligned16(shift)));
  if (dense) {
    const long threads = M * C;  // (m, c4, kh)
    SPCL_LAUNCH(patch_rows_fwd_vec_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a, N, H, W, C, Ho, Wo, mode,
                scale, shift, rows, threads);
  } else {
    const DcMap ma = {a, Ca, a_sn, a_sc, a_sh, a_sw}, mb = {b, Cb, b_sn, b_sc, b_sh, b_sw};
    SPCL_LAUNCH(patch_rows_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ma, mb, N, H, W, Ho, Wo, mode, scale,
                shift, rows, total);
  }
  SPCL_LAUNCH_CHECK("patch4s2_rows_forward");
  return SPCL_OK;
}

extern "C" int spcl_patch4s2_rows_backward(const float* drows, const float* x, int N, int H, int W, int C, int c_lo, int mode,
                                           const float* scale, const float* shift, float* dx, void* stream) {
  SPCL_CHECK_ARG(drows && dx, "patch4s2_rows_backward: null pointer");
  SPCL_CHECK_ARG(N > 0 && H >= 2 && W >= 2 && C > 0, "patch4s2_rows_backward: N, C > 0, H, W >= 2 (got %d, %d, %d, %d)", N, C, H, W);
  SPCL_CHECK_ARG(mode >= 0 && mode <= 2, "patch4s2_rows_backward: mode %d", mode);
  SPCL_CHECK_ARG(mode == 0 || x, "patch4s2_rows_backward: modes 1, 2 need the stored map");
  SPCL_CHECK_ARG(mode != 2 || (scale && shift), "patch4s2_rows_backward: mode 2 needs scale and shift");
  SPCL_CHECK_ARG(c_lo >= 0 && c_lo < C && (c_lo == 0 || mode == 0), "patch4s2_rows_backward: c_lo %d (mode %d, C %d)", c_lo, mode, C);
  const int Ho = H / 2, Wo = W / 2;
  const long total = (long)N * H * W * (C - c_lo);
  SPCL_CHECK_ARG((total + 255) / 256 < (1L << 31), "patch4s2_rows_backward: too large");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = c_lo == 0 && C % 4 == 0 && aligned16(drows) && aligned16(dx) && (mode == 0 || aligned16(x)) &&
                   (mode != 2 || (aligned16(scale) && aligned16(shift)));
  if (vec) {
    const long total4 = total / 4;
    SPCL_LAUNCH(patch_rows_bwd_vec_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, drows, x, N, H, W, C, Ho, Wo,
                mode, scale, shift, dx, total4);
  } else {
    SPCL_LAUNCH(patch_rows_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, drows, x, N, H, W, C, c_lo, Ho, Wo,
                mode, scale, shift, dx, total);
  }
  SPCL_LAUNCH_CHECK("patch4s2_rows_backward");
  return SPCL_OK;
}

extern "C" size_t spcl_rows_bn_workspace_bytes(int M, int C) {
  if (M < 2 || C <= 0 || C % 4 != 0 || C > 1024) return 0;
  const int nslab = cdiv(M, bn_slab_rows(M, C));
  return 64 + (size_t)nslab * 2 * C * sizeof(float);
}

static int rows_bn_check(const char* who, const void* x, int M, int C, const void* ws, size_t ws_bytes) {
  SPCL_CHECK_ARG(x && ws, "%s: null pointer", who);
  SPCL_CHECK_ARG(M >= 2 && C > 0 && C % 4 == 0 && C <= 1024, "%s: M >= 2, C a multiple of 4 up to 1024 (got %d, %d)", who, M, C);
  SPCL_CHECK_ARG(ws_bytes >= spcl_rows_bn_workspace_bytes(M, C), "%s: workspace of %zu bytes", who,
                 spcl_rows_bn_workspace_bytes(M, C));
  SPCL_CHECK_ARG(aligned16(x) && aligned16(ws), "%s: 16-byte aligned maps", who);
  return SPCL_OK;
}

extern "C" int spcl_rows_bn_forward(const float* x, int M, int C, const float* gamma, const float* beta, float eps, float momentum,
                                    float* running_mean, float* running_var, float* stats, void* ws, size_t ws_bytes,
                                    void* stream) {
  if (int rc = rows_bn_check("rows_bn_forward", x, M, C, ws, ws_bytes)) return rc;
  SPCL_CHECK_ARG(gamma && beta && stats, "rows_bn_forward: null pointer");
  SPCL_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "rows_bn_forward: running_mean and running_var go together");
  hipStream_t st = (hipStream_t)stream;
  unsigned int* ticket = (unsigned int*)ws;
  float* part = (float*)((char*)ws + 64);
  if (hipMemsetAsync(ticket, 0, sizeof(unsigned int), st) != hipSuccess) {
    spcl::set_error("rows_bn_forward: memset failed");
    return SPCL_ELAUNCH;
  }
  const int sr = bn_slab_rows(M, C), nslab = cdiv(M, sr);
  SPCL_LAUNCH(rows_bn_sums_kernel<0>, dim3((unsigned)nslab), dim3(256), 0, st, x, (const float*)nullptr, M, C, sr, gamma, beta, eps,
              momentum, running_mean, running_var, stats, (float*)nullptr, (float*)nullptr, part, ticket);
  SPCL_LAUNCH_CHECK("rows_bn_forward");
  return SPCL_OK;
}

extern "C" int spcl_rows_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                                        float eps, int C, float* stats, void* stream) {
  SPCL_CHECK_ARG(gamma && beta && running_mean && running_var && stats, "rows_bn_eval_affine: null pointer");
  SPCL_CHECK_ARG(C > 0, "rows_bn_eval_affine: C %d", C);
  SPCL_LAUNCH(rows_bn_affine_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, gamma, beta, running_mean,
              running_var, eps, C, stats);
  SPCL_LAUNCH_CHECK("rows_bn_eval_affine");
  return SPCL_OK;
}

extern "C" int spcl_rows_bn_backward(const float* du, const float* x, int M, int C, const float* gamma, const float* stats,
                                     int training, float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                                     void* stream) {
  if (int rc = rows_bn_check("rows_bn_backward", x, M, C, ws, ws_bytes)) return rc;
  SPCL_CHECK_ARG(du && gamma && stats && dx && dgamma && dbeta, "rows_bn_backward: null pointer");
  SPCL_CHECK_ARG(aligned16(du) && aligned16(dx) && aligned16(stats) && aligned16(dgamma) && aligned16(dbeta),
                 "rows_bn_backward: 16-byte aligned maps");
  hipStream_t st = (hipStream_t)stream;
  unsigned int* ticket = (unsigned int*)ws;
  float* part = (float*)((char*)ws + 64);
  if (hipMemsetAsync(ticket, 0, sizeof(unsigned int), st) != hipSuccess) {
    spcl::set_error("rows_bn_backward: memset failed");
    return SPCL_ELAUNCH;
  }
  const int sr = bn_slab_rows(M, C), nslab = cdiv(M, sr);
  SPCL_LAUNCH(rows_bn_sums_kernel<1>, dim3((unsigned)nslab), dim3(256), 0, st, x, du, M, C, sr, gamma, (const float*)nullptr, 0.f,
              0.f, (float*)nullptr, (float*)nullptr, (float*)stats, dgamma, dbeta, part, ticket);
  const long total4 = (long)M * (C / 4);
  SPCL_LAUNCH(rows_bn_dx_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, du, x, M, C, stats, (const float*)dgamma,
              (const float*)dbeta, training, dx, total4);
  SPCL_LAUNCH_CHECK("rows_bn_backward");
  return SPCL_OK;
}

extern "C" size_t spcl_discr_head_workspace_bytes(int N, int H, int W, int C) {
  if (N <= 0 || H < 4 || W < 4 || C <= 0 || C % 4 != 0) return 0;
  const long M = (long)N * (H - 3) * (W - 3);
  if (M >= (1L << 24)) return 0;
  const size_t fwd = 64 + (size_t)M * sizeof(double);
  const size_t bwd = (size_t)cdiv((int)M, head_slab((int)M)) * 16 * C * sizeof(float);
  return fwd > bwd ? fwd : bwd;
}

static int head_check(const char* who, const void* x, int N, int H, int W, int C, const void* scale, const void* shift,
                      const void* w, const void* ws, size_t ws_bytes) {
  SPCL_CHECK_ARG(x && scale && shift && w && ws, "%s: null pointer", who);
  SPCL_CHECK_ARG(N > 0 && H >= 4 && W >= 4, "%s: N > 0 and a map of at least 4 x 4 (got %d, %d x %d)", who, N, H, W);
  SPCL_CHECK_ARG(C > 0 && C % 4 == 0, "%s: C a multiple of 4 (got %d)", who, C);
  SPCL_CHECK_ARG((long)N * (H - 3) * (W - 3) < (1L << 24), "%s: too many output positions", who);
  SPCL_CHECK_ARG(ws_bytes >= spcl_discr_head_workspace_bytes(N, H, W, C), "%s: workspace of %zu bytes", who,
                 spcl_discr_head_workspace_bytes(N, H, W, C));
  SPCL_CHECK_ARG(aligned16(x) && aligned16(scale) && aligned16(shift) && aligned16(w) && aligned16(ws), "%s: 16-byte aligned maps",
                 who);
  return SPCL_OK;
}

extern "C" int spcl_discr_head_forward(const float* x, int N, int H, int W, int C, const float* scale, const float* shift,
                                       const float* w, int y, float* t, float* d, float* loss, float* dt, void* ws, size_t ws_bytes,
                                       void* stream) {
  if (int rc = head_check("discr_head_forward", x, N, H, W, C, scale, shift, w, ws, ws_bytes)) return rc;
  SPCL_CHECK_ARG(t && d, "discr_head_forward: null pointer");
  SPCL_CHECK_ARG(y <= 1 && (y < 0 || loss), "discr_head_forward: y is 0, 1 (with loss) or negative (got %d)", y);
  hipStream_t st = (hipStream_t)stream;
  const int Ho = H - 3, Wo = W - 3, M = N * Ho * Wo;
  unsigned int* ticket = (unsigned int*)ws;
  double* partial = (double*)((char*)ws + 64);
  if (y >= 0 && hipMemsetAsync(ticket, 0, sizeof(unsigned int), st) != hipSuccess) {
    spcl::set_error("discr_head_forward: memset failed");
    return SPCL_ELAUNCH;
  }
  SPCL_LAUNCH(discr_head_fwd_kernel, dim3((unsigned)M), dim3(256), 0, st, x, H, W, C, Ho, Wo, scale, shift, w, y < 0 ? -1 : y, t, d,
              loss, dt, partial, ticket);
  SPCL_LAUNCH_CHECK("discr_head_forward");
  return SPCL_OK;
}

extern "C" int spcl_discr_head_backward(const float* x, int N, int H, int W, int C, const float* scale, const float* shift,
                                        const float* w, const float* dt, const float* grad, float* du, float* dw, void* ws,
                                        size_t ws_bytes, void* stream) {
  if (int rc = head_check("discr_head_backward", x, N, H, W, C, scale, shift, w, ws, ws_bytes)) return rc;
  SPCL_CHECK_ARG(dt, "discr_head_backward: null pointer");
  SPCL_CHECK_ARG(du == nullptr || aligned16(du), "discr_head_backward: 16-byte aligned maps");
  SPCL_CHECK_ARG(dw == nullptr || aligned16(dw), "discr_head_backward: 16-byte aligned maps");
  hipStream_t st = (hipStream_t)stream;
  const int Ho = H - 3, Wo = W - 3, M = N * Ho * Wo;
  if (du != nullptr) {
    const long total4 = (long)N * H * W * (C / 4);
    SPCL_LAUNCH(discr_head_dx_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, x, H, W, C, Ho, Wo, scale, shift, w,
                dt, grad, du, total4);
  }
  if (dw != nullptr) {
    const int slab = head_slab(M), nslab = cdiv(M, slab), K = 16 * C;
    SPCL_LAUNCH(discr_head_dw_kernel, dim3((unsigned)cdiv(C, 256), (unsigned)nslab), dim3(256), 0, st, x, H, W, C, Ho, Wo, M, slab,
                scale, shift, dt, grad, (float*)ws);
    SPCL_LAUNCH(discr_fold_kernel, dim3((unsigned)cdiv(K, 256)), dim3(256), 0, st, (const float*)ws, nslab, K, dw);
  }
  SPCL_LAUNCH_CHECK("discr_head_backward");
  return SPCL_OK;
}
