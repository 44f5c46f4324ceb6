// Soft-Dice + class-weighted KL on one-hot targets: the supervised criterion contrastyou/losses/dice.py serves (it is not in
// the reference).  With p = softmax(logits), t = one-hot(label), M = N H W, S = all classes or 1 .. C-1, groups g = the whole
// batch (G = 1) or one per sample (G = N), and I_gc = sum p t, P_gc = sum p, T_gc = sum t over the pixels of group g:
//   L_dice = 1 - 1 / (G |S|) sum_g sum_{c in S} (2 I_gc + s) / (P_gc + T_gc + s)
//   L_kl   = 1 / M sum_i w[l_i] * -log((p_{i,l_i} + eps) / (1 + eps))          (w == 1: spcl_sup_loss_forward's value)
//   loss   = dice_weight L_dice + kl_weight L_kl
// A label outside [0, C) is an all-zero one-hot row: no KL term, nothing in I or T; its probabilities count in P.
//
// The gradient of a Dice term needs the group sums, so the criterion is two streaming passes over the class map:
//   1. sup_dice_sums_kernel: grid (gx, N), blockIdx.y = the sample (as sup_loss_fwd_kernel), a grid-stride loop over the
//      sample's pixels.  A thread forms the softmax in registers and keeps I_c, P_c (double) per class, the weighted KL terms
//      (double), and T_c plus the arg-max Dice counts as integers.  Every workgroup leaves one row of sums in the workspace.
//      sup_dice_finish_kernel, the same entry's second launch: workgroup n adds sample n's rows in index order, and the one
//      that takes the last of the N tickets adds the samples in index order (a fixed order: the same bits on every run, no
//      floating-point atomics) and writes the loss, its two parts and per (group, class) the coefficients
//      a = -2 / (G |S| D), b = (2 I + s) / (G |S| D^2), D = P + T + s.  The ticket is zero on entry and is left zero: no
//      memset per call.
//   2. sup_dice_grad_kernel re-forms the softmax; d loss / d p_c = dice_weight (a t_c + b) for c in S, plus
//      -kl_weight w_l / (M (p_l + eps)) on the labelled class; softmax_jacobian turns that into dlogits.  No reduction.
//
// Registers: CM classes cost 2 CM double accumulators (4 CM VGPRs) per thread, so the kernels are compiled for CM = 4 (one
// 16-byte access per pixel, counters packed in 16-bit fields as sup_loss_fwd4_kernel), 8 and 16; DESIGN.md has the counts.
#include "pixel_criterion.hpp"

namespace {

using spcl::row16_sum_f64;

struct dice_args {
  const float* x;        // [N][HW][C]
  const int64_t* y;      // [N][HW]
  const float* w;        // [C]
  int N, C, HW, gx;
  int per_sample, first; // first class of S (0, or 1 without the background)
  float dw, kw, smooth, eps;
  float* loss;           // [1]
  float* parts;          // [2]: L_kl, L_dice
  unsigned long long* inter;  // [N][C]
  unsigned long long* uni;    // [N][C]
  float* coef;           // [G][C][2]: a, b
  unsigned int* ticket;  // [1 + N]: the batch's, then one per sample
  double* rows_d;       // [N gx][2 C + 1]: I, P, KL of every workgroup
  unsigned int* rows_u;  // [N gx][3 C]: T, inter, union
  double* samp_d;        // [N][3 C + 1]: I, P, T, KL of every sample
};

__device__ __forceinline__ double wave_sum_f64(double v) {  // fixed order: deterministic
  v = row16_sum_f64(v);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}

constexpr int kMaxGx = 64;  // workgroups per sample (dice_gx)

// LDS of the two finishing stages, one buffer: a sample's rows (kMaxGx x (2 CM + 1) doubles, behind them kMaxGx x 3 CM
// unsigned ints), then chunks of per-sample sums
template <int CM>
struct finish_lds {
  static constexpr int ND = kMaxGx * (2 * CM + 1);
  static constexpr int NU = kMaxGx * 3 * CM;
  static constexpr int SB = ND + (NU + 1) / 2 > 1024 ? ND + (NU + 1) / 2 : 1024;
};

// The finish: a launch of its own behind the sums (sup_loss_finish_kernel's place), one workgroup per sample -- the launch
// boundary makes the rows visible, so the N gx workgroups of the first pass neither fence nor take a ticket (with a ticket and
// an agent-scope release per workgroup the first pass took 149 us at 32 x 4 x 224^2, most of it those fences).  Every row is
// fetched into LDS by the whole workgroup first (independent, coalesced loads: summed straight from memory the in-order chain
// paid one memory round trip per row) and added in index order from there.
//   A. workgroup n adds sample n's gx rows -> samp_d[n], inter / union of n;
//   B. the workgroup that takes the last of the N tickets adds the samples in index order (the KL term always; I, P, T where
//      the batch is one group), writes the coefficients, the two parts and the loss, and resets the ticket.
template <int CM>
__global__ void __launch_bounds__(256) sup_dice_finish_kernel(const dice_args a) {
  using L = finish_lds<CM>;
  __shared__ double sd[L::SB];
  __shared__ double tot[3 * CM + 1];
  __shared__ double gs[1024];  // the groups' sums of Dice ratios (G <= N <= 1024)
  __shared__ unsigned int last;
  const int C = a.C, N = a.N, gx = a.gx, ncd = 2 * C + 1, ncs = 3 * C + 1, tid = threadIdx.x, n = blockIdx.x;
  unsigned int* su32 = reinterpret_cast<unsigned int*>(sd + L::ND);
  {
    const double* rd = a.rows_d + (size_t)n * gx * ncd;
    const unsigned int* ru = a.rows_u + (size_t)n * gx * 3 * C;
    for (int i = tid; i < gx * ncd; i += blockDim.x) sd[i] = rd[i];
    for (int i = tid; i < gx * 3 * C; i += blockDim.x) su32[i] = ru[i];
  }
  __syncthreads();
  if (tid < ncs) {  // wave 0: the sample's I, P, T (as a double: below 2^31, exact), KL
    double s = 0.0;
    if (tid >= 2 * C && tid < 3 * C) {
      unsigned long long t = 0ull;
      for (int bx = 0; bx < gx; ++bx) t += su32[bx * 3 * C + (tid - 2 * C)];
      s = (double)t;
    } else {
      const int col = tid < 2 * C ? tid : 2 * C;
      for (int bx = 0; bx < gx; ++bx) s += sd[bx * ncd + col];
    }
    a.samp_d[(size_t)n * ncs + tid] = s;
  } else if (tid >= 64 && tid < 64 + 2 * C) {  // wave 1: the sample's Dice counts
    const int j = tid - 64, which = j / C, c = j - which * C;
    unsigned long long t = 0ull;
    for (int bx = 0; bx < gx; ++bx) t += su32[bx * 3 * C + (1 + which) * C + c];
    (which ? a.uni : a.inter)[(size_t)n * C + c] = t;
  }
  if (tid < 64) __threadfence();  // (release: samp_d[n] was written by this wave)
  if (tid == 0) last = atomicAdd(a.ticket, 1u) == (unsigned int)N - 1u;
  __syncthreads();
  if (!last) return;  // (uniform over the workgroup)
  __threadfence();    // (acquire: samp_d of the other samples)
  const int G = a.per_sample ? N : 1;
  const double norm = (double)G * (double)(C - a.first), sm = (double)a.smooth;
  // group g's I, P, T at v[0 .. 3 C) (LDS) -> its coefficients, and its sum of Dice ratios
  auto group = [&](const double* v, int g) {
    double ds = 0.0;
    for (int c = 0; c < C; ++c) {
      double ca = 0.0, cb = 0.0;
      if (c >= a.first) {
        const double D = v[C + c] + v[2 * C + c] + sm, num = 2.0 * v[c] + sm;
        ds += num / D;
        ca = -2.0 / (norm * D);
        cb = num / (norm * D * D);
      }
      a.coef[((size_t)g * C + c) * 2] = (float)ca;
      a.coef[((size_t)g * C + c) * 2 + 1] = (float)cb;
    }
    return ds;
  };
  double run = 0.0;
  const int chunk = L::SB / ncs;
  for (int n0 = 0; n0 < N; n0 += chunk) {
    const int m = N - n0 < chunk ? N - n0 : chunk;
    __syncthreads();
    for (int i = tid; i < m * ncs; i += blockDim.x) sd[i] = a.samp_d[(size_t)n0 * ncs + i];
    __syncthreads();
    if (tid < ncs)
      for (int j = 0; j < m; ++j) run += sd[j * ncs + tid];
    if (a.per_sample)  // (the waves behind wave 0 first: it is busy with the column sums)
      for (int j = (int)blockDim.x - 1 - tid; j < m; j += blockDim.x) gs[n0 + j] = group(sd + j * ncs, n0 + j);
  }
  if (tid < ncs) tot[tid] = run;
  __syncthreads();
  if (!a.per_sample && tid == 0) gs[0] = group(tot, 0);
  __syncthreads();
  if (tid == 0) {
    double ds = 0.0;
    for (int g = 0; g < G; ++g) ds += gs[g];
    const double ldice = 1.0 - ds / norm;
    const double lkl = tot[3 * C] / ((double)N * (double)a.HW);
    a.parts[0] = (float)lkl;
    a.parts[1] = (float)ldice;
    a.loss[0] = (float)((double)a.dw * ldice + (double)a.kw * lkl);
    *a.ticket = 0u;
  }
}

// CT == 4: C == 4, one 16-byte access per pixel (the host checked the alignment) and 16-bit packed counters (a thread sees
// fewer than 2^15 pixels: the host checked); CT == 0: any C <= CM, counters through integer LDS atomics
template <int CT, int CM>
__global__ void __launch_bounds__(256) sup_dice_sums_kernel(const dice_args a) {
  constexpr int NR = 2 * CM + 1;
  __shared__ float sw[16];
  __shared__ unsigned int st[16], si[16], su[16];
  __shared__ double red[4][NR];
  __shared__ unsigned int cred[4][12];
  const int n = blockIdx.y, C = CT == 4 ? 4 : a.C, HW = a.HW;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x < 16) {
    sw[threadIdx.x] = (int)threadIdx.x < C ? a.w[threadIdx.x] : 0.f;
    st[threadIdx.x] = si[threadIdx.x] = su[threadIdx.x] = 0u;
  }
  __syncthreads();
  double I[CM], P[CM], kl = 0.0;
#pragma unroll
  for (int k = 0; k < CM; ++k) I[k] = P[k] = 0.0;
  unsigned long long ct = 0ull, ci = 0ull, cu = 0ull;
  const float eps = a.eps;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
    const size_t p = (size_t)n * HW + i;
    const long l = a.y[p];
    float v[16];
    load_pixel<CT>(a.x + p * C, C, v);
    int best = 0;
    float bv = v[0];
#pragma unroll
    for (int k = 1; k < CM; ++k)
      if (k < C && v[k] > bv) {  // first maximum (torch.max(1)[1], spcl_argmax_classes)
        bv = v[k];
        best = k;
      }
    const float z = softmax_numerators(v, C);
    float pl = 0.f;
#pragma unroll
    for (int k = 0; k < CM; ++k)
      if (k < C) {
        const float pk = v[k] / z;
        const bool hit = l == k;
        P[k] += (double)pk;
        I[k] += hit ? (double)pk : 0.0;
        pl = hit ? pk : pl;
      }
    const bool ok = l >= 0 && l < C;
    if (ok) kl += (double)sw[l] * (double)(-logf((pl + eps) / (1.f + eps)));
    if (CT == 4) {
      cu += 1ull << (16 * best);
      if (ok) {
        cu += 1ull << (16 * (int)l);
        ct += 1ull << (16 * (int)l);
      }
      if (l == best) ci += 1ull << (16 * best);
    } else {
      atomicAdd(&su[best], 1u);
      if (ok) {
        atomicAdd(&su[l], 1u);
        atomicAdd(&st[l], 1u);
      }
      if (l == best) atomicAdd(&si[best], 1u);
    }
  }
#pragma unroll
  for (int k = 0; k < CM; ++k) {
    const double ti = wave_sum_f64(I[k]), tp = wave_sum_f64(P[k]);
    if (lane == 0) {
      red[wave][k] = ti;
      red[wave][CM + k] = tp;
    }
  }
  kl = wave_sum_f64(kl);
  if (lane == 0) red[wave][2 * CM] = kl;
  if (CT == 4) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const unsigned tt = wave_sum_u((unsigned)(ct >> (16 * c)) & 0xffffu);
      const unsigned ti = wave_sum_u((unsigned)(ci >> (16 * c)) & 0xffffu);
      const unsigned tu = wave_sum_u((unsigned)(cu >> (16 * c)) & 0xffffu);
      if (lane == 0) {
        cred[wave][c] = tt;
        cred[wave][4 + c] = ti;
        cred[wave][8 + c] = tu;
      }
    }
  }
  __syncthreads();
  const size_t row = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  if ((int)threadIdx.x < NR) {
    const int j = threadIdx.x, which = j / CM, k = j - which * CM;  // which: 0 = I, 1 = P, 2 = KL (k == 0)
    if (which == 2 || k < C) {
      const double s = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
      a.rows_d[row * (2 * C + 1) + (which == 2 ? 2 * C : which * C + k)] = s;
    }
  }
  if ((int)threadIdx.x < 3 * C) {
    const int j = threadIdx.x, which = j / C, c = j - which * C;
    unsigned int t;
    if (CT == 4) t = (cred[0][j] + cred[1][j]) + (cred[2][j] + cred[3][j]);
    else t = which == 0 ? st[c] : which == 1 ? si[c] : su[c];
    a.rows_u[row * 3 * C + j] = t;
  }
}

struct dice_grad_args {
  const float* x;
  const int64_t* y;
  const float* w;
  const float* coef;     // [G][C][2]
  const float* gscale;   // nullable: the upstream gradient, a device scalar
  int C, HW, per_sample;
  float dw, ckl, eps;    // ckl = kl_weight / M
  float* dx;
};

template <int CT>
__global__ void __launch_bounds__(256) sup_dice_grad_kernel(const dice_grad_args a) {
  __shared__ float sa[16], sb[16], sw[16];
  const int n = blockIdx.y, C = CT == 4 ? 4 : a.C, HW = a.HW;
  if ((int)threadIdx.x < C) {
    const float* cf = a.coef + ((size_t)(a.per_sample ? n : 0) * C + threadIdx.x) * 2;
    sa[threadIdx.x] = a.dw * cf[0];
    sb[threadIdx.x] = a.dw * cf[1];
    sw[threadIdx.x] = a.ckl * a.w[threadIdx.x];
  }
  __syncthreads();
  const float gs = a.gscale ? a.gscale[0] : 1.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
    const size_t p = (size_t)n * HW + i;
    const long l = a.y[p];
    float v[16], g[16];
    load_pixel<CT>(a.x + p * C, C, v);
    const float z = softmax_numerators(v, C);
    float sgp = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < C) {
        v[k] /= z;
        g[k] = sb[k];
        if (l == k) g[k] += sa[k] - sw[k] / (v[k] + a.eps);
        sgp = fmaf(g[k], v[k], sgp);
      }
    softmax_jacobian(v, sgp, g, C);
    if (a.gscale) {
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < C) g[k] *= gs;
    }
    store_pixel<CT>(a.dx + p * C, C, g);
  }
}

// workgroups per sample: at most kMaxGx = 64 (sup_loss_fwd_kernel's cap; a sample's rows are summed one by one from LDS) and
// about 2048 in all at large N, never fewer than 8; a grid-stride loop takes the rest, in equal shares -- the smallest grid
// that needs no more iterations than the cap does
inline int dice_gx(int N, long HW) {
  long g = (HW + 255) / 256, cap = 2048 / N;
  if (cap < 8) cap = 8;
  if (cap > 64) cap = 64;
  if (g <= cap) return (int)g;
  const long iters = (g + cap - 1) / cap;
  return (int)((g + iters - 1) / iters);
}

struct dice_layout {
  size_t rows_d, rows_u, samp_d, total;
};
inline dice_layout dice_ws(int N, int C, int H, int W) {
  const size_t R = (size_t)N * dice_gx(N, (long)H * W);
  dice_layout o;
  o.rows_d = 64;  // (the ticket's block: zero on entry, left zero by the workgroup that finishes)
  o.samp_d = o.rows_d + R * (2 * C + 1) * sizeof(double);
  o.rows_u = o.samp_d + (size_t)N * (3 * C + 1) * sizeof(double);
  o.total = o.rows_u + R * 3 * C * sizeof(unsigned int);
  o.total = (o.total + 15) / 16 * 16;
  return o;
}

inline bool dice_shape_ok(int N, int C, int H, int W) {
  return N > 0 && N <= 1024 && C >= 1 && C <= 16 && H > 0 && W > 0 && (long)N * H * W < (1L << 31);
}

}  // namespace

extern "C" size_t spcl_sup_dice_workspace_bytes(int N, int C, int H, int W) {
  return dice_shape_ok(N, C, H, W) ? dice_ws(N, C, H, W).total : 0;
}

extern "C" int spcl_sup_dice_forward(const float* logits, const int64_t* labels, const float* class_weight, int N, int C, int H,
                                     int W, float dice_weight, float kl_weight, int include_background, int per_sample,
                                     float smooth, float eps, float* loss, float* parts, int64_t* inter, int64_t* uni,
                                     float* coef, void* ws, size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(logits && labels && class_weight && loss && parts && inter && uni && coef && ws,
                 "spcl_sup_dice_forward: null pointer");
  SPCL_CHECK_ARG(dice_shape_ok(N, C, H, W), "spcl_sup_dice_forward: bad shape (N <= 1024, C <= 16)");
  SPCL_CHECK_ARG(include_background || C > 1, "spcl_sup_dice_forward: no class left without the background");
  SPCL_CHECK_ARG(smooth > 0.f && eps >= 0.f, "spcl_sup_dice_forward: smooth > 0, eps >= 0");
  const dice_layout lay = dice_ws(N, C, H, W);
  SPCL_CHECK_ARG(ws_bytes >= lay.total, "spcl_sup_dice_forward: workspace too small");
  SPCL_CHECK_ARG((uintptr_t)ws % 16 == 0, "spcl_sup_dice_forward: workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W, gx = dice_gx(N, HW);
  dice_args a;
  a.x = logits, a.y = labels, a.w = class_weight;
  a.N = N, a.C = C, a.HW = HW, a.gx = gx;
  a.per_sample = per_sample != 0, a.first = include_background ? 0 : 1;
  a.dw = dice_weight, a.kw = kl_weight, a.smooth = smooth, a.eps = eps;
  a.loss = loss, a.parts = parts, a.inter = (unsigned long long*)inter, a.uni = (unsigned long long*)uni, a.coef = coef;
  a.ticket = (unsigned int*)ws;
  a.rows_d = (double*)((char*)ws + lay.rows_d);
  a.samp_d = (double*)((char*)ws + lay.samp_d);
  a.rows_u = (unsigned int*)((char*)ws + lay.rows_u);
  const bool vec4 = C == 4 && (uintptr_t)logits % 16 == 0 && (HW + gx * 256 - 1) / (gx * 256) < 32768;
  spcl::prof_cost((double)N * HW * (C * 4.0 + 8.0), 0.0);
  if (vec4) SPCL_LAUNCH((sup_dice_sums_kernel<4, 4>), dim3(gx, N), dim3(256), 0, st, a);
  else if (C <= 8) SPCL_LAUNCH((sup_dice_sums_kernel<0, 8>), dim3(gx, N), dim3(256), 0, st, a);
  else SPCL_LAUNCH((sup_dice_sums_kernel<0, 16>), dim3(gx, N), dim3(256), 0, st, a);
  if (C <= 4) SPCL_LAUNCH((sup_dice_finish_kernel<4>), dim3(N), dim3(256), 0, st, a);
  else if (C <= 8) SPCL_LAUNCH((sup_dice_finish_kernel<8>), dim3(N), dim3(256), 0, st, a);
  else SPCL_LAUNCH((sup_dice_finish_kernel<16>), dim3(N), dim3(256), 0, st, a);
  SPCL_LAUNCH_CHECK("spcl_sup_dice_forward");
  return SPCL_OK;
}

extern "C" int spcl_sup_dice_backward(const float* logits, const int64_t* labels, const float* class_weight, const float* coef,
                                      int N, int C, int H, int W, float dice_weight, float kl_weight, int per_sample, float eps,
                                      const float* gscale, float* dlogits, void* stream) {
  SPCL_CHECK_ARG(logits && labels && class_weight && coef && dlogits, "spcl_sup_dice_backward: null pointer");
  SPCL_CHECK_ARG(dice_shape_ok(N, C, H, W), "spcl_sup_dice_backward: bad shape (N <= 1024, C <= 16)");
  const int HW = H * W;
  int gx = (HW + 255) / 256;
  const int cap = 4096 / N > 8 ? 4096 / N : 8;
  if (gx > cap) gx = cap;
  dice_grad_args a;
  a.x = logits, a.y = labels, a.w = class_weight, a.coef = coef, a.gscale = gscale;
  a.C = C, a.HW = HW, a.per_sample = per_sample != 0;
  a.dw = dice_weight, a.ckl = (float)((double)kl_weight / ((double)N * HW)), a.eps = eps;
  a.dx = dlogits;
  spcl::prof_cost((double)N * HW * (C * 8.0 + 8.0), 0.0);
  if (C == 4 && ((uintptr_t)logits | (uintptr_t)dlogits) % 16 == 0)
    SPCL_LAUNCH((sup_dice_grad_kernel<4>), dim3(gx, N), dim3(256), 0, (hipStream_t)stream, a);
  else
    SPCL_LAUNCH((sup_dice_grad_kernel<0>), dim3(gx, N), dim3(256), 0, (hipStream_t)stream, a);
  SPCL_LAUNCH_CHECK("spcl_sup_dice_backward");
  return SPCL_OK;
}
