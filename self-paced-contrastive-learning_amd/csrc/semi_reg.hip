// Regularisers of the mean-teacher, entropy-minimisation and mix-up baselines (semi_seg/hooks/mt.py, semi_seg/hooks/entmin.py,
// semi_seg/hooks/mixup.py).
//
//   spcl_ema_update:      the teacher's exponential moving average over ONE flat f32 buffer (mt.py:54 -> deepclustering2
//                         ema_updater: mul_(alpha), add_((1 - alpha) * s), mul_(1 - decay) per parameter tensor, ~180 launches
//                         for the UNet) as one launch.  12 bytes per element (read t, read s, write t), no reuse: bandwidth-
//                         bound.  16-byte loads / stores over the part of the teacher that is 16-byte aligned, a scalar head
//                         of up to 3 elements before it and a scalar tail of up to 3 behind it; the student is read with
//                         16-byte loads when it shares the teacher's misalignment, with four 4-byte loads otherwise.  The grid
//                         is capped at 2048 workgroups of 256 (8 per CU on 256 CUs), grid-stride beyond: the UNet's 2.16 M
//                         parameters are 540 k granules over 524 k threads, 26 MB in all.  Measured 7.9 - 8.1 us per launch
//                         (profiles/mt_step_time.txt; the buffers stay in the Infinity Cache between steps) against 0.77 ms
//                         for the per-tensor torch formulation.
//   spcl_mt_softmax_mse:  weight * mean((flip(T) - softmax(b))^2) and its gradient w.r.t. b in one launch; T = the teacher's
//                         raw output (mt.py:49-52 applies no softmax) or its softmax (the older _mixins.py:147).
//   spcl_entropy_softmax: weight * mean over pixels of -sum_c p_c log(p_c + eps), p = softmax(logits), and its gradient.
//   spcl_ucmt_softmax_mse: the uncertainty-aware mean teacher's criterion (semi_seg/epochers/comparable.py:84-105):
//                         weight * mean over pixels of m * mean_c (softmax(s) - softmax(flip(T)))^2 with m = [normalised entropy
//                         of softmax(mean of K noisy teacher maps) <= threshold], its gradient w.r.t. s, the number of kept
//                         pixels and (optionally) the mask, in one launch.  K + 2 maps read once, one written: the K pointers
//                         travel by value in the kernel's argument block, the average is accumulated while the maps stream in
//                         (16 live floats, then dead before the student / teacher pair is loaded).
//
// and of the mix-up baseline (semi_seg/hooks/mixup.py), over the VIRTUAL concatenation of two batches of B samples (sample n
// is a[n] for n < B, b[n - B] otherwise; nothing is concatenated) and a permutation index of its 2B samples:
//   spcl_mixup_images:    out[n] = lam * x[n] + (1 - lam) * x[index[n]] (mixup.py:30), three f32 roundings in torch's order
//                         (two products, one sum: never contracted to a fused multiply-add), bit for bit what torch computes.
//                         12 bytes per element, no reuse: bandwidth-bound.  One grid row per output sample, a capped grid
//                         stride in x; 16-byte loads / stores when the sample size is a multiple of four elements and the three
//                         base pointers are 16-byte aligned, 4-byte ones otherwise.
//   spcl_mixup_kl_onehot: weight * KL_div(eps)(softmax(logits), lam * onehot(y) + (1 - lam) * onehot(y[index])) and its
//                         gradient (mixup.py:31,66-75): the soft target is built per pixel from two labels, never stored.
//
// The criteria are pixel functors on the one skeleton of pixel_criterion.hpp (one thread per pixel, per-workgroup double
// partials, summed in index order by the last workgroup): loss and gradient are bitwise reproducible.
//   spcl_consistency_softmax_mse, spcl_mt_softmax_mse(teacher_mode = 1):  mt_mse<true> -- the same launch
//   spcl_mt_softmax_mse(teacher_mode = 0):                                mt_mse<false>
//   spcl_entropy_softmax:  entropy_term      spcl_ucmt_softmax_mse:  ucmt_mse<4> / ucmt_mse<0>
//   spcl_mixup_kl_onehot:  mixup_kl
#include "common.hpp"
#include "pixel_criterion.hpp"

namespace {

// three f32 roundings, in the reference's order: t * alpha | + (1 - alpha) * s (one fused multiply-add, as torch's
// add_(s, alpha=) computes it) | * (1 - decay).  DECAY = false leaves the last one out (no multiplication by 1.0).
template <bool DECAY>
__device__ __forceinline__ float ema_one(float t, float s, float alpha, float oma, float keep) {
  const float r = fmaf(oma, s, t * alpha);
  return DECAY ? r * keep : r;
}

// t + head is 16-byte aligned; n4 granules follow it; SVEC: s + head is 16-byte aligned too
template <bool DECAY, bool SVEC>
__global__ void __launch_bounds__(256) ema_update_kernel(float* __restrict__ t, const float* __restrict__ s, size_t head,
                                                         size_t n4, size_t n, float alpha, float oma, float keep) {
  f32x4* tv = reinterpret_cast<f32x4*>(t + head);
  const float* sb = s + head;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4 a = tv[i], b;
    if (SVEC) {
      b = reinterpret_cast<const f32x4*>(sb)[i];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) b[e] = sb[4 * i + e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = ema_one<DECAY>(a[e], b[e], alpha, oma, keep);
    tv[i] = a;
  }
  if (blockIdx.x == 0) {  // scalar head (< 4 elements) and tail (< 4 elements): threads 0 .. 7
    const size_t tail0 = head + 4 * n4;
    const size_t k = threadIdx.x;
    if (k < head) t[k] = ema_one<DECAY>(t[k], s[k], alpha, oma, keep);
    else if (k >= 4 && tail0 + (k - 4) < n) {
      const size_t i = tail0 + (k - 4);
      t[i] = ema_one<DECAY>(t[i], s[i], alpha, oma, keep);
    }
  }
}

// weight * mean((flip(T) - softmax(b))^2) and its gradient w.r.t. b; TSOFT: T = softmax(a), else T = a.  gs = 2 weight / (M C).
template <bool TSOFT>
struct mt_mse {
  static constexpr bool kCounts = false;
  const float* a;
  const float* b;
  int C, H, W;
  const uint8_t* flags;
  float gs;
  float* db;
  __device__ double operator()(long pix, bool&) const {
    float pa[16], pb[16], g[16];
    load_pixel<0>(a + flipped_pixel(pix, H, W, flags) * C, C, pa);
    load_pixel<0>(b + pix * C, C, pb);
    const float za = TSOFT ? softmax_numerators(pa, C) : 1.f, zb = softmax_numerators(pb, C);
    double sq = 0.0;
    float sgp = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < C) {
        if (TSOFT) pa[k] /= za;
        pb[k] /= zb;
        const float d = pb[k] - pa[k];
        sq += (double)d * d;
        g[k] = gs * d;
        sgp = fmaf(g[k], pb[k], sgp);
      }
    softmax_jacobian(pb, sgp, g, C);
    store_pixel<0>(db + pix * C, C, g);
    return sq;
  }
};

// weight / M * sum_pixels -sum_c p_c log(p_c + eps);  d/dx_k = p_k (g_k - sum_c p_c g_c),
// g_c = -(log(p_c + eps) + p_c / (p_c + eps)) * gs, gs = weight / M
struct entropy_term {
  static constexpr bool kCounts = false;
  const float* x;
  int C;
  float eps, gs;
  float* dx;
  __device__ double operator()(long pix, bool&) const {
    float p[16], g[16];
    load_pixel<0>(x + pix * C, C, p);
    const float z = softmax_numerators(p, C);
    float sgp = 0.f, e = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < C) {
        p[k] /= z;
        const float q = p[k] + eps;
        const float lq = logf(q);
        e = fmaf(p[k], lq, e);
        g[k] = -(lq + p[k] / q) * gs;
        sgp = fmaf(g[k], p[k], sgp);
      }
    softmax_jacobian(p, sgp, g, C);
    store_pixel<0>(dx + pix * C, C, g);
    return -(double)e;
  }
};

// the K noisy teacher maps of spcl_ucmt_softmax_mse, by value in the kernel's argument block
struct ucmt_noisy {
  const float* p[16];
};

// weight / (M C) * sum_pixels m * sum_c (softmax(b) - softmax(flip(a)))^2, m = (u <= threshold),
// u = -sum_c q_c log(q_c + eps) / log(C), q = softmax(flip((noisy[0] + ... + noisy[K-1]) / K)); d/db_k = m * the gradient of
// mt_mse<true>, gs = 2 weight / (M C).  CT = 4: C == 4 and every map 16-byte aligned (vector accesses); CT = 0: any C <= 16.
// A kept pixel restates mt_mse<true>'s lines instead of sharing them: in the straight-line code of CT = 4 the compiler fuses
// gs * d - sgp into one multiply-add (one rounding less than mt_mse<true>, whose per-channel branches keep the two apart), so
// the two gradients are not the same bits, and each entry keeps the bits it has always returned.
template <int CT>
struct ucmt_mse {
  static constexpr bool kCounts = true;
  const float* a;
  ucmt_noisy noisy;
  int K;
  const float* b;
  int C, H, W;
  const uint8_t* flags;
  float threshold, eps, gs;
  float* db;
  uint8_t* mask;
  __device__ double operator()(long pix, bool& keep) const {
    const int CC = CT ? CT : C;
    const long aoff = flipped_pixel(pix, H, W, flags) * CC;
    {  // the mask: the f32 sum of the K maps in list order, one division, softmax, normalised entropy
      float avg[16], x[16];
      load_pixel<CT>(noisy.p[0] + aoff, CC, avg);
      // (C == 4: four maps' loads in flight at a time, 16 registers; the additions stay in list order)
#pragma clang loop unroll_count(CT == 4 ? 4 : 1)
      for (int j = 1; j < K; ++j) {
        load_pixel<CT>(noisy.p[j] + aoff, CC, x);
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (k < CC) avg[k] += x[k];
      }
      const float fk = (float)K;
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < CC) avg[k] = avg[k] / fk;
      const float zq = softmax_numerators(avg, CC);
      float e = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < CC) {
          const float q = avg[k] / zq;
          e = fmaf(q, logf(q + eps), e);
        }
      const float unc = -e / logf((float)CC);
      keep = unc <= threshold;  // (a NaN entropy keeps nothing, as torch's comparison)
    }
    if (mask) mask[pix] = keep ? 1 : 0;
    double sq = 0.0;
    float g[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) g[k] = 0.f;
    if (keep) {
      float pa[16], pb[16];
      load_pixel<CT>(a + aoff, CC, pa);
      load_pixel<CT>(b + pix * CC, CC, pb);
      const float za = softmax_numerators(pa, CC), zb = softmax_numerators(pb, CC);
      float sgp = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < CC) {
          pa[k] /= za;
          pb[k] /= zb;
          const float d = pb[k] - pa[k];
          sq += (double)d * d;
          g[k] = gs * d;
          sgp = fmaf(g[k], pb[k], sgp);
        }
      softmax_jacobian(pb, sgp, g, CC);
    }
    store_pixel<CT>(db + pix * CC, CC, g);  // exact zeros where the pixel is masked out
    return sq;
  }
};

// sample n of the virtual concatenation (a, b) of two batches of B samples, per elements each
template <typename T>
__device__ __forceinline__ const T* cat_sample(const T* a, const T* b, int n, int B, size_t per) {
  return n < B ? a + (size_t)n * per : b + (size_t)(n - B) * per;
}

// an index outside [0, N2) (the callers refuse it on the host before the copy) selects the sample itself: no read outside
// the inputs whatever the buffer holds
__device__ __forceinline__ int mix_partner(const int* __restrict__ index, int n, int N2) {
  const int j = index[n];
  return (unsigned)j < (unsigned)N2 ? j : n;
}

// fl(fl(lam * u) + fl(oml * v)): the roundings of torch's `lam * x + (1 - lam) * x[index]` on an f32 tensor.  hipcc contracts
// a product and a sum into one fused multiply-add by default (and sees through __fmul_rn / __fadd_rn, which are plain
// operators compiled under that default), which rounds twice: the pragma keeps the three operations of this block apart.
__device__ __forceinline__ float mix_one(float u, float v, float lam, float oml) {
#pragma clang fp contract(off)
  const float a = lam * u;
  const float b = oml * v;
  return a + b;
}

// blockIdx.y = output sample; VEC: per % 4 == 0 and every base pointer 16-byte aligned (then every sample is)
template <bool VEC>
__global__ void __launch_bounds__(256) mixup_images_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           const int* __restrict__ index, int B, size_t per, float lam,
                                                           float oml, float* __restrict__ out) {
  const int n = blockIdx.y, N2 = 2 * B;
  const float* u = cat_sample(a, b, n, B, per);
  const float* v = cat_sample(a, b, mix_partner(index, n, N2), B, per);
  float* o = out + (size_t)n * per;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  if (VEC) {
    const size_t per4 = per / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per4; i += stride) {
      const f32x4 x = reinterpret_cast<const f32x4*>(u)[i], y = reinterpret_cast<const f32x4*>(v)[i];
      f32x4 r;
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = mix_one(x[e], y[e], lam, oml);
      reinterpret_cast<f32x4*>(o)[i] = r;
    }
  } else {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += stride) o[i] = mix_one(u[i], v[i], lam, oml);
  }
}

// loss = weight / M * sum_pixels sum_c -t_c log((p_c + eps) / (t_c + eps)), t_c = (c == la ? lam : 0) + (c == lb ? oml : 0) with
// la the pixel's own label and lb the label of the same pixel in sample index[n];  d/dx_k = p_k (g_k - sum_c g_c p_c),
// g_c = -(weight / M) t_c / (p_c + eps), evaluated as -(weight / M) (t_k r_k - p_k sum_c t_c r_c) with r_c = p_c / (p_c + eps)
// <= 1 (the same value; no quotient by a vanishing p_c + eps is ever formed).  Labels are compared with c only.  gs = weight / M.
struct mixup_kl {
  static constexpr bool kCounts = false;
  const float* x;
  const int64_t* ya;
  const int64_t* yb;
  const int* index;
  int B, HW, C;
  float lam, oml, eps, gs;
  float* dx;
  __device__ double operator()(long pix, bool&) const {
    const int n = (int)(pix / HW), rem = (int)(pix - (long)n * HW);
    const long la = cat_sample(ya, yb, n, B, (size_t)HW)[rem];
    const long lb = cat_sample(ya, yb, mix_partner(index, n, 2 * B), B, (size_t)HW)[rem];
    float p[16], tr[16];
    load_pixel<0>(x + pix * C, C, p);
    const float z = softmax_numerators(p, C);
    float str = 0.f, e = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < C) {
        p[k] /= z;
        const float t = (k == la ? lam : 0.f) + (k == lb ? oml : 0.f);
        const float q = p[k] + eps;
        tr[k] = 0.f;
        if (t != 0.f) {  // (a class outside the target adds -0 * log(..) = 0 and no gradient)
          e = fmaf(t, logf(q / (t + eps)), e);
          tr[k] = t * (p[k] / q);
          str += tr[k];
        }
      }
    float* dp = dx + pix * C;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < C) dp[k] = -gs * (tr[k] - p[k] * str);
    return -(double)e;
  }
};

template <bool DECAY>
void launch_ema(float* t, const float* s, size_t head, size_t n4, size_t n, float alpha, float oma, float keep, bool svec,
                unsigned blocks, hipStream_t st) {
  if (svec)
    SPCL_LAUNCH((ema_update_kernel<DECAY, true>), dim3(blocks), dim3(256), 0, st, t, s, head, n4, n, alpha, oma, keep);
  else
    SPCL_LAUNCH((ema_update_kernel<DECAY, false>), dim3(blocks), dim3(256), 0, st, t, s, head, n4, n, alpha, oma, keep);
}

}  // namespace

extern "C" int spcl_ema_update(float* teacher, const float* student, size_t n, double alpha, double decay, void* stream) {
  SPCL_CHECK_ARG(teacher && student, "spcl_ema_update: null pointer");
  SPCL_CHECK_ARG(n > 0, "spcl_ema_update: empty buffer");
  SPCL_CHECK_ARG(((uintptr_t)teacher | (uintptr_t)student) % 4 == 0, "spcl_ema_update: buffers must be 4-byte aligned");
  SPCL_CHECK_ARG(alpha >= 0.0 && alpha <= 1.0 && decay >= 0.0 && decay < 1.0, "spcl_ema_update: alpha in [0, 1], decay in [0, 1)");
  const uintptr_t lo = (uintptr_t)teacher, hi = lo + n * sizeof(float), so = (uintptr_t)student;
  SPCL_CHECK_ARG(so + n * sizeof(float) <= lo || so >= hi, "spcl_ema_update: teacher and student overlap");
  size_t head = ((16 - (uintptr_t)teacher % 16) % 16) / 4;  // elements before the teacher's first 16-byte boundary
  if (head > n) head = n;
  const size_t n4 = (n - head) / 4;
  const bool svec = (uintptr_t)(student + head) % 16 == 0;
  size_t blocks = (n4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipStream_t st = (hipStream_t)stream;
  spcl::prof_cost(12.0 * (double)n, 4.0 * (double)n);
  const float af = (float)alpha, oma = (float)(1.0 - alpha), keep = (float)(1.0 - decay);
  if (decay != 0.0) launch_ema<true>(teacher, student, head, n4, n, af, oma, keep, svec, (unsigned)blocks, st);
  else launch_ema<false>(teacher, student, head, n4, n, af, oma, keep, svec, (unsigned)blocks, st);
  SPCL_LAUNCH_CHECK("ema_update_kernel");
  return SPCL_OK;
}

extern "C" size_t spcl_consistency_workspace_bytes(int N, int H, int W) { return pixel_workspace_bytes((long)N * H * W); }

// mean teacher with a soft-maxed teacher under its older name: the same launch
extern "C" int spcl_consistency_softmax_mse(const float* a, const float* b, int N, int C, int H, int W, const uint8_t* flags_a,
                                            float weight, float* loss, float* db, void* ws, size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(a && b && loss && db && ws, "spcl_consistency_softmax_mse: null pointer");
  pixel_launch p;
  if (int rc = pixel_prepare("spcl_consistency_softmax_mse", "C <= 16", N, C, H, W, ws, ws_bytes, false, stream, &p)) return rc;
  const double inv = 1.0 / ((double)p.M * C);
  spcl::prof_cost(3.0 * p.M * C * 4, 20.0 * p.M * C);
  return launch_pixel_criterion("spcl_consistency_softmax_mse", mt_mse<true>{a, b, C, H, W, flags_a, (float)(2.0 * weight * inv), db},
                                p, inv * weight, loss);
}

extern "C" size_t spcl_mt_softmax_mse_workspace_bytes(int N, int H, int W) { return pixel_workspace_bytes((long)N * H * W); }

extern "C" int spcl_mt_softmax_mse(const float* teacher, const float* student_logits, int N, int C, int H, int W,
                                   const uint8_t* flags_teacher, int teacher_mode, float weight, float* loss, float* dstudent,
                                   void* ws, size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(teacher && student_logits && loss && dstudent && ws, "spcl_mt_softmax_mse: null pointer");
  SPCL_CHECK_ARG(teacher_mode == 0 || teacher_mode == 1, "spcl_mt_softmax_mse: teacher_mode %d is neither 0 (raw) nor 1 (softmax)",
                 teacher_mode);
  pixel_launch p;
  if (int rc = pixel_prepare("spcl_mt_softmax_mse", "C <= 16", N, C, H, W, ws, ws_bytes, false, stream, &p)) return rc;
  const double inv = 1.0 / ((double)p.M * C);
  const float gs = (float)(2.0 * weight * inv);
  spcl::prof_cost(3.0 * p.M * C * 4, 20.0 * p.M * C);
  if (teacher_mode == 1)
    return launch_pixel_criterion("spcl_mt_softmax_mse", mt_mse<true>{teacher, student_logits, C, H, W, flags_teacher, gs, dstudent},
                                  p, inv * weight, loss);
  return launch_pixel_criterion("spcl_mt_softmax_mse", mt_mse<false>{teacher, student_logits, C, H, W, flags_teacher, gs, dstudent},
                                p, inv * weight, loss);
}

extern "C" size_t spcl_entropy_softmax_workspace_bytes(int N, int H, int W) { return pixel_workspace_bytes((long)N * H * W); }

extern "C" int spcl_entropy_softmax(const float* logits, int N, int C, int H, int W, float eps, float weight, float* loss,
                                    float* dlogits, void* ws, size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(logits && loss && dlogits && ws, "spcl_entropy_softmax: null pointer");
  SPCL_CHECK_ARG(eps >= 0.f, "spcl_entropy_softmax: negative eps");
  pixel_launch p;
  if (int rc = pixel_prepare("spcl_entropy_softmax", "C <= 16", N, C, H, W, ws, ws_bytes, false, stream, &p)) return rc;
  const double inv = 1.0 / (double)p.M;
  spcl::prof_cost(2.0 * p.M * C * 4, 30.0 * p.M * C);
  return launch_pixel_criterion("spcl_entropy_softmax", entropy_term{logits, C, eps, (float)((double)weight * inv), dlogits}, p,
                                inv * weight, loss);
}

extern "C" size_t spcl_ucmt_workspace_bytes(int N, int H, int W) { return pixel_workspace_bytes((long)N * H * W, true); }

extern "C" int spcl_ucmt_softmax_mse(const float* teacher, const float* const* noisy, int K, const float* student_logits, int N,
                                     int C, int H, int W, const uint8_t* flags_teacher, float threshold, float eps, float weight,
                                     float* loss, float* dstudent, unsigned long long* kept, uint8_t* mask, void* ws,
                                     size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(K >= 1 && K <= 16, "spcl_ucmt_softmax_mse: K = %d noisy maps (1 <= K <= 16)", K);
  SPCL_CHECK_ARG(teacher && noisy && student_logits && loss && dstudent && kept && ws, "spcl_ucmt_softmax_mse: null pointer");
  ucmt_noisy maps{};
  bool vec = C == 4 && ((uintptr_t)teacher | (uintptr_t)student_logits | (uintptr_t)dstudent) % 16 == 0;
  for (int j = 0; j < K; ++j) {
    SPCL_CHECK_ARG(noisy[j], "spcl_ucmt_softmax_mse: null pointer (noisy map %d)", j);
    maps.p[j] = noisy[j];
    vec = vec && (uintptr_t)noisy[j] % 16 == 0;
  }
  SPCL_CHECK_ARG(eps >= 0.f, "spcl_ucmt_softmax_mse: negative eps");
  pixel_launch p;
  if (int rc = pixel_prepare("spcl_ucmt_softmax_mse", "C <= 16", N, C, H, W, ws, ws_bytes, true, stream, &p)) return rc;
  const double inv = 1.0 / ((double)p.M * C);
  const float gs = (float)(2.0 * weight * inv);
  spcl::prof_cost((double)(K + 3) * p.M * C * 4 + (mask ? (double)p.M : 0.0), (20.0 + 2.0 * K + 20.0) * p.M * C);
  if (vec)
    return launch_pixel_criterion("spcl_ucmt_softmax_mse", ucmt_mse<4>{teacher, maps, K, student_logits, C, H, W, flags_teacher,
                                                                        threshold, eps, gs, dstudent, mask},
                                  p, inv * weight, loss, kept);
  return launch_pixel_criterion("spcl_ucmt_softmax_mse", ucmt_mse<0>{teacher, maps, K, student_logits, C, H, W, flags_teacher,
                                                                      threshold, eps, gs, dstudent, mask},
                                p, inv * weight, loss, kept);
}

extern "C" int spcl_mixup_images(const float* image, const float* image_tf, const int* index, int N2, size_t per_sample,
                                 float lam, float oml, float* out, void* stream) {
  SPCL_CHECK_ARG(image && image_tf && index && out, "spcl_mixup_images: null pointer");
  SPCL_CHECK_ARG(N2 > 0 && N2 % 2 == 0 && N2 <= 65534 && per_sample > 0, "spcl_mixup_images: bad shape (N2 = 2 B <= 65534)");
  SPCL_CHECK_ARG(((uintptr_t)image | (uintptr_t)image_tf | (uintptr_t)out) % 4 == 0,
                 "spcl_mixup_images: buffers must be 4-byte aligned");
  const int B = N2 / 2;
  const uintptr_t half = (uintptr_t)B * per_sample * sizeof(float), lo = (uintptr_t)out, hi = lo + 2 * half;
  for (const float* in : {image, image_tf})
    SPCL_CHECK_ARG((uintptr_t)in + half <= lo || (uintptr_t)in >= hi, "spcl_mixup_images: out overlaps an input");
  const bool vec = per_sample % 4 == 0 && ((uintptr_t)image | (uintptr_t)image_tf | (uintptr_t)out) % 16 == 0;
  const size_t work = vec ? per_sample / 4 : per_sample;
  size_t bx = (work + 255) / 256, cap = 2048 / (size_t)N2;  // at most 2048 workgroups of 256 in all (8 per CU), stride beyond
  if (cap < 1) cap = 1;
  if (bx > cap) bx = cap;
  hipStream_t st = (hipStream_t)stream;
  spcl::prof_cost(12.0 * (double)N2 * (double)per_sample, 3.0 * (double)N2 * (double)per_sample);
  const dim3 grid((unsigned)bx, (unsigned)N2);
  if (vec) SPCL_LAUNCH(mixup_images_kernel<true>, grid, dim3(256), 0, st, image, image_tf, index, B, per_sample, lam, oml, out);
  else SPCL_LAUNCH(mixup_images_kernel<false>, grid, dim3(256), 0, st, image, image_tf, index, B, per_sample, lam, oml, out);
  SPCL_LAUNCH_CHECK("mixup_images_kernel");
  return SPCL_OK;
}

extern "C" size_t spcl_mixup_kl_workspace_bytes(int N2, int H, int W) { return pixel_workspace_bytes((long)N2 * H * W); }

extern "C" int spcl_mixup_kl_onehot(const float* logits, const int64_t* target, const int64_t* target_tf, const int* index,
                                    int N2, int C, int H, int W, float lam, float oml, float eps, float weight, float* loss,
                                    float* dlogits, void* ws, size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(logits && target && target_tf && index && loss && dlogits && ws, "spcl_mixup_kl_onehot: null pointer");
  SPCL_CHECK_ARG(N2 % 2 == 0, "spcl_mixup_kl_onehot: bad shape (N2 = 2 B, C <= 16)");
  SPCL_CHECK_ARG(eps >= 0.f, "spcl_mixup_kl_onehot: negative eps");
  pixel_launch p;
  if (int rc = pixel_prepare("spcl_mixup_kl_onehot", "N2 = 2 B, C <= 16", N2, C, H, W, ws, ws_bytes, false, stream, &p)) return rc;
  const double inv = 1.0 / (double)p.M;
  spcl::prof_cost(2.0 * p.M * C * 4 + 16.0 * p.M, 30.0 * p.M * C);
  return launch_pixel_criterion("spcl_mixup_kl_onehot", mixup_kl{logits, target, target_tf, index, N2 / 2, H * W, C, lam, oml, eps,
                                                                 (float)((double)weight * inv), dlogits},
                                p, inv * weight, loss);
}
