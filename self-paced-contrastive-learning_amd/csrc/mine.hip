// The two ends of the MINE statistics network (semi_seg/mi_estimator/mineestimator.py:19-36) that no other kernel of the
// library covers:
//   pairs   the network's two inputs, cat(feat1, feat2) and cat(feat1, roll(feat2)) (mineestimator.py:33-35), feat2 the first
//           half of the extracted feature seen through the batch's flips (semi_seg/epochers/_mixins.py:79-86): both written from
//           the feature itself, no flipped or rolled tensor in between; the backward is one gather
//   head    AdaptiveMaxPool2d((1, 1)) -> Flatten -> Linear(C / 2, 1) -> softplus -> mean of both passes
//           (mineestimator.py:27-29,34-35) in one launch, and its backward in one launch
// Every sum has a fixed order; no floating-point atomics.
#include "common.hpp"

#include <limits.h>

namespace spcl {

// V consecutive elements of T moved as one access (V * sizeof(T) == 16 on the wide path, V == 1 on the scalar one)
template <typename T, int V> struct alignas(sizeof(T) * V) MnPack {
  T v[V];
};

__device__ __forceinline__ int mn_flip(int i, int n, int on) { return on ? n - 1 - i : i; }

// one thread per V channels of one output pixel; C, Cs, C2s in elements (the wide path: all multiples of V)
template <typename T, int V>
__global__ __launch_bounds__(256) void mine_pairs_fwd_kernel(const T* __restrict__ feat, const uint8_t* __restrict__ flags, int n,
                                                             int H, int W, int C, int Cs, int C2s, T* __restrict__ joint,
                                                             T* __restrict__ marg, long total) {
  typedef MnPack<T, V> P;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;  // (pixel, chunk), chunk fastest
  if (e >= total) return;
  const int cpr = C2s / V;
  const long pix = e / cpr;
  const int c = (int)(e - pix * cpr) * V;
  const int w = (int)(pix % W), h = (int)((pix / W) % H), i = (int)(pix / ((long)W * H));
  P vj, vm;
#pragma unroll
  for (int k = 0; k < V; ++k) vj.v[k] = vm.v[k] = (T)0;  // pad channels
  if (c < C) {
    vj = vm = *(const P*)(feat + (((long)(n + i) * H + h) * W + w) * Cs + c);
  } else if (c < 2 * C) {
    const int im = i + 1 == n ? 0 : i + 1;
    const int fj = flags != nullptr ? flags[i] & 3 : 0, fm = flags != nullptr ? flags[im] & 3 : 0;
    vj = *(const P*)(feat + (((long)i * H + mn_flip(h, H, fj & 1)) * W + mn_flip(w, W, fj & 2)) * Cs + (c - C));
    vm = *(const P*)(feat + (((long)im * H + mn_flip(h, H, fm & 1)) * W + mn_flip(w, W, fm & 2)) * Cs + (c - C));
  }
  *(P*)(joint + pix * C2s + c) = vj;
  *(P*)(marg + pix * C2s + c) = vm;
}

// one thread per V channels of one pixel of dfeat [2n][H][W][Cs]
template <typename T, int V>
__global__ __launch_bounds__(256) void mine_pairs_bwd_kernel(const T* __restrict__ dj, const T* __restrict__ dm,
                                                             const uint8_t* __restrict__ flags, int n, int H, int W, int C, int Cs,
                                                             int C2s, T* __restrict__ dfeat, long total) {
  typedef MnPack<T, V> P;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int cpr = Cs / V;
  const long pix = e / cpr;
  const int c = (int)(e - pix * cpr) * V;
  const int w = (int)(pix % W), h = (int)((pix / W) % H), r = (int)(pix / ((long)W * H));
  P o;
#pragma unroll
  for (int k = 0; k < V; ++k) o.v[k] = (T)0;
  if (c < C) {
    P a, b;
    if (r >= n) {  // feat1: the first C channels of both maps, same sample, same pixel
      const long at = (((long)(r - n) * H + h) * W + w) * C2s + c;
      a = *(const P*)(dj + at);
      b = *(const P*)(dm + at);
    } else {  // feat2: read through the sample's own flip (its own inverse); the roll sends sample r to row r - 1 of marg
      const int f = flags != nullptr ? flags[r] & 3 : 0, rm = r == 0 ? n - 1 : r - 1;
      const int sh = mn_flip(h, H, f & 1), sw = mn_flip(w, W, f & 2);
      a = *(const P*)(dj + (((long)r * H + sh) * W + sw) * C2s + C + c);
      b = *(const P*)(dm + (((long)rm * H + sh) * W + sw) * C2s + C + c);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) Elem<T>::store(&o.v[k], Elem<T>::load(&a.v[k]) + Elem<T>::load(&b.v[k]));  // f32 sum, one rounding
  }
  *(P*)(dfeat + pix * Cs + c) = o;
}

// is (v, iv) the maximum rather than (best, ib)?  The larger value, the smaller index among equals; a NaN beats every number
// (nn.AdaptiveMaxPool2d propagates it), the first NaN beats a later one.
__device__ __forceinline__ bool mn_better(float v, int iv, float best, int ib) {
  const bool vn = v != v, bn = best != best;
  if (vn || bn) return vn && (!bn || iv < ib);
  return v > best || (v == best && iv < ib);
}

__device__ __forceinline__ float mn_softplus(float t) { return fmaxf(t, 0.f) + log1pf(expf(-fabsf(t))); }
__device__ __forceinline__ float mn_sigmoid(float t) {
  const float ex = expf(-fabsf(t));
  return t >= 0.f ? 1.f / (1.f + ex) : ex / (1.f + ex);
}

constexpr int kMnSlab = 256;  // pixels per workgroup of the head's forward
constexpr int kMnRowBuf = 8 * 257;  // floats of shared memory for the (pass, sample) rows the last workgroup finishes at a time
constexpr int kMnRowMax = 128;

// one workgroup per (pass, sample, slab of kMnSlab pixels): thread t reads channel t % cs of the slab's pixels t / cs +
// j * (256 / cs) -- consecutive threads read consecutive addresses --, the 256 / cs threads of a channel are folded through
// shared memory and the slab's (maximum, index) per channel goes to the workspace.  The workgroup that takes the last ticket
// folds the slabs in index order, forms the 2 n logits (an FMA chain in channel order each) and adds the softplus terms in
// index order in double.
template <typename T>
__global__ __launch_bounds__(256) void mine_head_fwd_kernel(const T* __restrict__ act_j, const T* __restrict__ act_m, int n, int HW,
                                                            int CH, int cs, int nsplit, const float* __restrict__ w,
                                                            const float* __restrict__ b, float* tout, float* mx, int* arg,
                                                            float* __restrict__ loss, float* pmax, int* parg,
                                                            unsigned int* __restrict__ ticket) {
  __shared__ float smax[256];
  __shared__ int sarg[256];
  __shared__ float srow[kMnRowBuf];  // rows of CH + 1 floats (odd stride: the threads of the logit chains read different banks)
  __shared__ float ssp[kMnRowMax];
  __shared__ unsigned int last;
  const int t = threadIdx.x, blk = blockIdx.x / nsplit, sp = blockIdx.x - blk * nsplit, pass = blk / n, i = blk - pass * n;
  const T* a = (pass ? act_m : act_j) + (long)i * HW * cs;
  const int S = 256 / cs, s = t / cs, c = t - s * cs;
  const int p0 = sp * kMnSlab, p1 = p0 + kMnSlab < HW ? p0 + kMnSlab : HW;
  float best = -INFINITY;
  int ib = INT_MAX;
  if (s < S) {
    for (int p = p0 + s; p < p1; p += S) {
      const float v = Elem<T>::load(a + (long)p * cs + c);
      if (mn_better(v, p, best, ib)) {
        best = v;
        ib = p;
      }
    }
  }
  smax[t] = best;
  sarg[t] = ib;
  __syncthreads();
  if (t < CH) {  // (s == 0, c == t)
    for (int j = 1; j < S; ++j) {
      const float v = smax[j * cs + t];
      const int iv = sarg[j * cs + t];
      if (mn_better(v, iv, best, ib)) {
        best = v;
        ib = iv;
      }
    }
    pmax[((long)blk * nsplit + sp) * CH + t] = best;
    parg[((long)blk * nsplit + sp) * CH + t] = ib;
    __threadfence();
  }
  __syncthreads();
  if (t == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  __syncthreads();
  if (!last) return;  // (uniform over the workgroup)
  __threadfence();
  // the last workgroup: as many (pass, sample) rows at a time as fit (8 at CH = 256, up to 128 for narrow maps) -- fold the slabs of every (row, channel) in slab order, then
  // one thread per row runs the logit's FMA chain from shared memory, then thread 0 adds the rows' softplus terms in order
  const volatile float* vmax = pmax;
  const volatile int* varg = parg;
  double sj = 0.0, sm = 0.0;
  const int stride = CH + 1, fit = kMnRowBuf / stride, rmax = fit < kMnRowMax ? fit : kMnRowMax;
  for (int k0 = 0; k0 < 2 * n; k0 += rmax) {
    const int rows = 2 * n - k0 < rmax ? 2 * n - k0 : rmax;
    for (int e = t; e < rows * CH; e += 256) {
      const int r = e / CH, ch = e - r * CH;
      const long at = (long)(k0 + r) * nsplit;
      float bv = -INFINITY;
      int bi = INT_MAX;
      int q = 0;
      for (; q + 4 <= nsplit; q += 4) {  // four slabs' loads in flight, compared in slab order
        float v[4];
        int iv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          v[u] = vmax[(at + q + u) * CH + ch];
          iv[u] = varg[(at + q + u) * CH + ch];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (mn_better(v[u], iv[u], bv, bi)) {
            bv = v[u];
            bi = iv[u];
          }
        }
      }
      for (; q < nsplit; ++q) {
        const float v = vmax[(at + q) * CH + ch];
        const int iv = varg[(at + q) * CH + ch];
        if (mn_better(v, iv, bv, bi)) {
          bv = v;
          bi = iv;
        }
      }
      mx[(long)(k0 + r) * CH + ch] = bv;
      arg[(long)(k0 + r) * CH + ch] = bi;
      srow[r * stride + ch] = bv;
    }
    __syncthreads();
    if (t < rows) {
      float tv = b[0];
      for (int ch = 0; ch < CH; ++ch) tv = fmaf(w[ch], srow[t * stride + ch], tv);
      tout[k0 + t] = tv;
      ssp[t] = mn_softplus(tv);
    }
    __syncthreads();
    if (t == 0) {
      for (int r = 0; r < rows; ++r) {
        if (k0 + r < n) sj += (double)ssp[r];
        else sm += (double)ssp[r];
      }
    }
  }
  if (t != 0) return;
  loss[0] = (float)(sm / (double)n + sj / (double)n);
  *ticket = 0u;
}

// one thread per element of the two dense activation gradients (w_c dt at the argmax, 0 elsewhere and in the pad channels); one
// more workgroup, the last, adds dw and db over (pass, sample) in index order
template <typename T>
__global__ __launch_bounds__(256) void mine_head_bwd_kernel(const float* __restrict__ tin, const float* __restrict__ mx,
                                                            const int* __restrict__ arg, const float* __restrict__ w,
                                                            const float* __restrict__ grad, int n, int HW, int CH, int cs,
                                                            T* __restrict__ dact_j, T* __restrict__ dact_m, float* __restrict__ dw,
                                                            float* __restrict__ db, long per_pass) {
  const float gs = (grad != nullptr ? grad[0] : 1.f) / (float)n;
  if (blockIdx.x == gridDim.x - 1) {
    const int c = threadIdx.x;
    if (c < CH && dw != nullptr) {
      float acc = 0.f;
      for (int k = 0; k < 2 * n; ++k) acc = fmaf(mn_sigmoid(tin[k]) * gs, mx[(long)k * CH + c], acc);
      dw[c] = acc;
    }
    if (c == 0 && db != nullptr) {
      float acc = 0.f;
      for (int k = 0; k < 2 * n; ++k) acc += mn_sigmoid(tin[k]) * gs;
      db[0] = acc;
    }
    return;
  }
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * per_pass) return;
  const int pass = e >= per_pass;
  const long r = e - (pass ? per_pass : 0);  // ((i, p), c), c fastest
  const int c = (int)(r % cs);
  const long ip = r / cs;
  const int p = (int)(ip % HW), i = (int)(ip / HW), k = pass * n + i;
  float v = 0.f;
  if (c < CH && arg[(long)k * CH + c] == p) v = w[c] * (mn_sigmoid(tin[k]) * gs);
  Elem<T>::store((pass ? dact_m : dact_j) + r, v);
}

static bool mn_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static int mn_ru16(int c) { return (c + 15) / 16 * 16; }

template <typename T, int V>
static void mn_launch_pairs_fwd(const void* feat, const uint8_t* flags, int n, int H, int W, int C, void* joint, void* marg,
                                hipStream_t st) {
  const int Cs = mn_ru16(C), C2s = mn_ru16(2 * C);
  const long total = (long)n * H * W * (C2s / V);
  SPCL_LAUNCH((mine_pairs_fwd_kernel<T, V>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const T*)feat, flags, n, H, W,
              C, Cs, C2s, (T*)joint, (T*)marg, total);
}

template <typename T, int V>
static void mn_launch_pairs_bwd(const void* dj, const void* dm, const uint8_t* flags, int n, int H, int W, int C, void* dfeat,
                                hipStream_t st) {
  const int Cs = mn_ru16(C), C2s = mn_ru16(2 * C);
  const long total = 2L * n * H * W * (Cs / V);
  SPCL_LAUNCH((mine_pairs_bwd_kernel<T, V>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const T*)dj, (const T*)dm,
              flags, n, H, W, C, Cs, C2s, (T*)dfeat, total);
}

static int mn_pairs_check(const char* who, const void* a, const void* b, const void* c, int dtype, int n, int H, int W, int C) {
  SPCL_CHECK_ARG(a && b && c, "%s: null pointer", who);
  SPCL_CHECK_ARG(dtype == SPCL_F32 || dtype == SPCL_BF16, "%s: dtype %d", who, dtype);
  SPCL_CHECK_ARG(n > 0 && H > 0 && W > 0 && C > 0, "%s: n, H, W, C > 0 (got %d, %d, %d, %d)", who, n, H, W, C);
  SPCL_CHECK_ARG(C <= (1 << 20) && 2L * n * H * W * mn_ru16(2 * C) < (1L << 38), "%s: too large", who);
  return SPCL_OK;
}

static int mn_head_check(const char* who, int dtype, int n, int H, int W, int C) {
  SPCL_CHECK_ARG(dtype == SPCL_F32 || dtype == SPCL_BF16, "%s: dtype %d", who, dtype);
  SPCL_CHECK_ARG(n > 0 && n <= (1 << 20) && H > 0 && W > 0 && (long)H * W < (1L << 24), "%s: n, H, W > 0 (got %d, %d, %d)", who, n,
                 H, W);
  SPCL_CHECK_ARG(C >= 2 && C % 2 == 0, "%s: an even channel count (got %d)", who, C);
  SPCL_CHECK_ARG(C / 2 <= 256, "%s: at most 256 pooled channels (got %d)", who, C / 2);
  SPCL_CHECK_ARG(2L * n * H * W * mn_ru16(C / 2) < (1L << 38), "%s: too large", who);
  return SPCL_OK;
}

}  // namespace spcl

using namespace spcl;

extern "C" int spcl_mine_pairs_forward(const void* feat, const uint8_t* flags, int dtype, int n, int H, int W, int C, void* joint,
                                       void* marg, void* stream) {
  if (int rc = mn_pairs_check("mine_pairs_forward", feat, joint, marg, dtype, n, H, W, C)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool wide = C % 16 == 0 && mn_aligned16(feat) && mn_aligned16(joint) && mn_aligned16(marg);
  if (dtype == SPCL_F32) {
    if (wide) mn_launch_pairs_fwd<float, 4>(feat, flags, n, H, W, C, joint, marg, st);
    else mn_launch_pairs_fwd<float, 1>(feat, flags, n, H, W, C, joint, marg, st);
  } else {
    if (wide) mn_launch_pairs_fwd<bf16_t, 8>(feat, flags, n, H, W, C, joint, marg, st);
    else mn_launch_pairs_fwd<bf16_t, 1>(feat, flags, n, H, W, C, joint, marg, st);
  }
  SPCL_LAUNCH_CHECK("mine_pairs_forward");
  return SPCL_OK;
}

extern "C" int spcl_mine_pairs_backward(const void* djoint, const void* dmarg, const uint8_t* flags, int dtype, int n, int H, int W,
                                        int C, void* dfeat, void* stream) {
  if (int rc = mn_pairs_check("mine_pairs_backward", djoint, dmarg, dfeat, dtype, n, H, W, C)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool wide = C % 16 == 0 && mn_aligned16(djoint) && mn_aligned16(dmarg) && mn_aligned16(dfeat);
  if (dtype == SPCL_F32) {
    if (wide) mn_launch_pairs_bwd<float, 4>(djoint, dmarg, flags, n, H, W, C, dfeat, st);
    else mn_launch_pairs_bwd<float, 1>(djoint, dmarg, flags, n, H, W, C, dfeat, st);
  } else {
    if (wide) mn_launch_pairs_bwd<bf16_t, 8>(djoint, dmarg, flags, n, H, W, C, dfeat, st);
    else mn_launch_pairs_bwd<bf16_t, 1>(djoint, dmarg, flags, n, H, W, C, dfeat, st);
  }
  SPCL_LAUNCH_CHECK("mine_pairs_backward");
  return SPCL_OK;
}

extern "C" size_t spcl_mine_head_workspace_bytes(int n, int H, int W, int C) {
  if (n <= 0 || n > (1 << 20) || H <= 0 || W <= 0 || (long)H * W >= (1L << 24) || C < 2 || C % 2 != 0 || C / 2 > 256) return 0;
  const size_t slabs = (size_t)2 * n * cdiv(H * W, kMnSlab);
  return 64 + slabs * (C / 2) * (sizeof(float) + sizeof(int));
}

extern "C" int spcl_mine_head_forward(const void* act_joint, const void* act_marg, int dtype, int n, int H, int W, int C,
                                      const float* w, const float* b, float* t, float* maxima, int* argmax, float* loss, void* ws,
                                      size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(act_joint && act_marg && w && b && t && maxima && argmax && loss && ws, "mine_head_forward: null pointer");
  if (int rc = mn_head_check("mine_head_forward", dtype, n, H, W, C)) return rc;
  SPCL_CHECK_ARG(ws_bytes >= spcl_mine_head_workspace_bytes(n, H, W, C), "mine_head_forward: workspace of %zu bytes",
                 spcl_mine_head_workspace_bytes(n, H, W, C));
  SPCL_CHECK_ARG(((uintptr_t)ws & 3u) == 0, "mine_head_forward: 4-byte aligned workspace");
  const int nsplit = cdiv(H * W, kMnSlab);
  SPCL_CHECK_ARG(2L * n * nsplit < (1L << 31), "mine_head_forward: too large");
  hipStream_t st = (hipStream_t)stream;
  unsigned int* ticket = (unsigned int*)ws;
  float* pmax = (float*)((char*)ws + 64);
  int* parg = (int*)(pmax + (size_t)2 * n * nsplit * (C / 2));
  if (hipMemsetAsync(ticket, 0, sizeof(unsigned int), st) != hipSuccess) {
    spcl::set_error("mine_head_forward: memset failed");
    return SPCL_ELAUNCH;
  }
  const int CH = C / 2, cs = mn_ru16(CH);
  if (dtype == SPCL_F32) {
    SPCL_LAUNCH(mine_head_fwd_kernel<float>, dim3((unsigned)(2 * n * nsplit)), dim3(256), 0, st, (const float*)act_joint,
                (const float*)act_marg, n, H * W, CH, cs, nsplit, w, b, t, maxima, argmax, loss, pmax, parg, ticket);
  } else {
    SPCL_LAUNCH(mine_head_fwd_kernel<bf16_t>, dim3((unsigned)(2 * n * nsplit)), dim3(256), 0, st, (const bf16_t*)act_joint,
                (const bf16_t*)act_marg, n, H * W, CH, cs, nsplit, w, b, t, maxima, argmax, loss, pmax, parg, ticket);
  }
  SPCL_LAUNCH_CHECK("mine_head_forward");
  return SPCL_OK;
}

extern "C" int spcl_mine_head_backward(const float* t, const float* maxima, const int* argmax, const float* w, const float* grad,
                                       int dtype, int n, int H, int W, int C, void* dact_joint, void* dact_marg, float* dw,
                                       float* db, void* stream) {
  SPCL_CHECK_ARG(t && maxima && argmax && w && dact_joint && dact_marg, "mine_head_backward: null pointer");
  if (int rc = mn_head_check("mine_head_backward", dtype, n, H, W, C)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int CH = C / 2, cs = mn_ru16(CH);
  const long per_pass = (long)n * H * W * cs;
  const unsigned grid = (unsigned)((2 * per_pass + 255) / 256) + 1u;
  if (dtype == SPCL_F32) {
    SPCL_LAUNCH(mine_head_bwd_kernel<float>, dim3(grid), dim3(256), 0, st, t, maxima, argmax, w, grad, n, H * W, CH, cs,
                (float*)dact_joint, (float*)dact_marg, dw, db, per_pass);
  } else {
    SPCL_LAUNCH(mine_head_bwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, t, maxima, argmax, w, grad, n, H * W, CH, cs,
                (bf16_t*)dact_joint, (bf16_t*)dact_marg, dw, db, per_pass);
  }
  SPCL_LAUNCH_CHECK("mine_head_backward");
  return SPCL_OK;
}
