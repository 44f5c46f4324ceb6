// The per-pixel class-map criteria (semi_reg.hip) as one kernel skeleton, and the device pieces they share with the IIC
// kernels (iic.hip, iic_patch.hip).
//
// A criterion is a pixel functor, passed by value: one thread per pixel holds C <= 16 channels in registers, forms a softmax,
// returns the pixel's float64 loss term and writes its own gradient row (for a unit upstream gradient).  The skeleton sums
// the terms per workgroup into a double partial; the last workgroup to take a ticket adds the partials in index order and
// resets the ticket: loss and gradient are bitwise reproducible.
#pragma once
#include "common.hpp"

namespace {

__device__ __forceinline__ int flip_idx(int x, int n, bool f) { return f ? n - 1 - x : x; }

// pixel `pix` of an [N][H][W] map, seen through its sample's flips (bit 0 flips H, bit 1 flips W; no flags: no flips)
__device__ __forceinline__ long flipped_pixel(long pix, int H, int W, const uint8_t* __restrict__ flags) {
  const int n = (int)(pix / ((long)H * W));
  const int rem = (int)(pix - (long)n * H * W), u = rem / W, v = rem - u * W;
  const uint8_t f = flags ? flags[n] : 0;
  return (long)(n * H + flip_idx(u, H, f & 1)) * W + flip_idx(v, W, f & 2);
}

__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r += sh[w];
  return r;
}

// CT channels of one pixel <-> v[0 .. CT); CT == 4: one 16-byte access (the caller checked the alignment), CT == 0: C of them
template <int CT>
__device__ __forceinline__ void load_pixel(const float* __restrict__ p, int C, float (&v)[16]) {
  if (CT == 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = x[k];
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < C) v[k] = p[k];
  }
}
template <int CT>
__device__ __forceinline__ void store_pixel(float* __restrict__ p, int C, const float (&v)[16]) {
  if (CT == 4) {
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = v[k];
    *reinterpret_cast<f32x4*>(p) = o;
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < C) p[k] = v[k];
  }
}

// p[0 .. C) <- exp(p - max p), -> their sum z: softmax(p)_k = p[k] / z.  The caller forms that quotient (a true division:
// iic_common.hpp's stage_prob multiplies by one reciprocal instead, other bits) in the loop that consumes it -- divided here,
// in a loop of their own, the quotients cost mt_mse<true> 15 more VGPRs and two waves per SIMD.
__device__ __forceinline__ float softmax_numerators(float (&p)[16], int C) {
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (k < C) m = fmaxf(m, p[k]);
  float z = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (k < C) {
      p[k] = expf(p[k] - m);
      z += p[k];
    }
  return z;
}

// g <- the gradient w.r.t. the logits of a loss whose gradient w.r.t. p = softmax(logits) is g; sgp = sum_c g_c p_c
__device__ __forceinline__ void softmax_jacobian(const float (&p)[16], float sgp, float (&g)[16], int C) {
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (k < C) g[k] = p[k] * (g[k] - sgp);
}

// Workgroup `bid` of `nblk` hands in its sum `v` (and, with `counts`, its integer `cnt`); the last one to take a ticket adds
// all of them in index order: its threads fetch 256 partials at a time into shared memory (one round trip to memory per 256
// instead of one per partial), thread 0 adds them in index order -- the same sequence of double additions as a plain loop.
// That thread then stores loss = (float)(total * scale), calls done(loss, total count) and resets the ticket.  Workgroups
// of at most 256 threads.
template <class Done>
__device__ __forceinline__ void ordered_total(double v, double scale, float* __restrict__ loss, double* __restrict__ partial,
                                              unsigned int* __restrict__ ticket, unsigned int bid, unsigned int nblk,
                                              unsigned int cnt, unsigned int* __restrict__ counts, Done done) {
  __shared__ unsigned int last;
  __shared__ double stage[256];
  __shared__ unsigned int cstage[256];
  if (threadIdx.x == 0) {
    partial[bid] = v;
    if (counts) counts[bid] = cnt;
    __threadfence();
    last = atomicAdd(ticket, 1u) == nblk - 1;
  }
  __syncthreads();
  if (last) {  // (uniform over the workgroup)
    __threadfence();
    double tot = 0.0;
    unsigned long long n = 0ull;
    for (unsigned int base = 0; base < nblk; base += blockDim.x) {
      const unsigned int q = base + threadIdx.x;
      if (q < nblk) {
        stage[threadIdx.x] = *((volatile double*)partial + q);
        if (counts) cstage[threadIdx.x] = *((volatile unsigned int*)counts + q);
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        const unsigned int m = nblk - base < blockDim.x ? nblk - base : blockDim.x;
        for (unsigned int i = 0; i < m; ++i) tot += stage[i];
        if (counts)
          for (unsigned int i = 0; i < m; ++i) n += cstage[i];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const float lv = (float)(tot * scale);
      loss[0] = lv;
      done(lv, n);
      *ticket = 0u;
    }
  }
}

// ---- criteria that hand in a ROW per workgroup: ND doubles and NC unsigned ints (cross_pseudo.hip, cutmix.hip;
// pseudo_label.hip, where this protocol comes from, keeps its own copy and its bits).  Workgroups of 256 threads.
__device__ __forceinline__ double wave_butterfly_sum_d(double v) {  // every lane gets the wave's sum
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// After the workgroup has stored its row: every storing wave drains its stores, one thread releases at device scope and takes
// a ticket.  -> true in the workgroup that took the last one (uniform over the workgroup); it has fenced and may read all rows.
__device__ __forceinline__ bool rows_take_ticket(unsigned int* __restrict__ ticket, unsigned int* s_last) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    *s_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!*s_last) return false;
  __threadfence();
  return true;
}

// In the closing workgroup: ncol = ND + NC columns, G = 256 / ncol groups of R = ceil(nblk / G) consecutive rows; thread
// (group, column) adds its column over its group's rows in row order -- all of its loads independent, the whole table in flight
// at once --, then thread `col` < ncol adds the G group sums in group order and returns with its column's total in tot (col <
// ND) or n.  G and R follow from the grid and the column count alone: one fixed association.  s_gd, s_gc: 256 entries each.
//
// EXTRA (cutmix.hip): a row holds one more integer behind its NC (row pitch NC + 1) that does NOT enter the column count, so
// the groups -- and with them the association of the double sums -- stay those of the NC-column criterion; the thread of the
// last column adds it beside its own and returns its total in `extra` (s_ge: 256 entries).  Integer sums do not depend on the
// grouping.  Without EXTRA the code is what it was.
template <bool EXTRA>
__device__ __forceinline__ void rows_grouped_total_x(const double* partial, const unsigned int* counts, int ND, int NC,
                                                     double* s_gd, unsigned long long* s_gc, unsigned long long* s_ge, double& tot,
                                                     unsigned long long& n, unsigned long long& extra) {
  const int tid = threadIdx.x, nblk = (int)gridDim.x;
  const int ncol = ND + NC, G = 256 / ncol, R = (nblk + G - 1) / G;
  const int pitch = EXTRA ? NC + 1 : NC;
  const int col = tid % ncol, grp = tid / ncol;
  tot = 0.0;
  n = 0ull;
  extra = 0ull;
  if (grp < G) {
    const int r0 = grp * R, r1 = r0 + R < nblk ? r0 + R : nblk;
    if (col < ND) {
      const volatile double* src = (const volatile double*)partial + col;
#pragma unroll 8
      for (int r = r0; r < r1; ++r) tot += src[(size_t)r * ND];
    } else {
      const volatile unsigned int* src = (const volatile unsigned int*)counts + (col - ND);
#pragma unroll 8
      for (int r = r0; r < r1; ++r) n += src[(size_t)r * pitch];
      if (EXTRA && col == ncol - 1) {
#pragma unroll 8
        for (int r = r0; r < r1; ++r) extra += src[(size_t)r * pitch + 1];
      }
    }
  }
  s_gd[tid] = tot;
  s_gc[tid] = n;
  if (EXTRA) s_ge[tid] = extra;
  __syncthreads();
  if (tid < ncol) {
    tot = 0.0;
    n = 0ull;
    extra = 0ull;
    for (int g = 0; g < G; ++g) {
      tot += s_gd[g * ncol + tid];
      n += s_gc[g * ncol + tid];
      if (EXTRA) extra += s_ge[g * ncol + tid];
    }
  }
}

__device__ __forceinline__ void rows_grouped_total(const double* partial, const unsigned int* counts, int ND, int NC,
                                                   double* s_gd, unsigned long long* s_gc, double& tot, unsigned long long& n) {
  unsigned long long extra;
  rows_grouped_total_x<false>(partial, counts, ND, NC, s_gd, s_gc, nullptr, tot, n, extra);
}

// the arg-max of C <= 16 logits (strictly greater: a tie stays with the lower class)
__device__ __forceinline__ int argmax_logits(const float (&x)[16], int C) {
  int y = 0;
  float best = x[0];
#pragma unroll
  for (int k = 1; k < 16; ++k)
    if (k < C && x[k] > best) {
      best = x[k];
      y = k;
    }
  return y;
}

// one direction of the cross pseudo supervision of a kept pixel (after softmax_numerators(x) -> z; m = max x, xy = x_y taken
// BEFORE): x holds the learner's logits, y the other network's label.  -> -log softmax(x)_y, with no
// quotient that could underflow; g <- gs * (softmax(x) - onehot(y)).  Dropped: 0 and exact zeros.
template <int CT>
__device__ __forceinline__ double cross_term(float (&x)[16], float z, float m, float xy, int y, bool keep, float gs, int C,
                                             float* __restrict__ dst) {
  float g[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) g[k] = 0.f;
  double term = 0.0;
  if (keep) {
    term = (double)(logf(z) - (xy - m));
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < C) g[k] = gs * (x[k] / z - (k == y ? 1.f : 0.f));
  }
  store_pixel<CT>(dst, C, g);
  return term;
}

// grid = ceil(M / 256) workgroups of 256.  f(pix, keep) -> the pixel's term; a functor with F::kCounts also sets `keep`, and
// the number of kept pixels goes to kept[0] (an exact integer, summed like the terms).
template <class F>
__global__ void __launch_bounds__(256) pixel_criterion_kernel(const F f, long M, double scale, float* __restrict__ loss,
                                                              double* __restrict__ partial, unsigned int* __restrict__ ticket,
                                                              unsigned int* __restrict__ counts,
                                                              unsigned long long* __restrict__ kept) {
  __shared__ double sh[8];
  const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
  double term = 0.0;
  bool keep = false;
  if (pix < M) term = f(pix, keep);
  unsigned int cnt = 0u;
  if (F::kCounts) cnt = (unsigned int)block_sum_d(keep ? 1.0 : 0.0, sh);  // (at most 256: exact)
  term = block_sum_d(term, sh);
  ordered_total(term, scale, loss, partial, ticket, blockIdx.x, gridDim.x, cnt, F::kCounts ? counts : nullptr,
                [kept](float, unsigned long long n) {
                  if (F::kCounts) kept[0] = n;
                });
}

// ---------------------------------------------------------------------------------------------------------------- host
// the workspace of a criterion over M pixels: [partials: nblk doubles][ticket, 64 bytes][counts: nblk unsigned ints, if any]
struct pixel_launch {
  long M;
  int nblk;
  double* partial;
  unsigned int* ticket;
  unsigned int* counts;
  hipStream_t st;
};

inline size_t pixel_workspace_bytes(long M, bool counts = false) {
  const size_t nblk = (size_t)((M + 255) / 256);
  return nblk * sizeof(double) + 64 + (counts ? nblk * sizeof(unsigned int) : 0);
}

// what every entry does before its launch: refuse a bad shape (`hint`: what the entry's message says about it) or a small
// workspace, lay the workspace out and zero the ticket
inline int pixel_prepare(const char* name, const char* hint, int N, int C, int H, int W, void* ws, size_t ws_bytes, bool counts,
                         void* stream, pixel_launch* p) {
  SPCL_CHECK_ARG(N > 0 && H > 0 && W > 0 && C >= 1 && C <= 16, "%s: bad shape (%s)", name, hint);
  SPCL_CHECK_ARG((long)N * H * W < (1L << 31), "%s: too many pixels", name);
  p->M = (long)N * H * W;
  SPCL_CHECK_ARG(ws_bytes >= pixel_workspace_bytes(p->M, counts), "%s: workspace too small", name);
  p->nblk = (int)((p->M + 255) / 256);
  p->partial = (double*)ws;
  p->ticket = (unsigned int*)((char*)ws + (size_t)p->nblk * sizeof(double));
  p->counts = counts ? (unsigned int*)((char*)p->ticket + 64) : nullptr;
  p->st = (hipStream_t)stream;
  if (hipMemsetAsync(p->ticket, 0, sizeof(unsigned int), p->st) != hipSuccess) {
    spcl::set_error("%s: memset failed", name);
    return SPCL_ELAUNCH;
  }
  return SPCL_OK;
}

template <class F>
int launch_pixel_criterion(const char* name, const F& f, const pixel_launch& p, double scale, float* loss,
                           unsigned long long* kept = nullptr) {
  SPCL_LAUNCH(pixel_criterion_kernel<F>, dim3(p.nblk), dim3(256), 0, p.st, f, p.M, scale, loss, p.partial, p.ticket, p.counts,
              kept);
  SPCL_LAUNCH_CHECK(name);
  return SPCL_OK;
}

}  // namespace
