// Label-guided pixel contrast: an on-device class-balanced sampler of decoder cells, the gather of the chosen rows and a
// supervised-contrastive criterion whose label structure is read from the per-class counts alone.  NOT in the reference.
//
// spcl_pixel_sample      cell i (flat index b h w + y w + x) of class c = cell_label[i] in [0, C) has the key
//                          key(i) = fmix32(((i + 1) * 0x9E3779B1 mod 2^32) ^ seed)       (fmix32: MurmurHash3's finaliser)
//                        with `seed` one word read from device memory.  Both steps are bijections of 32-bit words: distinct cells
//                        have distinct keys.  Per class the min(K, n_c) cells with the smallest keys are chosen and written in
//                        ascending index order, -1 behind them.  One memset and six launches whatever the data:
//   pxs_hist_kernel<P>   P = 0 .. 3: the histogram of key byte P (most significant first) over the cells whose higher bytes equal
//                        the prefix found so far -- a radix select of the K-th smallest key of every class.  Integer atomics in
//                        LDS, then one global integer atomic per non-empty bin: the sums do not depend on the order.  Every
//                        workgroup derives the prefix of pass P from the histogram of pass P - 1 by itself (pxs_advance: one wave
//                        per class, a 64-lane scan); workgroup 0 leaves it for the next launch.
//   pxs_count_kernel     the last advance gives the K-th key T_c (2^32 - 1 when n_c <= K); a wave owns a contiguous range of
//                        cells and counts, per class, its cells with key <= T_c (ballots);
//   pxs_write_kernel     the same ranges again: a wave's first slot of a class is the sum of the counts of the waves before it,
//                        a cell's slot the popcount of the ballot below its lane -- index order without a sort.
// spcl_rows_gather_*     rows[m] = feature[idx[m]] as f32 (zero rows for idx < 0) and its transpose: one memset of the feature
//                        gradient and plain vector stores (the indices are unique).
// spcl_pixel_supcon_*    slot m = c K + j is valid iff j < count[c].  64 x 64 tiles of S = z z^T on the exact-f32 MFMA, staged
//                        and contracted as embed_monitor.hip's sweep (features in the order of the padded row whatever the tile),
//                        the matrix never stored.  A row block's column tiles are dealt to up to 8 workgroups (psc_split: a
//                        function of M alone).  Forward: each sweeps its tiles with a running maximum and a running sum per row
//                        (psc_stats_kernel); one workgroup joins the splits in split order and adds the rows' terms in double
//                        in a fixed order (psc_loss_kernel).  Backward (psc_grad_kernel): the same sweep rebuilds S with the
//                        same bits, forms W = dL/dS + dL/dS^T for the tile from the saved log-sums of its rows AND columns, and
//                        a second MFMA product adds W z_j into the row block's gradient, which lives in registers for the
//                        sweep; psc_reduce_kernel adds the splits' slabs in split order.
//                        Invalid rows are replaced by zeros while staging and every mask is a select: what they hold (NaN
//                        included) never reaches a sum, and their gradient rows are exact zeros.
// Every floating-point sum runs in a fixed order (no floating-point atomics); nothing is read back; all calls are capturable.
#include <limits.h>
#include <algorithm>
#include "common.hpp"
#include "pixel_key.hpp"

namespace spcl {

constexpr int PXC_MAX_C = 16, PXC_MAX_K = 1024, PXC_MAX_M = 4096, PXC_MAX_D = 256;
constexpr int PXS_MAX_UNITS = 1024;  // waves of the count / write launches (four per workgroup)
constexpr int PXS_HIST_WORDS = 4 * PXC_MAX_C * 256;  // (pxs_key: pixel_key.hpp, shared with cutmix.hip)

struct PxsWs {
  uint32_t* hist;     // [4][16][256], zero on entry
  uint32_t* prefix;   // [5][16]: the key bytes chosen before pass P (entry 4: the whole K-th key)
  uint32_t* krem;     // [5][16]: the rank still looked for inside the prefix; 0: the class keeps every cell (n_c < K)
  uint32_t* ncls;     // [16]: n_c
  uint32_t* unitcnt;  // [units][16]
  size_t bytes;
};
static PxsWs pxs_ws(void* ws, int units) {
  PxsWs w;
  uint32_t* p = (uint32_t*)ws;
  w.hist = p;     p += PXS_HIST_WORDS;
  w.prefix = p;   p += 5 * PXC_MAX_C;
  w.krem = p;     p += 5 * PXC_MAX_C;
  w.ncls = p;     p += PXC_MAX_C;
  w.unitcnt = p;  p += (size_t)units * PXC_MAX_C;
  w.bytes = (size_t)((char*)p - (char*)ws);
  return w;
}
// cells per wave of the count / write launches (a multiple of 64) and the number of such waves
static void pxs_units(int N, int* per, int* units) {
  const int64_t p = (((int64_t)N + PXS_MAX_UNITS - 1) / PXS_MAX_UNITS + 63) / 64 * 64;
  *per = (int)(p < 256 ? 256 : p);
  *units = (int)(((int64_t)N + *per - 1) / *per);
}

// The state before pass P (1 .. 4) from the state before pass P - 1 and that pass's histogram, for all classes, into LDS
// (spre, skrem); workgroup 0 also leaves it in the workspace.  One wave per class: lane l holds bins 4 l .. 4 l + 3.
template <int P>
__device__ __forceinline__ void pxs_advance(const PxsWs& ws, int C, int K, uint32_t* spre, uint32_t* skrem) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int c = w; c < C; c += 4) {
    const uint32_t pre = P == 1 ? 0u : ws.prefix[(P - 1) * PXC_MAX_C + c];
    const uint32_t kr = P == 1 ? (uint32_t)K : ws.krem[(P - 1) * PXC_MAX_C + c];
    const uint32_t* h = ws.hist + ((size_t)(P - 1) * PXC_MAX_C + c) * 256 + 4 * lane;
    const uint32_t b0 = h[0], b1 = h[1], b2 = h[2], b3 = h[3];
    const uint32_t s = b0 + b1 + b2 + b3;
    uint32_t incl = s;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const uint32_t up = __shfl_up(incl, m, 64);
      incl += lane >= m ? up : 0u;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    uint32_t npre = 0u, nkr = 0u;
    if (kr != 0u && total >= kr) {  // (uniform in the wave)
      const int L = __builtin_ctzll(__ballot(incl >= kr));
      uint32_t r = kr - (incl - s), bin = 4 * lane;  // (meaningful in lane L)
      if (r > b0) { r -= b0; ++bin;
        if (r > b1) { r -= b1; ++bin;
          if (r > b2) { r -= b2; ++bin; } } }
      npre = (pre << 8) | __shfl(bin, L, 64);
      nkr = __shfl(r, L, 64);
    }
    if (lane == 0) {
      spre[c] = npre;
      skrem[c] = nkr;
      if (blockIdx.x == 0) {
        ws.prefix[P * PXC_MAX_C + c] = npre;
        ws.krem[P * PXC_MAX_C + c] = nkr;
        if (P == 1) ws.ncls[c] = total;
      }
    }
  }
  __syncthreads();
}

template <int P>
__global__ __launch_bounds__(256) void pxs_hist_kernel(const int32_t* __restrict__ cell_label, int N, int C, int K,
                                                      const uint32_t* __restrict__ seedp, PxsWs ws) {
  __shared__ uint32_t h[PXC_MAX_C * 256];
  __shared__ uint32_t spre[PXC_MAX_C], skrem[PXC_MAX_C];
  for (int t = threadIdx.x; t < C * 256; t += 256) h[t] = 0u;
  if constexpr (P > 0) pxs_advance<P>(ws, C, K, spre, skrem);
  else __syncthreads();
  const uint32_t seed = *seedp;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const int c = cell_label[i];
    if ((unsigned)c >= (unsigned)C) continue;
    const uint32_t key = pxs_key((uint32_t)i, seed);
    if constexpr (P > 0)
      if (skrem[c] == 0u || (key >> (32 - 8 * P)) != spre[c]) continue;
    atomicAdd(&h[c * 256 + ((key >> (24 - 8 * P)) & 255u)], 1u);
  }
  __syncthreads();
  uint32_t* g = ws.hist + (size_t)P * PXC_MAX_C * 256;
  for (int t = threadIdx.x; t < C * 256; t += 256)
    if (h[t] != 0u) atomicAdd(&g[t], h[t]);
}

// the class of cell i if it is chosen, else -1
__device__ __forceinline__ int pxs_chosen(const int32_t* cell_label, int64_t i, int64_t end, int C, uint32_t seed,
                                          const uint32_t* thr) {
  if (i >= end) return -1;
  const int c = cell_label[i];
  if ((unsigned)c >= (unsigned)C) return -1;
  return pxs_key((uint32_t)i, seed) <= thr[c] ? c : -1;
}

__global__ __launch_bounds__(256) void pxs_count_kernel(const int32_t* __restrict__ cell_label, int N, int C, int K, int per,
                                                       const uint32_t* __restrict__ seedp, PxsWs ws,
                                                       int32_t* __restrict__ count) {
  __shared__ uint32_t spre[PXC_MAX_C], skrem[PXC_MAX_C], thr[PXC_MAX_C];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  pxs_advance<4>(ws, C, K, spre, skrem);
  if (threadIdx.x < PXC_MAX_C) {
    const int c = threadIdx.x;
    const bool all = c >= C || skrem[c] == 0u;
    thr[c] = all ? 0xFFFFFFFFu : spre[c];
    if (blockIdx.x == 0 && c < C) count[c] = all ? (int32_t)ws.ncls[c] : K;  // (all: n_c < K, or no cell at all)
  }
  __syncthreads();
  const uint32_t seed = *seedp;
  const int u = blockIdx.x * 4 + w;
  const int64_t start = (int64_t)u * per, end = start + per < N ? start + per : N;
  uint32_t cnt = 0u;  // lane c: the chosen cells of class c in this wave's range
  for (int64_t i0 = start; i0 < end; i0 += 64) {
    const int c = pxs_chosen(cell_label, i0 + lane, end, C, seed, thr);
#pragma unroll
    for (int q = 0; q < PXC_MAX_C; ++q) {
      const uint32_t n = __popcll(__ballot(c == q));
      cnt += lane == q ? n : 0u;
    }
  }
  if (lane < PXC_MAX_C) ws.unitcnt[(size_t)u * PXC_MAX_C + lane] = cnt;
}

__global__ __launch_bounds__(256) void pxs_write_kernel(const int32_t* __restrict__ cell_label, int N, int C, int K, int per,
                                                       const uint32_t* __restrict__ seedp, PxsWs ws,
                                                       const int32_t* __restrict__ count, int32_t* __restrict__ idx) {
  __shared__ uint32_t thr[PXC_MAX_C];
  __shared__ uint32_t part[16][PXC_MAX_C];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x < PXC_MAX_C) {
    const int c = threadIdx.x;
    thr[c] = (c >= C || ws.krem[4 * PXC_MAX_C + c] == 0u) ? 0xFFFFFFFFu : ws.prefix[4 * PXC_MAX_C + c];
  }
  const int u0 = blockIdx.x * 4;
  {  // the chosen cells of every class in the waves before this workgroup: 16 strided partial sums per class, then in order
    const int c = threadIdx.x & 15, p = threadIdx.x >> 4;
    uint32_t s = 0u;
    for (int v = p; v < u0; v += 16) s += ws.unitcnt[(size_t)v * PXC_MAX_C + c];
    part[p][c] = s;
  }
  __syncthreads();
  uint32_t base = 0u;  // lane c: the next free slot of class c
  if (lane < PXC_MAX_C) {
    for (int p = 0; p < 16; ++p) base += part[p][lane];
    for (int v = 0; v < w; ++v) base += ws.unitcnt[(size_t)(u0 + v) * PXC_MAX_C + lane];
  }
  const uint32_t seed = *seedp;
  const int64_t start = (int64_t)(u0 + w) * per, end = start + per < N ? start + per : N;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t i0 = start; i0 < end; i0 += 64) {
    const int c = pxs_chosen(cell_label, i0 + lane, end, C, seed, thr);
#pragma unroll
    for (int q = 0; q < PXC_MAX_C; ++q) {
      const unsigned long long m = __ballot(c == q);
      if (m == 0ull) continue;  // (uniform)
      const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)base, q);
      const uint32_t pos = b + (uint32_t)__popcll(m & below);
      if (c == q && pos < (uint32_t)K) idx[(size_t)q * K + pos] = (int32_t)(i0 + lane);
      base += lane == q ? (uint32_t)__popcll(m) : 0u;
    }
  }
  if (blockIdx.x == 0)  // the slots behind the chosen cells (disjoint from the stores above)
    for (int t = threadIdx.x; t < C * K; t += 256) {
      const int c = t / K;
      if (t - c * K >= count[c]) idx[t] = -1;
    }
}

// ------------------------------------------------------------------------------------------------ gather / scatter of rows
template <typename T, int V>
__global__ __launch_bounds__(256) void pxg_forward_kernel(const T* __restrict__ feat, int ncells, int Cf, int64_t cs,
                                                         const int32_t* __restrict__ idx, int M, float* __restrict__ rows) {
  const int G = Cf / V;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)M * G) return;
  const int m = (int)(t / G), q = (int)(t - (int64_t)m * G);
  const int i = idx[m];
  const bool real = i >= 0 && i < ncells;  // (anything else: a zero row)
  const T* src = feat + (size_t)(real ? i : 0) * cs + (size_t)q * V;
  float* dst = rows + (size_t)m * Cf + (size_t)q * V;
  if constexpr (V == 4) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (real) {
      if constexpr (sizeof(T) == 4) {
        v = *(const f32x4*)src;
      } else {
        const s16x4 x = *(const s16x4*)src;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = bf16_to_f32((bf16_t)x[e]);
      }
    }
    *(f32x4*)dst = v;
  } else {
    dst[0] = real ? Elem<T>::load(src) : 0.f;
  }
}

template <typename T, int V>
__global__ __launch_bounds__(256) void pxg_backward_kernel(const float* __restrict__ drows, const int32_t* __restrict__ idx, int M,
                                                          int Cf, T* __restrict__ dfeat, int ncells, int64_t cs) {
  const int G = Cf / V;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)M * G) return;
  const int m = (int)(t / G), q = (int)(t - (int64_t)m * G);
  const int i = idx[m];
  if (i < 0 || i >= ncells) return;
  const float* src = drows + (size_t)m * Cf + (size_t)q * V;
  T* dst = dfeat + (size_t)i * cs + (size_t)q * V;
  if constexpr (V == 4 && sizeof(T) == 4) {
    *(f32x4*)dst = *(const f32x4*)src;
  } else if constexpr (V == 4) {
    const f32x4 x = *(const f32x4*)src;
    s16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (short)f32_to_bf16(x[e]);
    *(s16x4*)dst = o;
  } else {
    Elem<T>::store(dst, src[0]);
  }
}

// ------------------------------------------------------------------------------------------------ the criterion
constexpr int PSC_MAX_SPLIT = 8;
constexpr int PSC_WP = 68;  // row pitch of the W tile in LDS (the MFMA layout's writes and the operand reads are conflict-free)

__device__ __forceinline__ float psc_row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
  return v;
}

// slot m's class and whether it is valid (cnt: the counts in LDS, clamped to [0, K], zero behind C)
__device__ __forceinline__ bool psc_slot(int m, int M, int K, const int* cnt, int* cls) {
  const int c = m / K;
  *cls = c;
  return m < M && m - c * K < cnt[c < PXC_MAX_C ? c : PXC_MAX_C - 1];
}

// 64 rows x 64 features of z into LDS, swizzled in 16-byte groups as embed_monitor.hip's tiles; rows that are invalid or past
// M and features past d are zeros (a select: an invalid row's content is never loaded)
__device__ __forceinline__ void psc_stage(float* dst, const float* __restrict__ z, int d, int M, int K, const int* cnt, int row0,
                                          int kc) {
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int idx = threadIdx.x + 256 * it, r = idx >> 4, q = idx & 15;
    const int row = row0 + r, col = kc + 4 * q;
    int cls;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (psc_slot(row, M, K, cnt, &cls) && col < d) v = *(const f32x4*)(z + (size_t)row * d + col);
    *(f32x4*)(dst + r * 64 + ((q ^ (r & 15)) << 2)) = v;
  }
}
// one 64-feature chunk: acc[c] += A rows 16 w .. x B rows 16 c ..; the ONE statement of the contraction order of S
__device__ __forceinline__ void psc_mma(const float* As, const float* Bs, int w, int r16, int g, f32x4 (&acc)[4]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const f32x4 a4 = *(const f32x4*)(As + (16 * w + r16) * 64 + (((4 * s + g) ^ r16) << 2));
    f32x4 b4[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) b4[c] = *(const f32x4*)(Bs + (16 * c + r16) * 64 + (((4 * s + g) ^ r16) << 2));
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u], b4[c][u], acc[c], 0, 0, 0);
  }
}
// S[I0 .. I0 + 63][J0 .. J0 + 63]: acc[c][r] = S[16 w + 4 g + r][16 c + r16].  Leaves the LAST feature chunk of the column
// rows in Bs.  The caller puts a barrier between the last reader of As / Bs and the call.
__device__ __forceinline__ void psc_tile(float* As, float* Bs, const float* __restrict__ z, int d, int DP, int M, int K,
                                         const int* cnt, int I0, int J0, int w, int r16, int g, f32x4 (&acc)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int kc = 0; kc < DP; kc += 64) {
    if (kc > 0) __syncthreads();
    psc_stage(As, z, d, M, K, cnt, I0, kc);
    psc_stage(Bs, z, d, M, K, cnt, J0, kc);
    __syncthreads();
    psc_mma(As, Bs, w, r16, g, acc);
  }
}

// |I|: the valid rows whose class has a second sample
__device__ __forceinline__ int psc_anchors(const int* cnt, int C) {
  int n = 0;
  for (int c = 0; c < C; ++c) n += cnt[c] >= 2 ? cnt[c] : 0;
  return n;
}

// into how many column splits a row block's sweep is dealt: until the grid has 256 workgroups, 8 at the most (a function of M
// alone: the association of every sum is fixed by the shape)
static int psc_split(int M) {
  const int rb = cdiv(M, 64);
  int cs = 1;
  while (cs < PSC_MAX_SPLIT && 2 * cs <= rb && rb * cs < 256) cs *= 2;
  return cs;
}

struct PscWs {
  float* lse;  // [MP] the rows' log-sums (0 outside I)
  float* pm;   // [CS][MP] per column split: the running maximum,
  float* pse;  // [CS][MP] the sum of exp(t - maximum),
  float* pps;  // [CS][MP] the sum of the positives' logits
  float* pdz;  // [CS][MP][d] per column split: the unscaled gradient
  size_t bytes;
};
static PscWs psc_ws(const void* ws, int M, int d) {
  const size_t MP = round_up(M, 64), CS = psc_split(M);
  PscWs w;
  float* p = (float*)ws;
  w.lse = p;  p += MP;
  w.pm = p;   p += CS * MP;
  w.pse = p;  p += CS * MP;
  w.pps = p;  p += CS * MP;
  w.pdz = p;  p += CS * MP * d;
  w.bytes = (size_t)((char*)p - (char*)ws);
  return w;
}

__global__ __launch_bounds__(256) void psc_stats_kernel(const float* __restrict__ z, const int32_t* __restrict__ count, int M,
                                                       int K, int C, int d, float invT, int tps, float* __restrict__ pm,
                                                       float* __restrict__ pse, float* __restrict__ pps) {
  __shared__ __attribute__((aligned(16))) float As[64 * 64];
  __shared__ __attribute__((aligned(16))) float Bs[64 * 64];
  __shared__ int cnt[PXC_MAX_C];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
  if (threadIdx.x < PXC_MAX_C) cnt[threadIdx.x] = threadIdx.x < C ? min(max(count[threadIdx.x], 0), K) : 0;
  __syncthreads();
  const int I0 = 64 * blockIdx.x, DP = ((d + 63) & ~63), MP = (M + 63) & ~63;
  int ci[4];  // the rows' classes (an invalid row's sums are never read)
  float mx[4], se[4], ps[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    ci[r] = (I0 + 16 * w + 4 * g + r) / K;
    mx[r] = -INFINITY;
    se[r] = 0.f;
    ps[r] = 0.f;
  }
  const int t0 = blockIdx.y * tps, t1 = min(MP / 64, t0 + tps);
  for (int t = t0; t < t1; ++t) {
    const int J0 = 64 * t;
    f32x4 acc[4];
    if (t > t0) __syncthreads();
    psc_tile(As, Bs, z, d, DP, M, K, cnt, I0, J0, w, r16, g, acc);
    int cj[4];
    bool vj[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) vj[c] = psc_slot(J0 + 16 * c + r16, M, K, cnt, &cj[c]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = I0 + 16 * w + 4 * g + r;
      float t[4];
      bool ok[4];
      float tmax = -INFINITY;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        ok[c] = vj[c] && (J0 + 16 * c + r16 != i);
        t[c] = acc[c][r] * invT;
        tmax = ok[c] ? fmaxf(tmax, t[c]) : tmax;
      }
      tmax = row16_max(tmax);
      const float mn = fmaxf(mx[r], tmax);
      if (mn > -INFINITY) {
        float s = mx[r] > -INFINITY ? se[r] * expf(mx[r] - mn) : 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          s += ok[c] ? expf(t[c] - mn) : 0.f;
          ps[r] += (ok[c] && cj[c] == ci[r]) ? t[c] : 0.f;
        }
        se[r] = s;
        mx[r] = mn;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float tot = psc_row16_sum(se[r]), pst = psc_row16_sum(ps[r]);
    const size_t o = (size_t)blockIdx.y * MP + I0 + 16 * w + 4 * g + r;
    if (r16 == 0) {  // (an empty split leaves -inf, 0, 0; what an invalid row leaves is selected away by the close)
      pm[o] = mx[r];
      pse[o] = tot;
      pps[o] = pst;
    }
  }
}

// one workgroup: the splits' row statistics joined in split order, the rows' log-sums left for the backward call, the rows'
// terms added in double (per thread in row order, wave butterfly, the four waves in order)
__global__ __launch_bounds__(256) void psc_loss_kernel(const float* __restrict__ pm, const float* __restrict__ pse,
                                                      const float* __restrict__ pps, const int32_t* __restrict__ count, int M,
                                                      int K, int C, int CS, float* __restrict__ lse, float* __restrict__ loss) {
  __shared__ double red[4];
  __shared__ int cnt[PXC_MAX_C];
  if (threadIdx.x < PXC_MAX_C) cnt[threadIdx.x] = threadIdx.x < C ? min(max(count[threadIdx.x], 0), K) : 0;
  __syncthreads();
  const int MP = (M + 63) & ~63;
  double s = 0.0;
  for (int i = threadIdx.x; i < MP; i += 256) {
    int ci;
    const bool valid = psc_slot(i, M, K, cnt, &ci);
    const int np = valid ? cnt[ci] - 1 : 0;
    const bool anchor = valid && np >= 1;
    float m = -INFINITY;
    for (int c = 0; c < CS; ++c) m = fmaxf(m, pm[(size_t)c * MP + i]);
    float se = 0.f, ps = 0.f;
    for (int c = 0; c < CS; ++c) {
      const float mc = pm[(size_t)c * MP + i];
      se += mc > -INFINITY ? pse[(size_t)c * MP + i] * expf(mc - m) : 0.f;
      ps += pps[(size_t)c * MP + i];
    }
    const float l = anchor ? m + logf(se) : 0.f;
    lse[i] = l;
    s += anchor ? (double)(l - ps / (float)np) : 0.0;
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nI = psc_anchors(cnt, C);
    loss[0] = nI > 0 ? (float)(((red[0] + red[1]) + (red[2] + red[3])) / (double)nI) : 0.f;
  }
}

__global__ __launch_bounds__(256) void psc_grad_kernel(const float* __restrict__ z, const int32_t* __restrict__ count, int M,
                                                      int K, int C, int d, float invT, int tps, const float* __restrict__ lse,
                                                      float* __restrict__ pdz) {
  __shared__ __attribute__((aligned(16))) float As[64 * 64];
  __shared__ __attribute__((aligned(16))) float Bs[64 * 64];
  __shared__ float Ws[64 * PSC_WP];
  __shared__ int cnt[PXC_MAX_C];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
  if (threadIdx.x < PXC_MAX_C) cnt[threadIdx.x] = threadIdx.x < C ? min(max(count[threadIdx.x], 0), K) : 0;
  __syncthreads();
  const int I0 = 64 * blockIdx.x, DP = ((d + 63) & ~63), MP = (M + 63) & ~63;
  const int nI = psc_anchors(cnt, C);
  const float coef = nI > 0 ? invT / (float)nI : 0.f;
  int ci[4];
  bool vi[4], ai[4];
  float lsi[4], ipi[4];  // the row's log-sum and 1 / |P(i)|
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = I0 + 16 * w + 4 * g + r;
    vi[r] = psc_slot(i, M, K, cnt, &ci[r]);
    const int np = vi[r] ? cnt[ci[r]] - 1 : 0;
    ai[r] = vi[r] && np >= 1;
    ipi[r] = ai[r] ? 1.f / (float)np : 0.f;
    lsi[r] = lse[i];
  }
  f32x4 dacc[4][4];  // [feature chunk][16-feature tile]: dz[16 w + 4 g + r][64 fc + 16 ft + r16]
#pragma unroll
  for (int fc = 0; fc < 4; ++fc)
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) dacc[fc][ft] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int t0 = blockIdx.y * tps, t1 = min(MP / 64, t0 + tps);
  for (int t = t0; t < t1; ++t) {
    const int J0 = 64 * t;
    f32x4 acc[4];
    if (t > t0) __syncthreads();
    psc_tile(As, Bs, z, d, DP, M, K, cnt, I0, J0, w, r16, g, acc);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = J0 + 16 * c + r16;
      int cj;
      const bool vj = psc_slot(j, M, K, cnt, &cj);
      const int npj = vj ? cnt[cj < PXC_MAX_C ? cj : 0] - 1 : 0;
      const bool aj = vj && npj >= 1;
      const float ipj = aj ? 1.f / (float)npj : 0.f;
      const float lj = lse[j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = I0 + 16 * w + 4 * g + r;
        const bool ok = vi[r] && vj && i != j;
        const bool same = ci[r] == cj;
        const float t = acc[c][r] * invT;
        const float gi = ai[r] ? expf(t - lsi[r]) - (same ? ipi[r] : 0.f) : 0.f;
        const float gj = aj ? expf(t - lj) - (same ? ipj : 0.f) : 0.f;
        Ws[(16 * w + 4 * g + r) * PSC_WP + 16 * c + r16] = ok ? coef * (gi + gj) : 0.f;
      }
    }
    // dz[I0 ..] += W z[J0 ..]: A = the W tile (k = the column j), B = the column rows, one feature chunk at a time
#pragma unroll
    for (int fc = 0; fc < 4; ++fc) {
      if (64 * fc >= DP) continue;  // (uniform)
      __syncthreads();              // W complete; the S product is through with Bs
      if (DP > 64) {                // (d <= 64: Bs still holds the whole rows)
        psc_stage(Bs, z, d, M, K, cnt, J0, 64 * fc);
        __syncthreads();
      }
#pragma unroll 4
      for (int ks = 0; ks < 16; ++ks) {
        const int jj = 4 * ks + g;
        const float a = Ws[(16 * w + r16) * PSC_WP + jj];
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
          const int f = 16 * ft + r16;
          const float b = Bs[jj * 64 + ((((f >> 2) ^ (jj & 15)) << 2) | (f & 3))];
          dacc[fc][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, dacc[fc][ft], 0, 0, 0);
        }
      }
    }
  }
  float* out = pdz + (size_t)blockIdx.y * MP * d;  // this split's slab (an empty split stores zeros)
#pragma unroll
  for (int fc = 0; fc < 4; ++fc)
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = I0 + 16 * w + 4 * g + r, f = 64 * fc + 16 * ft + r16;
        if (i < M && f < d) out[(size_t)i * d + f] = vi[r] ? dacc[fc][ft][r] : 0.f;
      }
}

// dz = gscale * the splits' slabs added in split order, four features per thread
__global__ __launch_bounds__(256) void psc_reduce_kernel(const float* __restrict__ pdz, int M, int d, int MP, int CS,
                                                        const float* __restrict__ gscale, float* __restrict__ dz) {
  const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e >= (size_t)M * d) return;
  f32x4 s = *(const f32x4*)(pdz + e);
  for (int c = 1; c < CS; ++c) {
    const f32x4 v = *(const f32x4*)(pdz + (size_t)c * MP * d + e);
    s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
  }
  const float gs = gscale != nullptr ? gscale[0] : 1.f;
  *(f32x4*)(dz + e) = (f32x4){s[0] * gs, s[1] * gs, s[2] * gs, s[3] * gs};
}

}  // namespace spcl

using namespace spcl;

static bool pxs_shape_ok(int N, int C, int K) {
  return N >= 1 && C >= 2 && C <= PXC_MAX_C && K >= 1 && K <= PXC_MAX_K && C * K <= PXC_MAX_M;
}

extern "C" size_t spcl_pixel_sample_workspace_bytes(int ncells) {
  if (ncells < 1) return 0;
  int per, units;
  pxs_units(ncells, &per, &units);
  return pxs_ws(nullptr, round_up(units, 4)).bytes;
}

extern "C" int spcl_pixel_sample(const int32_t* cell_label, int ncells, int C, int K, const uint32_t* seed, int32_t* idx,
                                 int32_t* count, void* ws, size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(pxs_shape_ok(ncells, C, K),
                 "spcl_pixel_sample: %d cells (1 .. 2^31 - 1), C = %d (2 .. %d), K = %d (1 .. %d), C K = %d (<= %d)", ncells, C,
                 PXC_MAX_C, K, PXC_MAX_K, C * K, PXC_MAX_M);
  SPCL_CHECK_ARG(cell_label && seed && idx && count && ws, "spcl_pixel_sample: null pointer");
  SPCL_CHECK_ARG((uintptr_t)ws % 4 == 0, "spcl_pixel_sample: misaligned workspace");
  int per, units;
  pxs_units(ncells, &per, &units);
  const int blocks = cdiv(units, 4);
  const PxsWs w = pxs_ws(ws, 4 * blocks);
  SPCL_CHECK_ARG(ws_bytes >= w.bytes, "spcl_pixel_sample: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(w.hist, 0, PXS_HIST_WORDS * sizeof(uint32_t), st) != hipSuccess) {
    (void)hipGetLastError();
    set_error("spcl_pixel_sample: memset failed");
    return SPCL_ELAUNCH;
  }
  const int hb = (int)std::min<int64_t>(((int64_t)ncells + 1023) / 1024, 512);
  SPCL_LAUNCH(pxs_hist_kernel<0>, dim3(hb), dim3(256), 0, st, cell_label, ncells, C, K, seed, w);
  SPCL_LAUNCH(pxs_hist_kernel<1>, dim3(hb), dim3(256), 0, st, cell_label, ncells, C, K, seed, w);
  SPCL_LAUNCH(pxs_hist_kernel<2>, dim3(hb), dim3(256), 0, st, cell_label, ncells, C, K, seed, w);
  SPCL_LAUNCH(pxs_hist_kernel<3>, dim3(hb), dim3(256), 0, st, cell_label, ncells, C, K, seed, w);
  SPCL_LAUNCH(pxs_count_kernel, dim3(blocks), dim3(256), 0, st, cell_label, ncells, C, K, per, seed, w, count);
  SPCL_LAUNCH(pxs_write_kernel, dim3(blocks), dim3(256), 0, st, cell_label, ncells, C, K, per, seed, w, (const int32_t*)count,
              idx);
  SPCL_LAUNCH_CHECK("spcl_pixel_sample");
  return SPCL_OK;
}

static bool pxg_vec4(const void* p, int dtype, int Cf, int64_t cs) {
  return Cf % 4 == 0 && cs % 4 == 0 && (uintptr_t)p % (dtype == SPCL_F32 ? 16 : 8) == 0;
}

extern "C" int spcl_rows_gather_forward(const void* feat, int dtype, int ncells, int Cf, int64_t cs, const int32_t* idx, int M,
                                        float* rows, void* stream) {
  SPCL_CHECK_ARG(dtype == SPCL_F32 || dtype == SPCL_BF16, "spcl_rows_gather_forward: dtype %d", dtype);
  SPCL_CHECK_ARG(ncells >= 1 && Cf >= 1 && cs >= Cf && M >= 1, "spcl_rows_gather_forward: %d cells, %d channels, pitch %ld, %d rows",
                 ncells, Cf, (long)cs, M);
  SPCL_CHECK_ARG(feat && idx && rows, "spcl_rows_gather_forward: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = pxg_vec4(feat, dtype, Cf, cs) && (uintptr_t)rows % 16 == 0;
  const int64_t threads = (int64_t)M * (v4 ? Cf / 4 : Cf);
  const dim3 grid((unsigned)((threads + 255) / 256));
  if (dtype == SPCL_F32) {
    if (v4) SPCL_LAUNCH((pxg_forward_kernel<float, 4>), grid, dim3(256), 0, st, (const float*)feat, ncells, Cf, cs, idx, M, rows);
    else SPCL_LAUNCH((pxg_forward_kernel<float, 1>), grid, dim3(256), 0, st, (const float*)feat, ncells, Cf, cs, idx, M, rows);
  } else {
    if (v4) SPCL_LAUNCH((pxg_forward_kernel<bf16_t, 4>), grid, dim3(256), 0, st, (const bf16_t*)feat, ncells, Cf, cs, idx, M, rows);
    else SPCL_LAUNCH((pxg_forward_kernel<bf16_t, 1>), grid, dim3(256), 0, st, (const bf16_t*)feat, ncells, Cf, cs, idx, M, rows);
  }
  SPCL_LAUNCH_CHECK("spcl_rows_gather_forward");
  return SPCL_OK;
}

extern "C" int spcl_rows_gather_backward(const float* drows, const int32_t* idx, int M, int Cf, void* dfeat, int dtype, int ncells,
                                         int64_t cs, void* stream) {
  SPCL_CHECK_ARG(dtype == SPCL_F32 || dtype == SPCL_BF16, "spcl_rows_gather_backward: dtype %d", dtype);
  SPCL_CHECK_ARG(ncells >= 1 && Cf >= 1 && cs >= Cf && M >= 1, "spcl_rows_gather_backward: %d cells, %d channels, pitch %ld, %d rows",
                 ncells, Cf, (long)cs, M);
  SPCL_CHECK_ARG(drows && idx && dfeat, "spcl_rows_gather_backward: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(dfeat, 0, (size_t)ncells * cs * (dtype == SPCL_F32 ? 4 : 2), st) != hipSuccess) {
    (void)hipGetLastError();
    set_error("spcl_rows_gather_backward: memset failed");
    return SPCL_ELAUNCH;
  }
  const bool v4 = pxg_vec4(dfeat, dtype, Cf, cs) && (uintptr_t)drows % 16 == 0;
  const int64_t threads = (int64_t)M * (v4 ? Cf / 4 : Cf);
  const dim3 grid((unsigned)((threads + 255) / 256));
  if (dtype == SPCL_F32) {
    if (v4) SPCL_LAUNCH((pxg_backward_kernel<float, 4>), grid, dim3(256), 0, st, drows, idx, M, Cf, (float*)dfeat, ncells, cs);
    else SPCL_LAUNCH((pxg_backward_kernel<float, 1>), grid, dim3(256), 0, st, drows, idx, M, Cf, (float*)dfeat, ncells, cs);
  } else {
    if (v4) SPCL_LAUNCH((pxg_backward_kernel<bf16_t, 4>), grid, dim3(256), 0, st, drows, idx, M, Cf, (bf16_t*)dfeat, ncells, cs);
    else SPCL_LAUNCH((pxg_backward_kernel<bf16_t, 1>), grid, dim3(256), 0, st, drows, idx, M, Cf, (bf16_t*)dfeat, ncells, cs);
  }
  SPCL_LAUNCH_CHECK("spcl_rows_gather_backward");
  return SPCL_OK;
}

static bool psc_shape_ok(int C, int K, int d, float t) {
  return C >= 2 && C <= PXC_MAX_C && K >= 1 && K <= PXC_MAX_K && C * K <= PXC_MAX_M && d >= 4 && d <= PXC_MAX_D && d % 4 == 0 &&
         t > 0.f;
}

extern "C" size_t spcl_pixel_supcon_workspace_bytes(int M, int d) {
  if (M < 1 || M > PXC_MAX_M || d < 4 || d > PXC_MAX_D || d % 4 != 0) return 0;
  return psc_ws(nullptr, M, d).bytes;
}

extern "C" int spcl_pixel_supcon_forward(const float* z, const int32_t* count, int C, int K, int d, float t, float* loss, void* ws,
                                         size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(psc_shape_ok(C, K, d, t),
                 "spcl_pixel_supcon_forward: C = %d (2 .. %d), K = %d (1 .. %d), C K = %d (<= %d), d = %d (4 .. %d, a multiple "
                 "of 4), t = %g (> 0)", C, PXC_MAX_C, K, PXC_MAX_K, C * K, PXC_MAX_M, d, PXC_MAX_D, (double)t);
  SPCL_CHECK_ARG(z && count && loss && ws, "spcl_pixel_supcon_forward: null pointer");
  SPCL_CHECK_ARG((uintptr_t)z % 16 == 0 && (uintptr_t)ws % 16 == 0, "spcl_pixel_supcon_forward: misaligned rows or workspace");
  const int M = C * K, MP = round_up(M, 64), CS = psc_split(M), tps = cdiv(MP / 64, CS);
  const PscWs w = psc_ws(ws, M, d);
  SPCL_CHECK_ARG(ws_bytes >= w.bytes, "spcl_pixel_supcon_forward: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
  hipStream_t st = (hipStream_t)stream;
  prof_cost((double)MP * MP / 64 * round_up(d, 64) * 8.0, 2.0 * MP * MP * round_up(d, 64));
  SPCL_LAUNCH(psc_stats_kernel, dim3(MP / 64, CS), dim3(256), 0, st, z, count, M, K, C, d, 1.f / t, tps, w.pm, w.pse, w.pps);
  SPCL_LAUNCH(psc_loss_kernel, dim3(1), dim3(256), 0, st, (const float*)w.pm, (const float*)w.pse, (const float*)w.pps, count, M,
              K, C, CS, w.lse, loss);
  SPCL_LAUNCH_CHECK("spcl_pixel_supcon_forward");
  return SPCL_OK;
}

extern "C" int spcl_pixel_supcon_backward(const float* z, const int32_t* count, int C, int K, int d, float t, const float* gscale,
                                          void* ws, size_t ws_bytes, float* dz, void* stream) {
  SPCL_CHECK_ARG(psc_shape_ok(C, K, d, t),
                 "spcl_pixel_supcon_backward: C = %d (2 .. %d), K = %d (1 .. %d), C K = %d (<= %d), d = %d (4 .. %d, a multiple "
                 "of 4), t = %g (> 0)", C, PXC_MAX_C, K, PXC_MAX_K, C * K, PXC_MAX_M, d, PXC_MAX_D, (double)t);
  SPCL_CHECK_ARG(z && count && ws && dz, "spcl_pixel_supcon_backward: null pointer");
  SPCL_CHECK_ARG((uintptr_t)z % 16 == 0 && (uintptr_t)ws % 16 == 0 && (uintptr_t)dz % 16 == 0,
                 "spcl_pixel_supcon_backward: misaligned rows, workspace or gradient");
  const int M = C * K, MP = round_up(M, 64), CS = psc_split(M), tps = cdiv(MP / 64, CS);
  const PscWs w = psc_ws(ws, M, d);
  SPCL_CHECK_ARG(ws_bytes >= w.bytes, "spcl_pixel_supcon_backward: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
  hipStream_t st = (hipStream_t)stream;
  prof_cost((double)MP * MP / 64 * round_up(d, 64) * 12.0, 4.0 * MP * MP * round_up(d, 64));
  SPCL_LAUNCH(psc_grad_kernel, dim3(MP / 64, CS), dim3(256), 0, st, z, count, M, K, C, d, 1.f / t, tps, (const float*)w.lse, w.pdz);
  SPCL_LAUNCH(psc_reduce_kernel, dim3(cdiv(M * d / 4, 256)), dim3(256), 0, st, (const float*)w.pdz, M, d, MP, CS, gscale, dz);
  SPCL_LAUNCH_CHECK("spcl_pixel_supcon_backward");
  return SPCL_OK;
}
