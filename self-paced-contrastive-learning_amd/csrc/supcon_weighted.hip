// Weighted supervised-contrastive losses: SupConLoss2 (in / out mode), SupConLoss3 (soft pair weights) and SupConLoss4
// (block weights) of contrastyou/losses/contrast_loss.py:34-270, and their gradient -- one criterion.
//
// Over the 2n rows of z = cat(z1, z2) (unit rows), s_ij = z_i . z_j / t, a non-negative pair weight P_ij and a 0/1
// denominator switch E_ij (both 0 on the diagonal):
//     D_i = sum_j E_ij exp(s_ij)                 W_i = sum_j P_ij
//     out mode:  A_i = sum_j P_ij s_ij           loss = -mean_i [ A_i / W_i - log D_i ]
//     in  mode:  A_i = sum_j P_ij exp(s_ij)      loss = -mean_i [ log(A_i / D_i) / W_i ]
//     G_ij = d loss / d s_ij = -(1 / 2n) [ P_ij / W_i - E_ij exp(s_ij) / D_i ]                         (out mode)
//                            = -(1 / (2n W_i)) [ P_ij exp(s_ij) / A_i - E_ij exp(s_ij) / D_i ]          (in mode)
//     d loss / d z = (G + G^T) z / t
// Every exponential is taken of s_ij - m_i with a per-row constant m_i (it cancels in both forms; the reference subtracts
// the global maximum, contrast_loss.py:28-29).  A row with W_i = 0 gives 0 / 0 = NaN in out mode exactly as the reference's
// arithmetic does (:100,177,266); the Python side raises RuntimeError(loss) for it from the result block.
//
// P and E are never built as [2n, 2n] matrices: they are read by index from a label vector [n] (P = [label_u == label_v],
// E = 1; SimCLR is the label vector 0 .. n-1), or from up to three [n, n] blocks -- (1,1), (2,2) and one matrix for both
// (1,2) and (2,1), not transposed (:233-237) -- with a present bit each (E = 1 on the present blocks, P = the block's entry;
// P = E = 0 on an absent one); `mask_semantics` reads an entry w as P = [w == 1], E = [w == 0 or w == 1] (:62-66).
// u = i mod n, v = j mod n.
//
// Two schedules, chosen by size alone:
//   2n <= 64 and d <= 256 (the training sizes): one workgroup, one launch -- rows staged in LDS, S on the exact-f32 MFMA
//     (v_mfma_f32_16x16x4_f32, bitwise an fmaf chain), row statistics, the loss, and d loss / d z for a unit upstream gradient
//     left in the workspace (rows [0, 2n) x [0, d), pitch d, at its start): backward is one scaling launch;
//   above that (n <= 4096, d <= 4096): S in 64 x 64 tiles on the same MFMA, written to the workspace ([2n, 2n]); row kernels
//     in the manner of supcon_xpos.hip (one workgroup per row of S) for the statistics; S becomes G in place and stays
//     there for the backward, dz = (G + G^T) z / t, again 64 x 64 tiles on the MFMA, the contraction dealt over up to 8
//     workgroups whose partial tiles are added in order.  Four launches forward, two backward.
// All sums run in a fixed order: two runs give the same bits.
#include "common.hpp"

namespace spcl {

struct WPairs {
  const float* labels;  // [n] or null
  const float* w11;     // [n][n] block (1,1), read when blocks & 1
  const float* w22;     // block (2,2), blocks & 2
  const float* w12;     // blocks (1,2) and (2,1), blocks & 4
  int blocks, mask_sem, n;
};

// P_ij and E_ij BEFORE the diagonal is removed (what the taps show, contrast_loss.py:83-86,159-161,247-250)
__device__ __forceinline__ void wpair(const WPairs& a, int i, int j, float& p, float& e) {
  const int bi = i >= a.n ? 1 : 0, bj = j >= a.n ? 1 : 0;
  const int u = i - bi * a.n, v = j - bj * a.n;
  if (a.labels != nullptr) {
    p = a.labels[u] == a.labels[v] ? 1.f : 0.f;
    e = 1.f;
  } else {
    const int b = bi == bj ? bi : 2;
    p = e = 0.f;
    if ((a.blocks >> b) & 1) {
      const float* q = b == 0 ? a.w11 : (b == 1 ? a.w22 : a.w12);
      const float w = q[(size_t)u * a.n + v];
      if (a.mask_sem) {
        p = w == 1.f ? 1.f : 0.f;
        e = (w == 0.f || w == 1.f) ? 1.f : 0.f;
      } else {
        p = w;
        e = 1.f;
      }
    }
  }
}

// G_ij from the pair's P, E, x = exp(s_ij - m_i) and the row's statistics; kq = -1 / 2n
__device__ __forceinline__ float wgrad_entry(int in_mode, float kq, float p, float e, float x, float D, float W, float A) {
  const float den = e != 0.f ? x / D : 0.f;
  if (in_mode) return (kq / W) * ((p != 0.f ? p * x / A : 0.f) - den);
  return kq * (p / W - den);
}
__device__ __forceinline__ float wrow_loss(int in_mode, float D, float W, float A) {
  return in_mode ? logf(A / D) / W : A / W - logf(D);
}

// ------------------------------------------------------------------------------------------------ training sizes
// 16 waves on one CU: wave = (row block rb of 16 rows, column quarter cq).  Forward: the wave owns the 16 x 16 tile
// S[rb][cq]; backward: it owns dz[rb][64-feature slice cq] and reads the H = G + G^T tiles of its row block from LDS.
template <int DP>
__global__ __launch_bounds__(1024) void wsup_small_kernel(const float* __restrict__ z1, const float* __restrict__ z2,
                                                         int d, WPairs a, int in_mode, float inv_t,
                                                         float* __restrict__ out, float* __restrict__ dz_unit) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [64][DP] swizzled rows, then the exchange areas
  float* st_rn2 = lds + 64 * DP;  // [64]
  float* st_D = st_rn2 + 64;      // [64]
  float* st_W = st_D + 64;        // [64]
  float* st_A = st_W + 64;        // [64]
  float* st_rl = st_A + 64;       // [64] row losses
  float* part = st_rl + 64;       // [3][4 cq][64 rows]
  float* sx = part + 3 * 4 * 64;  // [4 rb][4 cq][4 r][64 lanes]
  const int N2 = 2 * a.n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int rb = wave & 3, cq = wave >> 2;
  const int I0 = rb * 16, i = I0 + r16;

  {  // padded rows into LDS, squared row norms: 4 rows per wave
    constexpr int KPL = DP / 64;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int row = 4 * wave + rr;
      const float* src = row < a.n ? z1 + (size_t)row * d : (row < N2 ? z2 + (size_t)(row - a.n) * d : nullptr);
      float s2 = 0.f;
#pragma unroll
      for (int q = 0; q < KPL; ++q) {
        const int k = lane + 64 * q;
        const float v = (src != nullptr && k < d) ? src[k] : 0.f;
        lds[row * DP + ((((k >> 2) ^ (row & 15)) << 2) | (k & 3))] = v;
        s2 += v * v;
      }
      s2 = wave_sum(s2);
      if (lane == 0) st_rn2[row] = s2;
    }
  }
  __syncthreads();
  const float m = wave_max(st_rn2[lane]) * inv_t;  // >= every s_ij (Cauchy-Schwarz); 1 / t for unit rows

  // the tile: c[r] = S[i][16 cq + 4 g + r]
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  {
    const float* arow = lds + (cq * 16 + r16) * DP;
    const float* brow = lds + i * DP;
#pragma unroll
    for (int s = 0; s < DP / 16; ++s) {
      const f32x4 a4 = *(const f32x4*)(arow + (((4 * s + g) ^ r16) << 2));
      const f32x4 b4 = *(const f32x4*)(brow + (((4 * s + g) ^ r16) << 2));
#pragma unroll
      for (int u = 0; u < 4; ++u) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u], b4[u], c, 0, 0, 0);
    }
  }
  float p[4], e[4], x[4];
  float accD = 0.f, accW = 0.f, accA = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = 16 * cq + 4 * g + r;
    p[r] = e[r] = 0.f;
    if (i < N2 && j < N2 && i != j) wpair(a, i, j, p[r], e[r]);
    c[r] = c[r] * inv_t - m;  // from here on c holds the shifted logits
    x[r] = expf(c[r]);
    accD += e[r] != 0.f ? x[r] : 0.f;
    accW += p[r];
    accA += p[r] != 0.f ? p[r] * (in_mode ? x[r] : c[r]) : 0.f;
  }
  accD += __shfl_xor(accD, 16, 64);
  accD += __shfl_xor(accD, 32, 64);
  accW += __shfl_xor(accW, 16, 64);
  accW += __shfl_xor(accW, 32, 64);
  accA += __shfl_xor(accA, 16, 64);
  accA += __shfl_xor(accA, 32, 64);
  if (g == 0) {
    part[cq * 64 + i] = accD;
    part[(4 + cq) * 64 + i] = accW;
    part[(8 + cq) * 64 + i] = accA;
  }
  __syncthreads();
  const float D_i = (part[i] + part[64 + i]) + (part[128 + i] + part[192 + i]);
  const float W_i = (part[256 + i] + part[320 + i]) + (part[384 + i] + part[448 + i]);
  const float A_i = (part[512 + i] + part[576 + i]) + (part[640 + i] + part[704 + i]);
  if (cq == 0 && g == 0) {
    st_D[i] = D_i;
    st_W[i] = W_i;
    st_A[i] = A_i;
    st_rl[i] = i < N2 ? wrow_loss(in_mode, D_i, W_i, A_i) : 0.f;
  }
  __syncthreads();
  if (wave == 0) {  // the scalars: 64 row losses by butterfly (fixed order)
    const float sl = wave_sum(st_rl[lane]);
    const float dm = wave_max(lane < N2 ? fabsf(sqrtf(st_rn2[lane]) - 1.f) : 0.f);
    if (lane == 0) {
      out[0] = -sl / (float)N2;
      out[1] = 1.f;
      out[2] = 1.f / (float)N2;
      out[3] = dm;  // largest | |row| - 1 |
    }
  }

  // H tile (rb, cq) = G + G^T from this wave's own logits, handed to the four waves of the row block through LDS
  const float kq = -1.f / (float)N2;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = 16 * cq + 4 * g + r;
    float hv = 0.f;
    if (i < N2 && j < N2 && i != j) {
      float pji, eji;
      wpair(a, j, i, pji, eji);
      hv = wgrad_entry(in_mode, kq, p[r], e[r], x[r], D_i, W_i, A_i) +
           wgrad_entry(in_mode, kq, pji, eji, x[r], st_D[j], st_W[j], st_A[j]);
    }
    sx[((rb * 4 + cq) * 4 + r) * 64 + lane] = hv;
  }
  __syncthreads();
  if (64 * cq >= DP) return;  // (feature slices beyond the padded width have nothing to do)
  f32x4 acc2[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc2[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    float h[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) h[r] = sx[((rb * 4 + nt) * 4 + r) * 64 + lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = nt * 16 + 4 * g + r;
      const f32x4 b4 = *(const f32x4*)(lds + row * DP + (((16 * cq + r16) ^ (row & 15)) << 2));
#pragma unroll
      for (int u = 0; u < 4; ++u) acc2[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(h[r], b4[u], acc2[u], 0, 0, 0);
    }
  }
  // acc2[u][rr] = (H z)[I0 + 4 g + rr][64 cq + 4 r16 + u]
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int row = I0 + 4 * g + rr;
    if (row >= N2) continue;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = 64 * cq + 4 * r16 + u;
      if (k < d) dz_unit[(size_t)row * d + k] = acc2[u][rr] * inv_t;
    }
  }
}

// dz = grad_out * (d loss / d z for a unit gradient)
__global__ __launch_bounds__(256) void wsup_scale_kernel(const float* __restrict__ dz_unit, int n, int d,
                                                        const float* __restrict__ grad_out, float* __restrict__ dz1,
                                                        float* __restrict__ dz2) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * n * d) return;
  const float v = dz_unit[idx] * grad_out[0];
  if (idx < n * d) dz1[idx] = v;
  else dz2[idx - n * d] = v;
}

// ------------------------------------------------------------------------------------------------ row kernels
constexpr int WSUP_MAX_D = 4096, WSUP_MAX_N = 4096;

struct WRows {
  const float* z1;
  const float* z2;
  int n, d;
  float inv_t;
};
__device__ __forceinline__ const float* wrow(const WRows& a, int i) {
  return i < a.n ? a.z1 + (size_t)i * a.d : a.z2 + (size_t)(i - a.n) * a.d;
}
__device__ __forceinline__ void wstage_row(const WRows& a, int i, float* zi) {
  const float* src = wrow(a, i);
  for (int e = threadIdx.x; e < a.d; e += 256) zi[e] = src[e];
  __syncthreads();
}
// z_i (in LDS) . z_j, for the taps (not a hot path)
__device__ __forceinline__ float wdot(const WRows& a, const float* zi, int j) {
  const float* q = wrow(a, j);
  float s = 0.f;
  for (int e = 0; e < a.d; ++e) s = fmaf(zi[e], q[e], s);
  return s;
}
static __device__ float wsum256(float v, float* red) {  // 256 threads, fixed order
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
static __device__ float wmax256(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// C tile [64 x 64] = A B^T on the exact-f32 MFMA, 4 waves: wave w owns rows 16 w .. 16 w + 15 and the tile's 64 columns (four
// accumulators); the operands go through LDS in chunks of 64 along the contraction, swizzled as in the one-workgroup kernel.
//   NN == false:  S = z z^T / t.  A = rows I0.. of z, B = rows J0.. of z, contraction over d; written to ws [2n][2n].
//   NN == true:   dz = go / t * (G + G^T) z.  A = rows I0.. of G (ws) plus columns I0.. of G, each staged with coalesced loads
//                 and added as MFMA operands; B[e][k] = z_k[J0 + e]; contraction over the 2n rows.
__device__ __forceinline__ int wswz(int k, int row) { return (((k >> 2) ^ (row & 15)) << 2) | (k & 3); }

template <bool NN>
__global__ __launch_bounds__(256) void wsup_tile_kernel(WRows a, float* __restrict__ ws, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float As[64 * 64];
  __shared__ __attribute__((aligned(16))) float Bs[64 * 64];
  __shared__ __attribute__((aligned(16))) float At[NN ? 64 * 64 : 4];  // NN: [m][k] = G[kc + k][I0 + m]
  const int n2 = 2 * a.n;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
  const int I0 = 64 * blockIdx.y, J0 = 64 * blockIdx.x;  // NN: J0 is the first feature of the tile
  const int K = NN ? n2 : a.d;
  // NN: the contraction is dealt over gridDim.z workgroups in whole chunks; their partial tiles are added in order afterwards
  const int chunks = (K + 63) / 64, cps = (chunks + (int)gridDim.z - 1) / (int)gridDim.z;
  const int c0 = cps * (int)blockIdx.z, c1 = min(chunks, c0 + cps);
  f32x4 acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int kc = 64 * c0; kc < 64 * c1; kc += 64) {
    // all loads first (clamped addresses, so that none hides behind a branch), then the stores with the padding zeros
    float va[16], vb[16], vt[NN ? 16 : 1];
    const int k = lane;
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int r = w + 4 * it;
      if constexpr (!NN) {
        const int kk = min(kc + k, a.d - 1);
        va[it] = wrow(a, min(I0 + r, n2 - 1))[kk];
        vb[it] = wrow(a, min(J0 + r, n2 - 1))[kk];
      } else {
        va[it] = ws[(size_t)min(I0 + r, n2 - 1) * n2 + min(kc + k, n2 - 1)];
        vt[it] = ws[(size_t)min(kc + r, n2 - 1) * n2 + min(I0 + k, n2 - 1)];
        vb[it] = wrow(a, min(kc + r, n2 - 1))[min(J0 + k, a.d - 1)];  // (r: row of z, k: feature)
      }
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int r = w + 4 * it;
      if constexpr (!NN) {
        const bool kin = kc + k < a.d;
        As[r * 64 + wswz(k, r)] = (I0 + r < n2 && kin) ? va[it] : 0.f;
        Bs[r * 64 + wswz(k, r)] = (J0 + r < n2 && kin) ? vb[it] : 0.f;
      } else {
        As[r * 64 + wswz(k, r)] = (I0 + r < n2 && kc + k < n2) ? va[it] : 0.f;
        At[k * 64 + wswz(r, k)] = (kc + r < n2 && I0 + k < n2) ? vt[it] : 0.f;
        Bs[k * 64 + wswz(r, k)] = (kc + r < n2 && J0 + k < a.d) ? vb[it] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      f32x4 a4 = *(const f32x4*)(As + (16 * w + r16) * 64 + (((4 * s + g) ^ r16) << 2));
      if constexpr (NN) a4 += *(const f32x4*)(At + (16 * w + r16) * 64 + (((4 * s + g) ^ r16) << 2));
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const f32x4 b4 = *(const f32x4*)(Bs + (16 * ct + r16) * 64 + (((4 * s + g) ^ r16) << 2));
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u], b4[u], acc[ct], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // acc[ct][r] = C[I0 + 16 w + 4 g + r][J0 + 16 ct + r16]
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = I0 + 16 * w + 4 * g + r, col = J0 + 16 * ct + r16;
      if (row >= n2) continue;
      if constexpr (!NN) {
        if (col < n2) ws[(size_t)row * n2 + col] = acc[ct][r] * a.inv_t;
      } else if (col < a.d) {
        part[((size_t)blockIdx.z * n2 + row) * a.d + col] = acc[ct][r];
      }
    }
}

// dz = go / t * (the partial tiles of the contraction's parts, added in order)
__global__ __launch_bounds__(256) void wsup_dz_kernel(const float* __restrict__ part, int ks, int n, int d, float inv_t,
                                                     const float* __restrict__ go, float* __restrict__ dz1,
                                                     float* __restrict__ dz2) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, half = (size_t)n * d;
  if (idx >= 2 * half) return;
  float s = part[idx];
  for (int z = 1; z < ks; ++z) s += part[(size_t)z * 2 * half + idx];
  s *= go[0] * inv_t;
  if (idx < half) dz1[idx] = s;
  else dz2[idx - half] = s;
}

// workspace of the row schedule: [2n][2n] S, then G | [2n] each: m, D, W, A, norm defect, row loss | [ks][2n][d] partial dz
// one workgroup per row of S: its maximum, D_i, W_i, A_i, the row's loss and norm defect
__global__ __launch_bounds__(256) void wsup_rowstats_kernel(WRows a, WPairs pr, int in_mode, float* __restrict__ ws) {
  __shared__ float red[4];
  const int n2 = 2 * a.n, i = blockIdx.x;
  const float* srow = ws + (size_t)i * n2;
  float* st = ws + (size_t)n2 * n2;
  const float* zi = wrow(a, i);
  float s2 = 0.f, mx = -INFINITY;
  for (int e = threadIdx.x; e < a.d; e += 256) s2 = fmaf(zi[e], zi[e], s2);
  s2 = wsum256(s2, red);
  for (int j = threadIdx.x; j < n2; j += 256) mx = fmaxf(mx, srow[j]);
  mx = wmax256(mx, red);
  float sD = 0.f, sW = 0.f, sA = 0.f;
  for (int j = threadIdx.x; j < n2; j += 256) {
    if (j == i) continue;
    float p, e;
    wpair(pr, i, j, p, e);
    const float l = srow[j] - mx, x = expf(l);
    sD += e != 0.f ? x : 0.f;
    sW += p;
    sA += p != 0.f ? p * (in_mode ? x : l) : 0.f;
  }
  sD = wsum256(sD, red);
  sW = wsum256(sW, red);
  sA = wsum256(sA, red);
  if (threadIdx.x == 0) {
    st[i] = mx;
    st[(size_t)n2 + i] = sD;
    st[2 * (size_t)n2 + i] = sW;
    st[3 * (size_t)n2 + i] = sA;
    st[4 * (size_t)n2 + i] = fabsf(sqrtf(s2) - 1.f);
    st[5 * (size_t)n2 + i] = wrow_loss(in_mode, sD, sW, sA);
  }
}

// S -> G = d loss / d S in place (each element needs only itself and its row's statistics)
__global__ __launch_bounds__(256) void wsup_g_kernel(WPairs pr, int in_mode, float* __restrict__ ws) {
  const int n2 = 2 * pr.n, i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n2) return;
  const float* st = ws + (size_t)n2 * n2;
  float gv = 0.f;
  if (i != j) {
    float p, e;
    wpair(pr, i, j, p, e);
    gv = wgrad_entry(in_mode, -1.f / (float)n2, p, e, expf(ws[(size_t)i * n2 + j] - st[i]), st[(size_t)n2 + i],
                     st[2 * (size_t)n2 + i], st[3 * (size_t)n2 + i]);
  }
  ws[(size_t)i * n2 + j] = gv;
}

__global__ __launch_bounds__(256) void wsup_finish_kernel(int n2, const float* __restrict__ ws, float* __restrict__ out) {
  __shared__ float red[4];
  const float* st = ws + (size_t)n2 * n2;
  float s = 0.f, mx = 0.f;
  for (int j = threadIdx.x; j < n2; j += 256) {
    s += st[5 * (size_t)n2 + j];
    mx = fmaxf(mx, st[4 * (size_t)n2 + j]);
  }
  s = wsum256(s, red);
  mx = wmax256(mx, red);
  if (threadIdx.x == 0) {
    out[0] = -s / (float)n2;
    out[1] = 1.f;
    out[2] = 1.f / (float)n2;
    out[3] = mx;
  }
}

// ------------------------------------------------------------------------------------------------ taps
__global__ __launch_bounds__(256) void wsup_tap_rowmax_kernel(WRows a, float* __restrict__ rowmax) {
  __shared__ __attribute__((aligned(16))) float zi[WSUP_MAX_D];
  __shared__ float red[4];
  const int n2 = 2 * a.n, i = blockIdx.x;
  wstage_row(a, i, zi);
  float mx = -INFINITY;
  for (int j = threadIdx.x; j < n2; j += 256) mx = fmaxf(mx, wdot(a, zi, j) * a.inv_t);
  mx = wmax256(mx, red);
  if (threadIdx.x == 0) rowmax[i] = mx;
}
__global__ __launch_bounds__(256) void wsup_tap_fill_kernel(WRows a, WPairs pr, const float* __restrict__ rowmax,
                                                           float* __restrict__ sim_logits, float* __restrict__ sim_exp,
                                                           float* __restrict__ pos_weight, float* __restrict__ enable) {
  __shared__ __attribute__((aligned(16))) float zi[WSUP_MAX_D];
  __shared__ float red[4];
  const int n2 = 2 * a.n, i = blockIdx.x;
  float m = 0.f;
  if (sim_logits != nullptr || sim_exp != nullptr) {
    wstage_row(a, i, zi);
    m = -INFINITY;
    for (int j = threadIdx.x; j < n2; j += 256) m = fmaxf(m, rowmax[j]);
    m = wmax256(m, red);  // the maximum of the whole matrix, diagonal included (contrast_loss.py:28)
  }
  for (int j = threadIdx.x; j < n2; j += 256) {
    const size_t o = (size_t)i * n2 + j;
    if (sim_logits != nullptr || sim_exp != nullptr) {
      const float l = wdot(a, zi, j) * a.inv_t - m;
      if (sim_logits != nullptr) sim_logits[o] = l;
      if (sim_exp != nullptr) sim_exp[o] = expf(l);
    }
    if (pos_weight != nullptr || enable != nullptr) {
      float p, e;
      wpair(pr, i, j, p, e);
      if (pos_weight != nullptr) pos_weight[o] = p;
      if (enable != nullptr) enable[o] = e;
    }
  }
}

static bool wsup_small(int n, int d) { return 2 * n <= 64 && d <= 256; }
// into how many parts the backward deals its contraction over the 2n rows: until the grid has 512 workgroups, 8 at the most
static int wsup_ksplit(int n, int d) {
  const int chunks = cdiv(2 * n, 64), tiles = chunks * cdiv(d, 64);
  int ks = 1;
  while (ks < 8 && 2 * ks <= chunks && tiles * ks < 512) ks *= 2;
  return ks;
}
}  // namespace spcl

using namespace spcl;

// floats: the schedule's own block, then [2n] scratch for the taps' row maxima
extern "C" size_t spcl_supcon_weighted_workspace_bytes(int n, int d) {
  if (n <= 0 || d <= 0 || n > WSUP_MAX_N || d > WSUP_MAX_D) return 0;
  const size_t n2 = 2 * (size_t)n;
  const size_t own = wsup_small(n, d) ? n2 * (size_t)d : n2 * n2 + 6 * n2 + (size_t)wsup_ksplit(n, d) * n2 * d;
  return (own + n2) * sizeof(float);
}

static bool wsup_pairs_ok(const float* w11, const float* w22, const float* w12, int blocks) {
  return blocks >= 0 && blocks <= 7 && (!(blocks & 1) || w11) && (!(blocks & 2) || w22) && (!(blocks & 4) || w12);
}

extern "C" int spcl_supcon_weighted_forward(const float* z1, const float* z2, const float* labels, const float* w11,
                                            const float* w22, const float* w12, int blocks, int mask_semantics,
                                            int in_mode, int n, int d, float temperature, float* ws, float* out,
                                            void* stream) {
  SPCL_CHECK_ARG(z1 && z2 && ws && out, "supcon_weighted_forward: null pointer");
  SPCL_CHECK_ARG(spcl_supcon_weighted_workspace_bytes(n, d) > 0 && temperature > 0.f,
                 "supcon_weighted_forward: n=%d d=%d temperature=%g", n, d, (double)temperature);
  SPCL_CHECK_ARG(wsup_pairs_ok(w11, w22, w12, blocks), "supcon_weighted_forward: blocks=%d names a null block", blocks);
  SPCL_CHECK_ARG(!(labels && blocks), "supcon_weighted_forward: labels and weight blocks together");
  hipStream_t st = (hipStream_t)stream;
  const WPairs pr{labels, w11, w22, w12, blocks, mask_semantics ? 1 : 0, n};
  const float inv_t = 1.f / temperature;
  in_mode = in_mode ? 1 : 0;
  if (wsup_small(n, d)) {
    const int DP = d <= 64 ? 64 : (d <= 128 ? 128 : 256);
    const size_t lds = ((size_t)64 * DP + 5 * 64 + 3 * 4 * 64 + 4 * 4 * 4 * 64) * sizeof(float);
#define SPCL_WSMALL(DP_)                                                                                            \
  do {                                                                                                              \
    if (lds > 65536) spcl::func_lds_limit((const void*)wsup_small_kernel<DP_>, (int)lds, "wsup_small_kernel");      \
    SPCL_LAUNCH((wsup_small_kernel<DP_>), dim3(1), dim3(1024), lds, st, z1, z2, d, pr, in_mode, inv_t, out, ws);    \
  } while (0)
    if (DP == 64) SPCL_WSMALL(64);
    else if (DP == 128) SPCL_WSMALL(128);
    else SPCL_WSMALL(256);
#undef SPCL_WSMALL
    SPCL_LAUNCH_CHECK("supcon_weighted_forward");
    return SPCL_OK;
  }
  const WRows a{z1, z2, n, d, inv_t};
  SPCL_LAUNCH(wsup_tile_kernel<false>, dim3(cdiv(2 * n, 64), cdiv(2 * n, 64)), dim3(256), 0, st, a, ws, (float*)nullptr);
  SPCL_LAUNCH(wsup_rowstats_kernel, dim3(2 * n), dim3(256), 0, st, a, pr, in_mode, ws);
  SPCL_LAUNCH(wsup_g_kernel, dim3(cdiv(2 * n, 256), 2 * n), dim3(256), 0, st, pr, in_mode, ws);
  SPCL_LAUNCH(wsup_finish_kernel, dim3(1), dim3(256), 0, st, 2 * n, ws, out);
  SPCL_LAUNCH_CHECK("supcon_weighted_forward");
  return SPCL_OK;
}

extern "C" int spcl_supcon_weighted_backward(const float* z1, const float* z2, int n, int d, float temperature,
                                             float* ws, const float* grad_out, float* dz1, float* dz2,
                                             void* stream) {
  SPCL_CHECK_ARG(z1 && z2 && ws && grad_out && dz1 && dz2, "supcon_weighted_backward: null pointer");
  SPCL_CHECK_ARG(spcl_supcon_weighted_workspace_bytes(n, d) > 0 && temperature > 0.f,
                 "supcon_weighted_backward: n=%d d=%d temperature=%g", n, d, (double)temperature);
  hipStream_t st = (hipStream_t)stream;
  if (wsup_small(n, d)) {
    SPCL_LAUNCH(wsup_scale_kernel, dim3(cdiv(2 * n * d, 256)), dim3(256), 0, st, ws, n, d, grad_out, dz1, dz2);
  } else {
    const WRows a{z1, z2, n, d, 1.f / temperature};
    const int ks = wsup_ksplit(n, d);
    float* part = ws + (size_t)4 * n * n + 12 * (size_t)n;
    SPCL_LAUNCH(wsup_tile_kernel<true>, dim3(cdiv(d, 64), cdiv(2 * n, 64), ks), dim3(256), 0, st, a, ws, part);
    SPCL_LAUNCH(wsup_dz_kernel, dim3((unsigned)(((size_t)2 * n * d + 255) / 256)), dim3(256), 0, st, part, ks, n, d,
                a.inv_t, grad_out, dz1, dz2);
  }
  SPCL_LAUNCH_CHECK("supcon_weighted_backward");
  return SPCL_OK;
}

extern "C" int spcl_supcon_weighted_materialize(const float* z1, const float* z2, const float* labels, const float* w11,
                                                const float* w22, const float* w12, int blocks, int mask_semantics,
                                                int n, int d, float temperature, float* ws, float* sim_logits,
                                                float* sim_exp, float* pos_weight, float* enable_mask, void* stream) {
  SPCL_CHECK_ARG(z1 && z2 && ws, "supcon_weighted_materialize: null pointer");
  const size_t bytes = spcl_supcon_weighted_workspace_bytes(n, d);
  SPCL_CHECK_ARG(bytes > 0 && temperature > 0.f, "supcon_weighted_materialize: n=%d d=%d temperature=%g", n, d,
                 (double)temperature);
  SPCL_CHECK_ARG(wsup_pairs_ok(w11, w22, w12, blocks), "supcon_weighted_materialize: blocks=%d names a null block", blocks);
  SPCL_CHECK_ARG(!(labels && blocks), "supcon_weighted_materialize: labels and weight blocks together");
  if (!sim_logits && !sim_exp && !pos_weight && !enable_mask) return SPCL_OK;
  hipStream_t st = (hipStream_t)stream;
  const WPairs pr{labels, w11, w22, w12, blocks, mask_semantics ? 1 : 0, n};
  const WRows a{z1, z2, n, d, 1.f / temperature};
  float* rowmax = ws + bytes / sizeof(float) - 2 * (size_t)n;
  if (sim_logits || sim_exp) SPCL_LAUNCH(wsup_tap_rowmax_kernel, dim3(2 * n), dim3(256), 0, st, a, rowmax);
  SPCL_LAUNCH(wsup_tap_fill_kernel, dim3(2 * n), dim3(256), 0, st, a, pr, rowmax, sim_logits, sim_exp, pos_weight,
              enable_mask);
  SPCL_LAUNCH_CHECK("supcon_weighted_materialize");
  return SPCL_OK;
}
