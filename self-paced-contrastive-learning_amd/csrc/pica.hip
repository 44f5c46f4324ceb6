// PICA (partition confidence / partition-uncertainty-index) criteria: contrastyou/losses/pica_loss.py of the reference,
// PUILoss (:9-38) and PUISegLoss (:41-84), which PICALossWrapper (semi_seg/utils.py:242-263) plugs into the cluster heads
// of the IIC criteria (iic.hip).
//
// Dense (PUISegLoss): the displacement joint J[s][dy][dx][i][j] is iic.hip's (spcl_iic_joint_forward leaves it as 32.32
// fixed-point words, spcl_iic_joint_backward turns dJ into d(logits)); only the criterion between the two is new.  With
// q = J - min(J) + 1e-16 (the min of the whole subhead, detached), s_t = sum_ab q_t,ab and t running over the T^2
// displacements, the symmetrised mean joint has the diagonal Pbar_ii = (1/T^2) sum_t q_t,ii / s_t and
//   ce = -(1/K^2) sum_i log(Pbar_ii + 1e-16),   g_i = -1 / (K^2 (Pbar_ii + 1e-16)),   c_t = sum_i g_i q_t,ii / s_t,
//   d ce / d J_t,ab = ((a == b ? g_a : 0) - c_t) / (T^2 s_t).
// dJ needs Pbar of the whole subhead, so ONE workgroup takes a subhead and walks its displacements (at most 225 x 1024
// words: next to the joint launches this is nothing); no workgroup waits for another.  The balance term of pica_loss.py:76-77
// is a constant of the shape (its mean runs over the class axis of the permuted map: every entry is 1/K), handed in by the
// host as lamda * ne.
//
// Global (PUILoss): logits rows [N][ld], subhead s in columns s*K .. s*K+K-1; a workgroup per subhead makes two passes over
// the rows (32 at a time through LDS, any N): first A = x^T y, the column norms and the column means, then -- with
// C_ij = A_ij / (a_i b_j), G = (softmax_rows(C) - I) / K, M_ij = G_ij / (a_i b_j), u_i = sum_j G_ij C_ij, w_j = sum_i G_ij C_ij --
//   d / d x_nk = sum_j M_kj y_nj - x_nk u_k / a_k^2 + lamda (log p_k + 1) / N,    d / d y_nj = sum_i M_ij x_ni - y_nj w_j / b_j^2
// followed by the grouped-softmax backward.  (A column whose norm is below F.normalize's 1e-12 clamp is divided by the clamp:
// its u / w term is dropped, as autograd does.)  log p_k carries no epsilon, as in the reference.
//
// Everything from the joint (the softmax probabilities) on is float64 with sums in a fixed order; the subheads' terms are
// added in index order by the workgroup that finishes last (nobody reads that sum inside the launch): bitwise reproducible.
#include "common.hpp"
#include "iic_common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 32;  // logits rows staged per pass of the global criterion
constexpr int kKP = 32;    // cluster pitch in LDS (K <= 32)

__device__ __forceinline__ double jval(const long long* jacc, const float* jf, long e) {
  return jacc ? (double)jacc[e] / kFix : (double)jf[e];
}

__device__ __forceinline__ double wave_sum_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Subhead `s` of `S` hands in its ce and its ce + lamda * ne; the workgroup that takes the last ticket adds them in index
// order, stores loss = scale * sum total, ce_out = scale * sum ce, and resets the ticket.  partial: [2][S] doubles.
__device__ __forceinline__ void subhead_total(double ce, double total, double scale, int s, int S, float* __restrict__ loss,
                                              float* __restrict__ ce_out, double* __restrict__ partial,
                                              unsigned int* __restrict__ ticket) {
  if (threadIdx.x != 0) return;
  partial[s] = ce;
  partial[S + s] = total;
  __threadfence();
  if (atomicAdd(ticket, 1u) != (unsigned int)S - 1u) return;
  __threadfence();
  double tc = 0.0, tt = 0.0;
  for (int q = 0; q < S; ++q) {
    tc += *((volatile double*)partial + q);
    tt += *((volatile double*)partial + S + q);
  }
  loss[0] = (float)(tt * scale);
  if (ce_out) ce_out[0] = (float)(tc * scale);
  *ticket = 0u;
}

// ------------------------------------------------------------------------------------------------------------ dense
// grid (S), 256 threads; dynamic LDS (doubles): [T*T] 1 / s_t, [T*T] c_t, [32] g, [32] log terms, [8][32] partial Pbar, [8]
// reductions.  Divisions and logarithms in float64 are long instruction sequences: none is left to a single thread's loop.
__global__ void __launch_bounds__(kThreads) pica_seg_kernel(const long long* __restrict__ jacc, const float* __restrict__ jf,
                                                            int S, int K, int T, double lamda_ne, float scale,
                                                            float* __restrict__ jout, float* __restrict__ loss,
                                                            float* __restrict__ ce_out, float* __restrict__ djout,
                                                            double* __restrict__ partial, unsigned int* __restrict__ ticket) {
  extern __shared__ double sd[];
  const int TT = T * T;
  double* sS = sd;
  double* sC = sd + TT;
  double* sG = sd + 2 * TT;
  double* sLg = sG + kKP;
  double* sPart = sLg + kKP;
  double* sh = sPart + (kThreads / kKP) * kKP;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long KK = (long)K * K, sub = (long)s * TT * KK;
  double mn = INFINITY;
  for (long e = tid; e < TT * KK; e += kThreads) {
    const double a = jval(jacc, jf, sub + e);
    if (jout && jacc) jout[sub + e] = (float)a;
    mn = fmin(mn, a);
  }
  const double shift = 1e-16 - block_min_d(mn, sh);
  // 1 / s_t: a wave per displacement, lanes strided over its K^2 entries
  for (int t = wave; t < TT; t += kThreads / 64) {
    double z = 0.0;
    for (int e = lane; e < KK; e += 64) z += jval(jacc, jf, sub + t * KK + e) + shift;
    z = wave_sum_d(z);
    if (lane == 0) sS[t] = 1.0 / z;
  }
  __syncthreads();
  {  // Pbar_ii: thread (part, i) adds the displacements part, part + 8, ...; the 8 parts are then added in order
    const int i = tid % kKP, part = tid / kKP;
    double pb = 0.0;
    if (i < K)
      for (int t = part; t < TT; t += kThreads / kKP) pb += (jval(jacc, jf, sub + t * KK + (long)i * K + i) + shift) * sS[t];
    sPart[part * kKP + i] = pb;
  }
  __syncthreads();
  if (tid < K) {
    double pb = 0.0;
    for (int part = 0; part < kThreads / kKP; ++part) pb += sPart[part * kKP + tid];
    pb /= (double)TT;
    sLg[tid] = log(pb + 1e-16);
    sG[tid] = -1.0 / ((double)KK * (pb + 1e-16));
  }
  __syncthreads();
  double ce = 0.0;
  if (tid == 0) {
    for (int i = 0; i < K; ++i) ce -= sLg[i];
    ce /= (double)KK;
  }
  for (int t = tid; t < TT; t += kThreads) {
    double c = 0.0;
    for (int i = 0; i < K; ++i) c += sG[i] * (jval(jacc, jf, sub + t * KK + (long)i * K + i) + shift);
    sC[t] = c * sS[t];
  }
  __syncthreads();
  const double coef = (double)scale / (double)TT;
  for (long e = tid; e < TT * KK; e += kThreads) {
    const int t = (int)(e / KK), r = (int)(e - t * KK), a = r / K, b = r - a * K;
    djout[sub + e] = (float)(((a == b ? sG[a] : 0.0) - sC[t]) * (coef * sS[t]));
  }
  subhead_total(ce, ce + lamda_ne, (double)scale, s, S, loss, ce_out, partial, ticket);
}

// ------------------------------------------------------------------------------------------------------------ global
// stage rows r0 .. r0 + nr - 1 of both maps as probabilities, pitch kKP
__device__ __forceinline__ void stage_rows(const float* __restrict__ lx, const float* __restrict__ ly, long ld, int r0, int nr,
                                           int s, int K, float* sX, float* sY) {
  for (int q = threadIdx.x; q < 2 * nr; q += kThreads) {
    const int r = q >> 1;
    if (q & 1)
      stage_prob<kKP>(ly, ld, 1, 1, r0 + r, 0, 0, s, K, sY + r * kKP);
    else
      stage_prob<kKP>(lx, ld, 1, 1, r0 + r, 0, 0, s, K, sX + r * kKP);
  }
}

// grid (S), 256 threads
__global__ void __launch_bounds__(kThreads) pica_global_kernel(const float* __restrict__ lx, const float* __restrict__ ly,
                                                               long ld, int N, int S, int K, double lamda, float scale,
                                                               const float* __restrict__ gscale, float* __restrict__ loss,
                                                               float* __restrict__ ce_out, float* __restrict__ dlx,
                                                               float* __restrict__ dly, double* __restrict__ partial,
                                                               unsigned int* __restrict__ ticket) {
  __shared__ __attribute__((aligned(16))) float sX[kRows * kKP];
  __shared__ __attribute__((aligned(16))) float sY[kRows * kKP];
  __shared__ double sGr[2][kRows * kKP];  // the gradient w.r.t. the probabilities of the staged rows (X, Y)
  __shared__ double sDot[2][kRows];       // sum_k g_k p_k of a staged row
  __shared__ double sM[kKP * kKP];        // C, then M
  __shared__ double sE[kKP * kKP];        // exp(C)
  __shared__ double sA[kKP], sB[kKP], sP[kKP], sU[kKP], sW[kKP], sZ[kKP], sL[2 * kKP];
  const int s = blockIdx.x, tid = threadIdx.x;
  // ---- pass 1: A = x^T y, squared column norms, column sums
  double acc[4] = {0.0, 0.0, 0.0, 0.0}, n2 = 0.0, cs = 0.0;
  for (int r0 = 0; r0 < N; r0 += kRows) {
    const int nr = min(kRows, N - r0);
    __syncthreads();
    stage_rows(lx, ly, ld, r0, nr, s, K, sX, sY);
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int e = tid + a * kThreads, i = e / kKP, j = e % kKP;
      if (i < K && j < K)
        for (int r = 0; r < nr; ++r) acc[a] += (double)sX[r * kKP + i] * (double)sY[r * kKP + j];
    }
    if (tid < K) {
      for (int r = 0; r < nr; ++r) {
        const double v = sX[r * kKP + tid];
        n2 += v * v;
        cs += v;
      }
    } else if (tid >= 64 && tid < 64 + K) {
      for (int r = 0; r < nr; ++r) {
        const double v = sY[r * kKP + tid - 64];
        n2 += v * v;
      }
    }
  }
  if (tid < K) {
    sA[tid] = fmax(sqrt(n2), 1e-12);
    sU[tid] = sqrt(n2) < 1e-12 ? 0.0 : 1.0;  // (1: the norm is the divisor, it has a gradient of its own)
    sP[tid] = cs / (double)N;
  } else if (tid >= 64 && tid < 64 + K) {
    sB[tid - 64] = fmax(sqrt(n2), 1e-12);
    sW[tid - 64] = sqrt(n2) < 1e-12 ? 0.0 : 1.0;
  }
  __syncthreads();
  // C and E = exp(C), every thread four entries (the cosines lie in [0, 1]: exp needs no shift by the row maximum)
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int e = tid + a * kThreads, i = e / kKP, j = e % kKP;
    const bool in = i < K && j < K;
    const double c = in ? acc[a] / (sA[i] * sB[j]) : 0.0;
    sM[e] = c;
    sE[e] = in ? exp(c) : 0.0;
  }
  __syncthreads();
  if (tid < K) {  // row sums of E: softmax_j(C_i.) = E_ij / z_i, log-sum-exp = log z_i
    double z = 0.0;
    for (int j = 0; j < K; ++j) z += sE[tid * kKP + j];
    sZ[tid] = 1.0 / z;
    sL[tid] = log(z) - sM[tid * kKP + tid];  // row tid's cross-entropy term
  } else if (tid >= 64 && tid < 64 + K) {
    const double p = sP[tid - 64];
    sL[kKP + tid - 64] = p * log(p);  // the balance term's entries (no epsilon, as the reference)
  }
  __syncthreads();
  double ce = 0.0, ne = 0.0;
  if (tid == 0) {
    for (int i = 0; i < K; ++i) ce += sL[i];
    ce /= (double)K;
    for (int k = 0; k < K; ++k) ne += sL[kKP + k];
    ne += log((double)K);
  }
  if (tid < K) {  // u_i = sum_j G_ij C_ij, G = (E / z - I) / K
    double u = 0.0;
    for (int j = 0; j < K; ++j)
      u += (sE[tid * kKP + j] * sZ[tid] - (j == tid ? 1.0 : 0.0)) / (double)K * sM[tid * kKP + j];
    sU[tid] *= u / (sA[tid] * sA[tid]);
  } else if (tid >= 64 && tid < 64 + K) {  // w_j = sum_i G_ij C_ij
    const int j = tid - 64;
    double w = 0.0;
    for (int i = 0; i < K; ++i) w += (sE[i * kKP + j] * sZ[i] - (i == j ? 1.0 : 0.0)) / (double)K * sM[i * kKP + j];
    sW[j] *= w / (sB[j] * sB[j]);
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int e = tid + a * kThreads, i = e / kKP, j = e % kKP;
    if (i < K && j < K) sM[e] = (sE[e] * sZ[i] - (i == j ? 1.0 : 0.0)) / (double)K / (sA[i] * sB[j]);  // M
  }
  if (tid < K) sP[tid] = lamda * (log(sP[tid]) + 1.0) / (double)N;  // the balance term's gradient w.r.t. x_nk
  // ---- pass 2: the gradients
  const double gs = (double)scale * (gscale ? (double)gscale[0] : 1.0);
  for (int r0 = 0; r0 < N; r0 += kRows) {
    const int nr = min(kRows, N - r0);
    __syncthreads();
    stage_rows(lx, ly, ld, r0, nr, s, K, sX, sY);
    __syncthreads();
    for (int q = tid; q < nr * 2 * kKP; q += kThreads) {
      const int r = q / (2 * kKP), side = (q / kKP) & 1, k = q % kKP;
      if (k >= K) continue;
      double g = 0.0;
      if (side == 0) {
        for (int j = 0; j < K; ++j) g += sM[k * kKP + j] * (double)sY[r * kKP + j];
        g += sP[k] - (double)sX[r * kKP + k] * sU[k];
      } else {
        for (int i = 0; i < K; ++i) g += sM[i * kKP + k] * (double)sX[r * kKP + i];
        g -= (double)sY[r * kKP + k] * sW[k];
      }
      sGr[side][r * kKP + k] = g;
    }
    __syncthreads();
    for (int q = tid; q < 2 * nr; q += kThreads) {
      const int r = q >> 1, side = q & 1;
      const float* p = (side ? sY : sX) + r * kKP;
      double d = 0.0;
      for (int k = 0; k < K; ++k) d += sGr[side][r * kKP + k] * (double)p[k];
      sDot[side][r] = d;
    }
    __syncthreads();
    for (int q = tid; q < nr * 2 * kKP; q += kThreads) {
      const int r = q / (2 * kKP), side = (q / kKP) & 1, k = q % kKP;
      if (k >= K) continue;
      const double p = (side ? sY : sX)[r * kKP + k];
      (side ? dly : dlx)[(long)(r0 + r) * ld + (long)s * K + k] = (float)(gs * p * (sGr[side][r * kKP + k] - sDot[side][r]));
    }
  }
  subhead_total(ce, ce + lamda * ne, (double)scale, s, S, loss, ce_out, partial, ticket);
}

int zero_ticket(const char* name, unsigned int* ticket, hipStream_t st) {
  if (hipMemsetAsync(ticket, 0, sizeof(unsigned int), st) != hipSuccess) {
    spcl::set_error("%s: memset failed", name);
    return SPCL_ELAUNCH;
  }
  return SPCL_OK;
}

}  // namespace

extern "C" size_t spcl_pica_workspace_bytes(int S) { return S > 0 ? (size_t)S * 2 * sizeof(double) + 64 : 0; }

extern "C" int spcl_pica_seg_loss(const long long* jacc, const float* jf32, int S, int K, int T, double lamda_ne, float scale,
                                  float* j_out, float* loss, float* ce_out, float* dj, void* ws, size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG((jacc != nullptr) != (jf32 != nullptr), "spcl_pica_seg_loss: give exactly one of jacc / jf32");
  SPCL_CHECK_ARG(S > 0 && S <= 65535 && K >= 2 && K <= 32 && T >= 1 && T <= 15 && (T & 1),
                 "spcl_pica_seg_loss: bad shape S=%d K=%d T=%d", S, K, T);
  SPCL_CHECK_ARG(loss && dj && ws && ws_bytes >= spcl_pica_workspace_bytes(S), "spcl_pica_seg_loss: missing buffer");
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)ws;
  unsigned int* ticket = (unsigned int*)((char*)ws + (size_t)S * 2 * sizeof(double));
  if (int rc = zero_ticket("spcl_pica_seg_loss", ticket, st)) return rc;
  const int lds = (2 * T * T + 2 * kKP + kThreads + 8) * (int)sizeof(double);
  SPCL_LAUNCH(pica_seg_kernel, dim3(S), dim3(kThreads), lds, st, jacc, jf32, S, K, T, lamda_ne, scale, j_out, loss, ce_out, dj,
              partial, ticket);
  SPCL_LAUNCH_CHECK("pica_seg_kernel");
  return SPCL_OK;
}

extern "C" int spcl_pica_global_loss(const float* lx, const float* ly, long ld, int N, int S, int K, float lamda, float scale,
                                     const float* gscale, float* loss, float* ce_out, float* dlx, float* dly, void* ws,
                                     size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(lx && ly && loss && dlx && dly, "spcl_pica_global_loss: null pointer");
  SPCL_CHECK_ARG(N >= 1 && S > 0 && S <= 65535 && K >= 2 && K <= 32, "spcl_pica_global_loss: bad shape N=%d S=%d K=%d", N, S, K);
  SPCL_CHECK_ARG(ld >= (long)S * K, "spcl_pica_global_loss: row pitch %ld < S*K = %d", ld, S * K);
  SPCL_CHECK_ARG(ws && ws_bytes >= spcl_pica_workspace_bytes(S), "spcl_pica_global_loss: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)ws;
  unsigned int* ticket = (unsigned int*)((char*)ws + (size_t)S * 2 * sizeof(double));
  if (int rc = zero_ticket("spcl_pica_global_loss", ticket, st)) return rc;
  SPCL_LAUNCH(pica_global_kernel, dim3(S), dim3(kThreads), 0, st, lx, ly, ld, N, S, K, (double)lamda, scale, gscale, loss,
              ce_out, dlx, dly, partial, ticket);
  SPCL_LAUNCH_CHECK("pica_global_kernel");
  return SPCL_OK;
}
