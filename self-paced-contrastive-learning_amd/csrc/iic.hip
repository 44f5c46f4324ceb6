// IIC (invariant information clustering) criteria of the UDA-IIC baseline (semi_seg/hooks/discretemi.py,
// contrastyou/losses/iic_loss.py).
//
// Form (b) of the joint: the cluster heads' logits come from spcl_rows_linear_forward (all S subheads in one product, the
// rows [N][H][W][ld] f32 with subhead s in columns s*K .. s*K+K-1); the kernels apply the grouped softmax as they stage a
// pixel row into LDS, so the 100-column probability maps are never written.  X is read through its per-sample flips
// (bit 0 flips H, bit 1 flips W: spcl_flip_batch's flags), so the flipped copy is never made either.
//
//   J[s][dy][dx][i][j] = sum_{n,u,v} PX[n,s,i,u+dy-p,v+dx-p] * PY[n,s,j,u,v]        (PX = 0 outside the image)
//
// Packing: K clusters are padded to KP = K rounded up to 4 (20 -> 20: no waste at the reference's K; 10 -> 12).  A thread
// owns 4 x 4 (i, j) outputs of one horizontal displacement dx and runs over a row's pixels; per pixel it reads two float4
// from LDS (the X probabilities at v + dx, the Y probabilities at v) for 16 FMAs, i.e. 2 B of LDS per FMA per lane.  At
// ds_read_b128's 256 B/clk/CU (MI355X_MICROARCH.md) that allows the full f32 vector FMA rate, so the bound is the f32
// vector ALU (~157 TF peak; 49 GFLOP at Up_conv2, p = 3 -> >= 0.3 ms forward).  Measured: the whole criterion (forward,
// loss, backward) runs at 9-10 TFLOP/s useful (Up_conv3: 0.79 ms at p = 1, 3.8 ms at p = 3), far from that bound: the
// staging of a row (softmax of T * W logits rows per workgroup, repeated for each of the T vertical displacements) and,
// at p = 3, T * 25 = 175 tiles in a 256-thread workgroup (81 threads idle in the compute loop) are the likely
// costs (not profiled separately).  Not used here: exact-f32 MFMA (16x16x4 f32, 155 TF) or split-bf16 products (conv.hip's f32 mode),
// which the issue's 1 ms aim for Up_conv2, p = 3 would need; plain bf16 operands are too coarse for the min-shifted J.
// Determinism: a workgroup folds its pixel groups in LDS in a fixed order and adds its tile into the joint as 32.32
// fixed-point words (exact integer adds: the sum is independent of the order the workgroups finish in; J < 2^31).
//
// Backward: per pixel dPY[j] = sum_{dy,dx,i} dJ[dy,dx,i,j] PX[u+dy-p, v+dx-p, i] and dPX[i] = sum dJ[dy,dx,i,j]
// PY[u-dy+p, v-dx+p, j]: dJ is uniform across the workgroup (scalar loads), the probabilities come from LDS, then the
// grouped-softmax backward writes d(logits) (X's at its flipped position).  Each output is written once: deterministic.
#include "common.hpp"
#include "iic_common.hpp"

namespace {

constexpr int kFwdThreads = 256;
constexpr int kFwdCW = 128;     // pixel columns staged per pass
constexpr int kMaxItems = 4;    // (dx, 4x4 tile) items per thread

// grid (nband, T, S); rows r = n*H + u of Y, band b covers [b*R, min((b+1)*R, N*H))
template <int KP>
__global__ void __launch_bounds__(kFwdThreads) iic_joint_fwd_kernel(const float* __restrict__ lx, const float* __restrict__ ly,
                                                                   long ld, int N, int H, int W, int K, int pad, int R,
                                                                   const uint8_t* __restrict__ flags,
                                                                   unsigned long long* __restrict__ jacc) {
  constexpr int NB = KP / 4;
  __shared__ __attribute__((aligned(16))) float sY[kFwdCW * KP];
  __shared__ __attribute__((aligned(16))) float sX[(kFwdCW + 14) * KP];
  __shared__ float sRed[kFwdThreads * 16];
  const int T = 2 * pad + 1;
  const int dyi = blockIdx.y, s = blockIdx.z, dyv = dyi - pad;
  const int tid = threadIdx.x;
  const int ntile = T * NB * NB;
  const int G = ntile >= kFwdThreads ? 1 : kFwdThreads / ntile;
  const int grp = tid / ntile;           // pixel group (G > 1) -- the thread's tile is tid % ntile
  float acc[kMaxItems][16];
#pragma unroll
  for (int a = 0; a < kMaxItems; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[a][e] = 0.f;
  const int r0 = blockIdx.x * R, r1 = min(r0 + R, N * H);
  for (int r = r0; r < r1; ++r) {
    const int n = r / H, u = r - n * H, ux = u + dyv;
    if (ux < 0 || ux >= H) continue;  // uniform: X row outside the image contributes nothing
    const uint8_t f = flags ? flags[n] : 0;
    const int uxs = flip_idx(ux, H, f & 1);
    for (int c0 = 0; c0 < W; c0 += kFwdCW) {
      const int cw = min(kFwdCW, W - c0);
      __syncthreads();
      for (int q = tid; q < cw + (cw + 2 * pad); q += kFwdThreads) {
        if (q < cw) {
          stage_prob<KP>(ly, ld, H, W, n, u, c0 + q, s, K, sY + q * KP);
        } else {
          const int qx = q - cw, vx = c0 + qx - pad;
          const bool in = vx >= 0 && vx < W;
          stage_prob<KP>(lx, ld, H, W, n, uxs, in ? flip_idx(vx, W, f & 2) : -1, s, K, sX + qx * KP);
        }
      }
      __syncthreads();
      if (grp < G) {
#pragma unroll
        for (int a = 0; a < kMaxItems; ++a) {
          const int it = (G > 1 ? tid % ntile : tid) + a * kFwdThreads;
          if (it >= ntile) break;
          const int dx = it / (NB * NB), ib = (it / NB) % NB, jb = it % NB;
          for (int v = grp; v < cw; v += G) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(sX + (v + dx) * KP + ib * 4);
            const f32x4 yv = *reinterpret_cast<const f32x4*>(sY + v * KP + jb * 4);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[a][i * 4 + j] = fmaf(xv[i], yv[j], acc[a][i * 4 + j]);
          }
          if (G > 1) break;  // G > 1 means ntile < 256: one item per thread
        }
      }
    }
  }
  // fold the pixel groups in a fixed order, then one fixed-point add per output
  const long base = (long)(s * T + dyi) * T * K * K;
  if (G > 1) {
    __syncthreads();
    if (grp < G)
#pragma unroll
      for (int e = 0; e < 16; ++e) sRed[tid * 16 + e] = acc[0][e];
    __syncthreads();
    for (int q = tid; q < ntile * 16; q += kFwdThreads) {
      const int it = q / 16, e = q % 16;
      float v = 0.f;
      for (int g = 0; g < G; ++g) v += sRed[(g * ntile + it) * 16 + e];
      const int dx = it / (NB * NB), ib = (it / NB) % NB, jb = it % NB;
      const int i = ib * 4 + e / 4, j = jb * 4 + e % 4;
      if (i < K && j < K && v != 0.f)
        atomicAdd(jacc + base + ((long)dx * K + i) * K + j, (unsigned long long)llrint((double)v * kFix));
    }
  } else {
#pragma unroll
    for (int a = 0; a < kMaxItems; ++a) {
      const int it = tid + a * kFwdThreads;
      if (it >= ntile) break;
      const int dx = it / (NB * NB), ib = (it / NB) % NB, jb = it % NB;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = ib * 4 + e / 4, j = jb * 4 + e % 4;
        if (i < K && j < K && acc[a][e] != 0.f)
          atomicAdd(jacc + base + ((long)dx * K + i) * K + j, (unsigned long long)llrint((double)acc[a][e] * kFix));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- backward
// grid (N*H, S); block = min(256, W rounded up to 64) threads, one pixel column each per pass
template <int KP>
__global__ void __launch_bounds__(256) iic_joint_bwd_kernel(const float* __restrict__ lx, const float* __restrict__ ly, long ld,
                                                            int N, int H, int W, int K, int pad,
                                                            const uint8_t* __restrict__ flags, const float* __restrict__ dj,
                                                            const float* __restrict__ gscale, float* __restrict__ dlx,
                                                            float* __restrict__ dly) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int T = 2 * pad + 1;
  const int CW = blockDim.x;
  float* sPX = lds;                         // [(CW + 2p) * KP]: X row u + dy - p, columns c0 - p ..
  float* sPY = lds + (CW + 2 * pad) * KP;   // [(CW + 2p) * KP]: Y row u - dy + p, columns c0 - p ..
  const int r = blockIdx.x, s = blockIdx.y;
  const int n = r / H, u = r - n * H, tid = threadIdx.x;
  const uint8_t f = flags ? flags[n] : 0;
  const float g = gscale ? gscale[0] : 1.f;
  const float* djs = dj + (long)s * T * T * K * K;
  for (int c0 = 0; c0 < W; c0 += CW) {
    const int cw = min(CW, W - c0);
    const int v = c0 + tid;
    float dX[KP], dY[KP], oX[KP], oY[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) dX[k] = dY[k] = oX[k] = oY[k] = 0.f;
    for (int dyi = 0; dyi < T; ++dyi) {
      const int dyv = dyi - pad;
      const int ux = u + dyv, uy = u - dyv;
      const bool xin = ux >= 0 && ux < H, yin = uy >= 0 && uy < H;
      if (!xin && !yin) continue;
      __syncthreads();
      for (int q = tid; q < 2 * (cw + 2 * pad); q += CW) {
        const bool isx = q < cw + 2 * pad;
        const int qq = isx ? q : q - (cw + 2 * pad);
        const int vv = c0 + qq - pad;
        const bool in = vv >= 0 && vv < W;
        if (isx)
          stage_prob<KP>(lx, ld, H, W, n, xin ? flip_idx(ux, H, f & 1) : -1, in ? flip_idx(vv, W, f & 2) : -1, s, K,
                         sPX + qq * KP);
        else
          stage_prob<KP>(ly, ld, H, W, n, yin ? uy : -1, vv, s, K, sPY + qq * KP);
      }
      __syncthreads();
      if (tid >= cw) continue;
      if (dyv == 0) {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
          oX[k] = sPX[(tid + pad) * KP + k];
          oY[k] = sPY[(tid + pad) * KP + k];
        }
      }
      const float* djd = djs + (long)dyi * T * K * K;
      for (int dxi = 0; dxi < T; ++dxi) {
        const float* djt = djd + (long)dxi * K * K;
        float px[KP], py[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) {
          px[k] = sPX[(tid + dxi) * KP + k];               // X at (u + dy - p, v + dx - p)
          py[k] = sPY[(tid + T - 1 - dxi) * KP + k];       // Y at (u - dy + p, v - dx + p)
        }
#pragma unroll
        for (int i = 0; i < KP; ++i) {
          if (i >= K) break;
#pragma unroll
          for (int j = 0; j < KP; ++j) {
            if (j >= K) break;
            const float w = djt[i * K + j];
            dY[j] = fmaf(w, px[i], dY[j]);
            dX[i] = fmaf(w, py[j], dX[i]);
          }
        }
      }
    }
    if (tid < cw) {
      float sx = 0.f, sy = 0.f;
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        sx = fmaf(oX[k], dX[k], sx);
        sy = fmaf(oY[k], dY[k], sy);
      }
      float* oxp = dlx + ((long)(n * H + flip_idx(u, H, f & 1)) * W + flip_idx(v, W, f & 2)) * ld + (long)s * K;
      float* oyp = dly + ((long)(n * H + u) * W + v) * ld + (long)s * K;
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        if (k >= K) break;
        oxp[k] = g * oX[k] * (dX[k] - sx);
        oyp[k] = g * oY[k] * (dY[k] - sy);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- loss
// grid (T*T, S), 256 threads: one displacement of one subhead each; the subhead's min is recomputed by each workgroup
// (T^2 K^2 reads from L2).  The partial losses are summed in a fixed order by the last workgroup to finish.
__device__ __forceinline__ double jval(const long long* jacc, const float* jf, long e) {
  return jacc ? (double)jacc[e] / kFix : (double)jf[e];
}

__global__ void __launch_bounds__(256) iic_loss_kernel(const long long* __restrict__ jacc, const float* __restrict__ jf, int K,
                                                       int T, int dense, float scale, float* __restrict__ jout,
                                                       float* __restrict__ loss, float* __restrict__ djout,
                                                       int* __restrict__ nan_flag, double* __restrict__ partial,
                                                       unsigned int* __restrict__ ticket) {
  extern __shared__ double sd[];  // [K*K] Pn, [K*K] P, [K] r, [8] reductions
  double* sPn = sd;
  double* sP = sd + K * K;
  double* sR = sd + 2 * K * K;
  double* sh = sd + 2 * K * K + K;
  const int t = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const long KK = (long)K * K, sub = (long)s * T * T * KK, off = sub + t * KK;
  const double eps = dense ? 1e-16 : 1e-10;
  double m = 0.0;
  if (dense) {
    double mn = INFINITY;
    for (long e = tid; e < T * T * KK; e += blockDim.x) mn = fmin(mn, jval(jacc, jf, sub + e));
    m = block_min_d(mn, sh);
  }
  const double shift = dense ? 1e-16 - m : 0.0;
  double z = 0.0;
  for (int e = tid; e < KK; e += blockDim.x) {
    const double a = jval(jacc, jf, off + e);
    if (jout && jacc) jout[off + e] = (float)a;
    z += a + shift;
  }
  z = block_sum_d(z, sh);
  for (int e = tid; e < KK; e += blockDim.x) sPn[e] = (jval(jacc, jf, off + e) + shift) / z;
  __syncthreads();
  for (int e = tid; e < KK; e += blockDim.x) {
    const int i = e / K, j = e - i * K;
    sP[e] = (sPn[i * K + j] + sPn[j * K + i]) * 0.5;
  }
  __syncthreads();
  for (int i = tid; i < K; i += blockDim.x) {
    double r = 0.0;
    for (int j = 0; j < K; ++j) r += sP[i * K + j];
    sR[i] = r;
  }
  __syncthreads();
  double l = 0.0, gp = 0.0;
  for (int e = tid; e < KK; e += blockDim.x) {
    const int i = e / K, j = e - i * K;
    const double p = sP[e], ri = sR[i], rj = sR[j];
    const double lp = log(p + eps), li = log(ri + eps), lj = log(rj + eps);
    l -= p * (lp - lj - li);
    const double gg = -(lp + p / (p + eps)) + lj + rj / (rj + eps) + li + ri / (ri + eps);
    gp += gg * p;
  }
  l = block_sum_d(l, sh);
  gp = block_sum_d(gp, sh);
  const double coef = (double)scale / ((double)T * T);
  for (int e = tid; e < KK; e += blockDim.x) {
    const int i = e / K, j = e - i * K;
    const double p = sP[e], ri = sR[i], rj = sR[j];
    const double gg = -(log(p + eps) + p / (p + eps)) + log(rj + eps) + rj / (rj + eps) + log(ri + eps) + ri / (ri + eps);
    djout[off + e] = (float)((gg - gp) / z * coef);
  }
  // fixed-order sum of the partial losses by the last workgroup
  ordered_total(l, coef, loss, partial, ticket, s * gridDim.x + t, gridDim.x * gridDim.y, 0u, nullptr,
                [nan_flag, dense](float lv, unsigned long long) {
                  if (nan_flag) nan_flag[0] = (dense && isnan(lv)) ? 1 : 0;
                });
}

template <int KP>
int launch_fwd(const float* lx, const float* ly, long ld, int N, int H, int W, int S, int K, int pad, const uint8_t* flags,
               unsigned long long* jacc, hipStream_t st) {
  const int T = 2 * pad + 1;
  const int rows = N * H;
  int nband = (2048 + T * S - 1) / (T * S);
  nband = max(1, min(nband, rows));
  const int R = (rows + nband - 1) / nband;
  nband = (rows + R - 1) / R;
  spcl::prof_cost((double)T * rows * W * S * K * 4.0 * 2, 2.0 * T * T * (double)rows * W * S * K * K);
  SPCL_LAUNCH(iic_joint_fwd_kernel<KP>, dim3(nband, T, S), dim3(kFwdThreads), 0, st, lx, ly, ld, N, H, W, K, pad, R, flags,
              jacc);
  SPCL_LAUNCH_CHECK("iic_joint_fwd_kernel");
  return SPCL_OK;
}

template <int KP>
int launch_bwd(const float* lx, const float* ly, long ld, int N, int H, int W, int S, int K, int pad, const uint8_t* flags,
               const float* dj, const float* gscale, float* dlx, float* dly, hipStream_t st) {
  const int block = min(256, (W + 63) / 64 * 64);
  const int lds = 2 * (block + 2 * pad) * KP * (int)sizeof(float);
  if (lds > 65536) spcl::func_lds_limit((const void*)iic_joint_bwd_kernel<KP>, lds, "iic_joint_bwd_kernel");
  const int T = 2 * pad + 1;
  spcl::prof_cost((double)T * N * H * W * S * K * 4.0 * 2 + 2.0 * N * H * W * S * K * 4.0,
                  4.0 * T * T * (double)N * H * W * S * K * K);
  SPCL_LAUNCH(iic_joint_bwd_kernel<KP>, dim3(N * H, S), dim3(block), lds, st, lx, ly, ld, N, H, W, K, pad, flags, dj, gscale,
              dlx, dly);
  SPCL_LAUNCH_CHECK("iic_joint_bwd_kernel");
  return SPCL_OK;
}

#define SPCL_IIC_DISPATCH(fn, ...)           \
  switch ((K + 3) / 4) {                     \
    case 1: return fn<4>(__VA_ARGS__);       \
    case 2: return fn<8>(__VA_ARGS__);       \
    case 3: return fn<12>(__VA_ARGS__);      \
    case 4: return fn<16>(__VA_ARGS__);      \
    case 5: return fn<20>(__VA_ARGS__);      \
    case 6: return fn<24>(__VA_ARGS__);      \
    case 7: return fn<28>(__VA_ARGS__);      \
    default: return fn<32>(__VA_ARGS__);     \
  }

int check_joint_args(const char* name, int N, int H, int W, int S, int K, int pad, long ld) {
  SPCL_CHECK_ARG(N > 0 && H > 0 && W > 0 && S > 0, "%s: empty input", name);
  SPCL_CHECK_ARG(K >= 2 && K <= 32, "%s: K = %d clusters outside [2, 32]", name, K);
  SPCL_CHECK_ARG(pad >= 0 && pad <= 7, "%s: padding %d outside [0, 7]", name, pad);
  SPCL_CHECK_ARG(ld >= (long)S * K, "%s: row pitch %ld < S*K = %d", name, ld, S * K);
  const int T = 2 * pad + 1, NB = (K + 3) / 4;
  SPCL_CHECK_ARG(T * NB * NB <= kMaxItems * kFwdThreads, "%s: T * (K/4)^2 = %d tiles > %d", name, T * NB * NB,
                 kMaxItems * kFwdThreads);
  SPCL_CHECK_ARG((long)N * H * W < (1L << 31), "%s: too many pixel rows", name);
  return SPCL_OK;
}

}  // namespace

extern "C" size_t spcl_iic_joint_workspace_bytes(int S, int K, int pad) {
  const long T = 2 * pad + 1;
  return (size_t)(S * T * T * K * K) * sizeof(long long);
}

extern "C" int spcl_iic_joint_forward(const float* lx, const float* ly, long ld, int N, int H, int W, int S, int K, int pad,
                                      const uint8_t* flags_x, long long* jacc, void* stream) {
  if (int rc = check_joint_args("spcl_iic_joint_forward", N, H, W, S, K, pad, ld)) return rc;
  SPCL_CHECK_ARG(lx && ly && jacc, "spcl_iic_joint_forward: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(jacc, 0, spcl_iic_joint_workspace_bytes(S, K, pad), st) != hipSuccess) {
    spcl::set_error("spcl_iic_joint_forward: memset failed");
    return SPCL_ELAUNCH;
  }
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(jacc);
  SPCL_IIC_DISPATCH(launch_fwd, lx, ly, ld, N, H, W, S, K, pad, flags_x, acc, st)
}

extern "C" int spcl_iic_joint_backward(const float* lx, const float* ly, long ld, int N, int H, int W, int S, int K, int pad,
                                       const uint8_t* flags_x, const float* dj, const float* gscale, float* dlx, float* dly,
                                       void* stream) {
  if (int rc = check_joint_args("spcl_iic_joint_backward", N, H, W, S, K, pad, ld)) return rc;
  SPCL_CHECK_ARG(lx && ly && dj && dlx && dly, "spcl_iic_joint_backward: null pointer");
  hipStream_t st = (hipStream_t)stream;
  SPCL_IIC_DISPATCH(launch_bwd, lx, ly, ld, N, H, W, S, K, pad, flags_x, dj, gscale, dlx, dly, st)
}

extern "C" size_t spcl_iic_loss_workspace_bytes(int S, int T) {
  return (size_t)S * T * T * sizeof(double) + 64;
}

extern "C" int spcl_iic_loss(const long long* jacc, const float* jf32, int S, int K, int T, int dense, float scale,
                             float* j_out, float* loss, float* dj, int* nan_flag, void* ws, size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG((jacc != nullptr) != (jf32 != nullptr), "spcl_iic_loss: give exactly one of jacc / jf32");
  SPCL_CHECK_ARG(S > 0 && K >= 2 && K <= 32 && T >= 1 && T <= 15 && (T & 1), "spcl_iic_loss: bad shape S=%d K=%d T=%d", S,
                 K, T);
  SPCL_CHECK_ARG(dense || T == 1, "spcl_iic_loss: the encoder criterion has no displacements (T = 1)");
  SPCL_CHECK_ARG(loss && dj && ws && ws_bytes >= spcl_iic_loss_workspace_bytes(S, T), "spcl_iic_loss: missing buffer");
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)ws;
  unsigned int* ticket = (unsigned int*)((char*)ws + (size_t)S * T * T * sizeof(double));
  if (hipMemsetAsync(ticket, 0, sizeof(unsigned int), st) != hipSuccess) {
    spcl::set_error("spcl_iic_loss: memset failed");
    return SPCL_ELAUNCH;
  }
  const int lds = (2 * K * K + K + 8) * (int)sizeof(double);
  if (lds > 65536) spcl::func_lds_limit((const void*)iic_loss_kernel, lds, "iic_loss_kernel");
  SPCL_LAUNCH(iic_loss_kernel, dim3(T * T, S), dim3(256), lds, st, jacc, jf32, K, T, dense, scale, j_out, loss, dj, nan_flag,
              partial, ticket);
  SPCL_LAUNCH_CHECK("iic_loss_kernel");
  return SPCL_OK;
}
