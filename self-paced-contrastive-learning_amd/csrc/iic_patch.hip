// Patch-wise IIC segmentation criterion of the MIDL baseline: IIDSegmentationSmallPathLoss (contrastyou/losses/iic_loss.py:
// 103-162, with patch_generator) applied to the segmentation output, as semi_seg/epochers/comparable.py:195-224 drives it.
//
// The class maps are cut into overlapping patches (stride = patch / 2, the last patch pushed back to the border; a map no
// larger than the patch gives one clipped patch) and the displacement-joint criterion of iic.hip is evaluated per patch:
//
//   J_P[dy][dx][i][j] = sum_{n,u,v in P} PX[n,i,u+dy-p,v+dx-p] * PY[n,j,u,v]      (PX = 0 outside the PATCH)
//
// with PX = softmax(lx), PY = softmax(flip(ly)); the result is scale * mean_P IIDSegmentationLoss(J_P).  The patch starts
// along an axis of length h are k * step for k < nreg and then last = max(h - patch, 0) (PatchAxis, computed on the host);
// every patch has min(patch, h) rows, so a pixel's covering patches follow from two divisions.
//
// Three launches, as in iic.hip:
//   joint     grid (nP * nsplit, T): a workgroup owns one vertical displacement of one band of one patch's (sample, row)
//             pairs.  Blocks of rows are staged into LDS with the softmax applied as the logits are read (the probability maps
//             are never written); a thread owns a 4 x 4 (i, j) tile of one dx and a share of the block's pixels, and adds the
//             products in float64 (each is exact there); at the end the sums go as 32.32 fixed-point words through an LDS
//             accumulator into the patch's joint (integer adds: independent of the order the workgroups finish in).  nsplit
//             grows as the patches get fewer, so one 224 x 224 patch still fills the chip.
//   criterion grid (nP): float64 min-shift, normalisation, symmetrisation, marginals, loss_P and dJ_P (one wave per
//             displacement); the last workgroup to finish adds the patch losses in index order.
//   backward  grid (N * H, column chunks), a thread per pixel: it gathers dPX / dPY from every patch that covers it (the
//             displaced pixel must lie in the same patch), applies the softmax backward and writes each gradient element
//             once -- no atomics.  d(ly) is written (at Y's unflipped position) only when asked for.
#include "common.hpp"
#include "iic_common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kBlkPix = 384;  // pixels (with their 2 * pad border columns) staged per block, for each of X and Y
constexpr int kMaxCW = 256;   // patch columns per pass: kMaxCW + 2 * 7 <= kBlkPix

struct PatchAxis {
  int nreg, step, last, n, len;  // starts k * step (k < nreg), then last; n = nreg + 1 patches of len = min(patch, h) rows
};

PatchAxis make_axis(int h, int patch) {
  PatchAxis a;
  a.step = patch / 2;
  a.nreg = h > patch ? (h - patch + a.step - 1) / a.step : 0;
  a.last = h > patch ? h - patch : 0;
  a.n = a.nreg + 1;
  a.len = h < patch ? h : patch;
  return a;
}

__device__ __forceinline__ int axis_start(const PatchAxis& a, int k) { return k < a.nreg ? k * a.step : a.last; }
// the regular patches covering x are k0 .. k1 (empty when k0 > k1); the last patch covers x when x >= a.last
__device__ __forceinline__ void axis_cover(const PatchAxis& a, int x, int& k0, int& k1) {
  k0 = x >= a.len ? (x - a.len) / a.step + 1 : 0;
  k1 = min(a.nreg - 1, x / a.step);
}

__device__ __forceinline__ double wave_sum_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------------------------------------- joint
template <int KP>
__global__ void __launch_bounds__(kThreads) iic_patch_joint_kernel(const float* __restrict__ lx, const float* __restrict__ ly,
                                                                   int N, int H, int W, int C, int pad, PatchAxis ah,
                                                                   PatchAxis aw, int nsplit, const uint8_t* __restrict__ flags,
                                                                   unsigned long long* __restrict__ jacc) {
  constexpr int NB = KP / 4;
  static_assert(15 * NB * NB * 16 * 8 <= 2 * kBlkPix * KP * 4, "the fixed-point fold reuses the staging buffer");
  __shared__ __attribute__((aligned(16))) float sbuf[2 * kBlkPix * KP];
  float* sX = sbuf;
  float* sY = sbuf + kBlkPix * KP;
  const int T = 2 * pad + 1, tid = threadIdx.x;
  const int P = blockIdx.x / nsplit, band = blockIdx.x - P * nsplit;
  const int dyi = blockIdx.y, dyv = dyi - pad;
  const int pr = P / aw.n, pc = P - pr * aw.n;
  const int a = axis_start(ah, pr), b = axis_start(aw, pc), ph = ah.len, pw = aw.len;
  const int rows = N * ph, R = (rows + nsplit - 1) / nsplit;
  const int r0 = band * R, r1 = min(r0 + R, rows);
  const int ntile = T * NB * NB, G = kThreads / ntile;  // ntile <= 15 * 16 = 240
  const int grp = tid / ntile, it = tid - grp * ntile;
  const int dx = it / (NB * NB), ib = (it / NB) % NB, jb = it % NB;
  double acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.0;
  for (int c0 = 0; c0 < pw; c0 += kMaxCW) {
    const int cw = min(kMaxCW, pw - c0), pitch = cw + 2 * pad;
    const int RB = max(1, kBlkPix / pitch);
    for (int rb0 = r0; rb0 < r1; rb0 += RB) {
      const int npx = min(RB, r1 - rb0) * pitch;
      __syncthreads();
      for (int q = tid; q < npx; q += kThreads) {
        const int rr = q / pitch, c = q - rr * pitch, r = rb0 + rr;
        const int n = r / ph, u = a + r - n * ph, v = b + c0 + c - pad, ux = u + dyv;
        const uint8_t f = flags ? flags[n] : 0;
        const bool yin = c >= pad && c < pad + cw;
        const bool xin = ux >= a && ux < a + ph && v >= b && v < b + pw;
        stage_prob<KP>(ly, C, H, W, n, yin ? flip_idx(u, H, f & 1) : -1, yin ? flip_idx(v, W, f & 2) : -1, 0, C, sY + q * KP);
        stage_prob<KP>(lx, C, H, W, n, xin ? ux : -1, v, 0, C, sX + q * KP);
      }
      __syncthreads();
      if (grp < G) {
        // Y at the block's flat pixel q (zeros in the border columns), X at q + dx - pad: inside the block for every q below.
        // The product of two f32 values is exact in float64 and the float64 sum of a band's products is good to 1e-16: the
        // joint carries the rounding of the softmax only (the criterion divides by J - min J, which can be 1e-4 of J).
        for (int q = pad + grp; q < npx - pad; q += G) {
          const f32x4 xv = *reinterpret_cast<const f32x4*>(sX + (q + dx - pad) * KP + ib * 4);
          const f32x4 yv = *reinterpret_cast<const f32x4*>(sY + q * KP + jb * 4);
          double xd[4], yd[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            xd[i] = (double)xv[i];
            yd[i] = (double)yv[i];
          }
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i * 4 + j] = fma(xd[i], yd[j], acc[i * 4 + j]);
        }
      }
    }
  }
  // fold the pixel groups as fixed-point words in LDS, then one fixed-point add per output into the patch's joint
  unsigned long long* sAcc = reinterpret_cast<unsigned long long*>(sbuf);
  __syncthreads();
  for (int o = tid; o < ntile * 16; o += kThreads) sAcc[o] = 0ull;
  __syncthreads();
  if (grp < G) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const unsigned long long w = (unsigned long long)llrint(acc[e] * kFix);
      if (w != 0ull) atomicAdd(sAcc + it * 16 + e, w);
    }
  }
  __syncthreads();
  const long base = ((long)P * T + dyi) * T * C * C;
  for (int o = tid; o < ntile * 16; o += kThreads) {
    const int t2 = o / 16, e = o - t2 * 16;
    const int dx2 = t2 / (NB * NB), i = ((t2 / NB) % NB) * 4 + e / 4, j = (t2 % NB) * 4 + e % 4;
    const unsigned long long w = sAcc[o];
    if (i < C && j < C && w != 0ull) atomicAdd(jacc + base + ((long)dx2 * C + i) * C + j, w);
  }
}

// ---------------------------------------------------------------------------------------------------------- criterion
// grid (nP), 256 threads = 4 waves; wave w < NW takes the displacements t = w, w + NW, ... of the patch (NW = 4; 2 for K > 24,
// whose per-wave matrices would not fit 64 KiB of LDS four times).  dj is [nP][T*T][KP][KP] (rows and columns >= K hold
// zeros), already times scale / (T^2 nmean).  nP counts the joints; the total is scale * sum / nmean (nmean = nP for one
// subhead; with S subheads the launch runs over S * nP joints and still divides by the nP patches of a subhead).
template <int NW>
__global__ void __launch_bounds__(kThreads) iic_patch_loss_kernel(const long long* __restrict__ jacc, int K, int KP, int T,
                                                                  int nP, int nmean, float scale, float* __restrict__ patch_loss,
                                                                  float* __restrict__ loss, float* __restrict__ dj,
                                                                  int* __restrict__ nan_flag, double* __restrict__ partial,
                                                                  unsigned int* __restrict__ ticket) {
  extern __shared__ double sd[];  // [8] reductions, [4] wave losses, then per wave [K*K] Pn, [K*K] P, [K] r
  const int P = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int KK = K * K, TT = T * T;
  double* sh = sd;
  double* sWave = sd + 8;
  double* sPn = sd + 12 + wave * (2 * KK + K);
  double* sP = sPn + KK;
  double* sR = sP + KK;
  const long long* jp = jacc + (long)P * TT * KK;
  const double eps = 1e-16;
  double mn = INFINITY;
  for (int e = tid; e < TT * KK; e += kThreads) mn = fmin(mn, (double)jp[e] / kFix);
  // (J - min) + 1e-16 in this order, as torch evaluates it: at the minimum entry the result is 1e-16, where J + (1e-16 - min)
  // gives 0 -- when that entry lies on the diagonal it survives the symmetrisation and carries the largest dJ of the patch
  const double m = block_min_d(mn, sh);
  const double coef = (double)scale / ((double)TT * nmean);
  float* djp = dj + (long)P * TT * KP * KP;
  double lw = 0.0;
  for (int t0 = 0; t0 < TT; t0 += NW) {
    const int t = t0 + wave;
    const bool valid = wave < NW && t < TT;  // uniform in a wave
    const long long* jt = jp + (long)(valid ? t : 0) * KK;
    double z = 0.0;
    if (valid)
      for (int e = lane; e < KK; e += 64) z += ((double)jt[e] / kFix - m) + 1e-16;
    z = wave_sum_d(z);
    if (valid)
      for (int e = lane; e < KK; e += 64) sPn[e] = (((double)jt[e] / kFix - m) + 1e-16) / z;
    __syncthreads();
    if (valid)
      for (int e = lane; e < KK; e += 64) {
        const int i = e / K, j = e - i * K;
        sP[e] = (sPn[i * K + j] + sPn[j * K + i]) * 0.5;
      }
    __syncthreads();
    if (valid)
      for (int i = lane; i < K; i += 64) {
        double r = 0.0;
        for (int j = 0; j < K; ++j) r += sP[i * K + j];
        sR[i] = r;
      }
    __syncthreads();
    double l = 0.0, gp = 0.0;
    if (valid)
      for (int e = lane; e < KK; e += 64) {
        const int i = e / K, j = e - i * K;
        const double p = sP[e], ri = sR[i], rj = sR[j];
        const double lp = log(p + eps), li = log(ri + eps), lj = log(rj + eps);
        l -= p * (lp - lj - li);
        gp += (-(lp + p / (p + eps)) + lj + rj / (rj + eps) + li + ri / (ri + eps)) * p;
      }
    l = wave_sum_d(l);
    gp = wave_sum_d(gp);
    if (valid) {
      lw += l;
      for (int e = lane; e < KP * KP; e += 64) {
        const int i = e / KP, j = e - i * KP;
        float g = 0.f;
        if (i < K && j < K) {
          const double p = sP[i * K + j], ri = sR[i], rj = sR[j];
          const double gg =
              -(log(p + eps) + p / (p + eps)) + log(rj + eps) + rj / (rj + eps) + log(ri + eps) + ri / (ri + eps);
          g = (float)((gg - gp) / z * coef);
        }
        djp[(long)t * KP * KP + e] = g;
      }
    }
    __syncthreads();
  }
  if (lane == 0) sWave[wave] = lw;
  __syncthreads();
  // fixed-order sum of the patch losses by the last workgroup
  __shared__ unsigned int last;
  if (tid == 0) {
    const double lp = (sWave[0] + sWave[1] + sWave[2] + sWave[3]) / (double)TT;
    if (patch_loss) patch_loss[P] = (float)lp;
    partial[P] = lp;
    __threadfence();
    last = atomicAdd(ticket, 1u) == (unsigned)(nP - 1);
  }
  __syncthreads();
  if (last) {  // (uniform over the workgroup)
    // 256 partials at a time into shared memory, added by one thread in index order (pixel_criterion.hpp's ordered_total: a chain
    // of dependent global loads would cost more than the rest of the launch)
    __shared__ double stage[kThreads];
    __threadfence();
    double tot = 0.0;
    int bad = 0;
    for (int base = 0; base < nP; base += kThreads) {
      if (base + tid < nP) stage[tid] = *((volatile double*)partial + base + tid);
      __syncthreads();
      if (tid == 0) {
        const int m = min(kThreads, nP - base);
        for (int q = 0; q < m; ++q) {
          bad |= isnan(stage[q]) ? 1 : 0;
          tot += stage[q];
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      loss[0] = (float)(tot * (double)scale / (double)nmean);
      nan_flag[0] = bad;
      *ticket = 0u;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- backward
// grid (N*H, column chunks); block = min(256, W rounded up to 64) threads, one pixel each
template <int KP, bool WANT_Y>
__global__ void __launch_bounds__(kThreads) iic_patch_bwd_kernel(const float* __restrict__ lx, const float* __restrict__ ly,
                                                                 int N, int H, int W, int C, int pad, PatchAxis ah, PatchAxis aw,
                                                                 const uint8_t* __restrict__ flags, const float* __restrict__ dj,
                                                                 const float* __restrict__ gscale, float* __restrict__ dlx,
                                                                 float* __restrict__ dly) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int T = 2 * pad + 1, CW = blockDim.x, tid = threadIdx.x;
  float* sPY = lds;                        // [(CW + 2p) * KP]: Y row u - dy + p, columns c0 - p ..
  float* sPX = lds + (CW + 2 * pad) * KP;  // [(CW + 2p) * KP]: X row u + dy - p (WANT_Y only)
  const int r = blockIdx.x, n = r / H, u = r - n * H;
  const int c0 = blockIdx.y * CW, cw = min(CW, W - c0), v = c0 + tid;
  const uint8_t f = flags ? flags[n] : 0;
  const float g = gscale ? gscale[0] : 1.f;
  int kr0, kr1, kc0, kc1;
  axis_cover(ah, u, kr0, kr1);
  axis_cover(aw, min(v, W - 1), kc0, kc1);
  const int nrow = kr1 - kr0 + 1 + (u >= ah.last ? 1 : 0);          // covering row patches: kr0 .. kr1, then the last one
  const int ncol = kc1 - kc0 + 1 + (v >= aw.last && v < W ? 1 : 0);
  double dX[KP], dY[KP];  // float64 sums: the terms of a pixel's gather cancel
  float oX[KP], oY[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    dX[k] = dY[k] = 0.0;
    oX[k] = oY[k] = 0.f;
  }
  for (int dyi = 0; dyi < T; ++dyi) {
    const int dyv = dyi - pad, ux = u + dyv, uy = u - dyv;
    const bool xin = WANT_Y && ux >= 0 && ux < H, yin = uy >= 0 && uy < H;
    if (!xin && !yin) continue;
    __syncthreads();
    for (int q = tid; q < cw + 2 * pad; q += CW) {
      const int vv = c0 + q - pad;
      const bool in = vv >= 0 && vv < W;
      stage_prob<KP>(ly, C, H, W, n, yin ? flip_idx(uy, H, f & 1) : -1, in ? flip_idx(vv, W, f & 2) : -1, 0, C, sPY + q * KP);
      if (WANT_Y) stage_prob<KP>(lx, C, H, W, n, xin ? ux : -1, vv, 0, C, sPX + q * KP);
    }
    __syncthreads();
    if (tid >= cw) continue;
    if (dyv == 0) {
#pragma unroll
      for (int k = 0; k < KP; ++k) oY[k] = sPY[(tid + pad) * KP + k];
    }
    for (int qr = 0; qr < nrow; ++qr) {
      const int kr = qr < kr1 - kr0 + 1 ? kr0 + qr : ah.nreg;
      const int a = axis_start(ah, kr);
      const bool xrow = xin && ux >= a && ux < a + ah.len, yrow = yin && uy >= a && uy < a + ah.len;
      if (!xrow && !yrow) continue;
      for (int qc = 0; qc < ncol; ++qc) {
        const int kc = qc < kc1 - kc0 + 1 ? kc0 + qc : aw.nreg;
        const int b = axis_start(aw, kc);
        const float* djd = dj + (((long)kr * aw.n + kc) * T + dyi) * T * KP * KP;
        for (int dxi = 0; dxi < T; ++dxi) {
          const int vx = v + dxi - pad, vy = v - dxi + pad;
          const bool xok = xrow && vx >= b && vx < b + aw.len, yok = yrow && vy >= b && vy < b + aw.len;
          if (!xok && !yok) continue;
          const float* djt = djd + dxi * KP * KP;
          float px[KP], py[KP];
#pragma unroll
          for (int k = 0; k < KP; ++k) {
            px[k] = WANT_Y && xok ? sPX[(tid + dxi) * KP + k] : 0.f;      // X at (u + dy - p, v + dx - p)
            py[k] = yok ? sPY[(tid + T - 1 - dxi) * KP + k] : 0.f;        // Y at (u - dy + p, v - dx + p)
          }
#pragma unroll
          for (int i = 0; i < KP; ++i) {
            const f32x4* row = reinterpret_cast<const f32x4*>(djt + i * KP);
#pragma unroll
            for (int j4 = 0; j4 < KP / 4; ++j4) {
              const f32x4 w = row[j4];
#pragma unroll
              for (int jj = 0; jj < 4; ++jj) {
                const int j = j4 * 4 + jj;
                if (WANT_Y) dY[j] = fma((double)w[jj], (double)px[i], dY[j]);
                dX[i] = fma((double)w[jj], (double)py[j], dX[i]);
              }
            }
          }
        }
      }
    }
  }
  if (tid < cw) {
    stage_prob<KP>(lx, C, H, W, n, u, v, 0, C, oX);
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      sx = fma((double)oX[k], dX[k], sx);
      sy = fma((double)oY[k], dY[k], sy);
    }
    float* oxp = dlx + ((long)(n * H + u) * W + v) * C;
#pragma unroll
    for (int k = 0; k < KP; ++k)
      if (k < C) oxp[k] = g * (float)((double)oX[k] * (dX[k] - sx));
    if (WANT_Y) {
      float* oyp = dly + ((long)(n * H + flip_idx(u, H, f & 1)) * W + flip_idx(v, W, f & 2)) * C;
#pragma unroll
      for (int k = 0; k < KP; ++k)
        if (k < C) oyp[k] = g * (float)((double)oY[k] * (dY[k] - sy));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- S subheads
// The decoder criterion of the IIC estimators (semi_seg/mi_estimator/discrete_mi_estimator.py:33-40, :53-60:
// IIDSegmentationSmallPathLoss(padding, patch_size) on each of the S probability maps of a DenseClusterHead, averaged over the
// subheads by the caller's scale).  The logits rows are [ld] wide with subhead s in columns s*K .. s*K+K-1, K <= 32; a
// workgroup's subhead is blockIdx.z and the joints are [S][nP][T][T][K][K].  Two things differ from the kernels above:
//   * T * (KP/4)^2 reaches 960 (dx, tile) items at KP = 32: a thread of the wide instantiations (KP > 16) owns up to kItems = 4
//     of them, item = tid + a * 256, as iic.hip's joint does; with 256 items or more there is one pixel group and the sums go
//     straight to the joint, otherwise the pixel groups fold through LDS as above (at most 128 items then: 16 KiB);
//   * the staging block shrinks with KP so that 2 * kBlk * KP floats stay within 64 KiB of static LDS (two workgroups a CU).
template <int KP>
struct HeadsCfg {
  static constexpr int kItems = KP > 16 ? 4 : 1;
  static constexpr int kBlk = KP <= 16 ? 384 : (KP <= 24 ? 320 : 256);  // staged pixels, for each of X and Y
  static constexpr int kCW = KP <= 16 ? 256 : kBlk / 2;                  // patch columns per pass: kCW + 14 <= kBlk
  static constexpr int kBwdCW = KP <= 16 ? 256 : 128;                    // backward's pixels per workgroup: 2 (kBwdCW + 14) KP floats
};

template <int KP>
__global__ void __launch_bounds__(kThreads) iic_patch_heads_joint_kernel(const float* __restrict__ lx,
                                                                         const float* __restrict__ ly, long ld, int N, int H,
                                                                         int W, int K, int pad, PatchAxis ah, PatchAxis aw,
                                                                         int nsplit, const uint8_t* __restrict__ flags,
                                                                         unsigned long long* __restrict__ jacc) {
  constexpr int NB = KP / 4, ITEMS = HeadsCfg<KP>::kItems, BLK = HeadsCfg<KP>::kBlk, CWMAX = HeadsCfg<KP>::kCW;
  static_assert(2 * BLK * KP * 4 <= 65536, "static LDS");
  static_assert((15 * NB * NB < 128 ? 15 * NB * NB : 128) * 16 * 8 <= 2 * BLK * KP * 4, "the fold reuses the staging buffer");
  static_assert(15 * NB * NB <= ITEMS * kThreads, "items per thread");
  __shared__ __attribute__((aligned(16))) float sbuf[2 * BLK * KP];
  float* sX = sbuf;
  float* sY = sbuf + BLK * KP;
  const int T = 2 * pad + 1, tid = threadIdx.x, nP = ah.n * aw.n;
  const int P = blockIdx.x / nsplit, band = blockIdx.x - P * nsplit;
  const int dyi = blockIdx.y, dyv = dyi - pad, s = blockIdx.z;
  const int pr = P / aw.n, pc = P - pr * aw.n;
  const int a = axis_start(ah, pr), b = axis_start(aw, pc), ph = ah.len, pw = aw.len;
  const int rows = N * ph, R = (rows + nsplit - 1) / nsplit;
  const int r0 = band * R, r1 = min(r0 + R, rows);
  const int ntile = T * NB * NB;
  const int G = ntile >= kThreads ? 1 : kThreads / ntile;
  const int grp = tid / ntile, it0 = tid - grp * ntile;  // (G == 1 with ntile >= 256: grp = 0, it0 = tid)
  double acc[ITEMS][16];
#pragma unroll
  for (int m = 0; m < ITEMS; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[m][e] = 0.0;
  for (int c0 = 0; c0 < pw; c0 += CWMAX) {
    const int cw = min(CWMAX, pw - c0), pitch = cw + 2 * pad;
    const int RB = max(1, BLK / pitch);
    for (int rb0 = r0; rb0 < r1; rb0 += RB) {
      const int npx = min(RB, r1 - rb0) * pitch;
      __syncthreads();
      for (int q = tid; q < npx; q += kThreads) {
        const int rr = q / pitch, c = q - rr * pitch, r = rb0 + rr;
        const int n = r / ph, u = a + r - n * ph, v = b + c0 + c - pad, ux = u + dyv;
        const uint8_t f = flags ? flags[n] : 0;
        const bool yin = c >= pad && c < pad + cw;
        const bool xin = ux >= a && ux < a + ph && v >= b && v < b + pw;
        stage_prob<KP>(ly, ld, H, W, n, yin ? flip_idx(u, H, f & 1) : -1, yin ? flip_idx(v, W, f & 2) : -1, s, K, sY + q * KP);
        stage_prob<KP>(lx, ld, H, W, n, xin ? ux : -1, v, s, K, sX + q * KP);
      }
      __syncthreads();
      if (grp < G) {
#pragma unroll
        for (int m = 0; m < ITEMS; ++m) {
          const int it = it0 + m * kThreads;
          if (it >= ntile) break;
          const int dx = it / (NB * NB), ib = (it / NB) % NB, jb = it % NB;
          // Y at the block's flat pixel q (zeros in the border columns), X at q + dx - pad: inside the block for every q below
          for (int q = pad + grp; q < npx - pad; q += G) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(sX + (q + dx - pad) * KP + ib * 4);
            const f32x4 yv = *reinterpret_cast<const f32x4*>(sY + q * KP + jb * 4);
            double xd[4], yd[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              xd[i] = (double)xv[i];
              yd[i] = (double)yv[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[m][i * 4 + j] = fma(xd[i], yd[j], acc[m][i * 4 + j]);
          }
        }
      }
    }
  }
  const long base = (((long)s * nP + P) * T + dyi) * T * K * K;
  if (G > 1) {  // (uniform) fewer than 256 items, one a thread: fold the pixel groups as fixed-point words in LDS
    unsigned long long* sAcc = reinterpret_cast<unsigned long long*>(sbuf);
    __syncthreads();
    for (int o = tid; o < ntile * 16; o += kThreads) sAcc[o] = 0ull;
    __syncthreads();
    if (grp < G) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const unsigned long long w = (unsigned long long)llrint(acc[0][e] * kFix);
        if (w != 0ull) atomicAdd(sAcc + it0 * 16 + e, w);
      }
    }
    __syncthreads();
    for (int o = tid; o < ntile * 16; o += kThreads) {
      const int t2 = o / 16, e = o - t2 * 16;
      const int dx2 = t2 / (NB * NB), i = ((t2 / NB) % NB) * 4 + e / 4, j = (t2 % NB) * 4 + e % 4;
      const unsigned long long w = sAcc[o];
      if (i < K && j < K && w != 0ull) atomicAdd(jacc + base + ((long)dx2 * K + i) * K + j, w);
    }
  } else {
#pragma unroll
    for (int m = 0; m < ITEMS; ++m) {
      const int it = tid + m * kThreads;
      if (it >= ntile) break;
      const int dx = it / (NB * NB), ib = (it / NB) % NB, jb = it % NB;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = ib * 4 + e / 4, j = jb * 4 + e % 4;
        const unsigned long long w = (unsigned long long)llrint(acc[m][e] * kFix);
        if (i < K && j < K && w != 0ull) atomicAdd(jacc + base + ((long)dx * K + i) * K + j, w);
      }
    }
  }
}

// grid (N*H, column chunks, S); block = min(kBwdCW, W rounded up to 64) threads, one pixel of one subhead each.  dj is
// [S][nP][T*T][KP][KP]; the gradients go to columns s*K + k of the [ld]-wide rows, the others are not touched.
template <int KP, bool WANT_Y>
__global__ void __launch_bounds__(kThreads) iic_patch_heads_bwd_kernel(const float* __restrict__ lx, const float* __restrict__ ly,
                                                                       long ld, int N, int H, int W, int K, int pad,
                                                                       PatchAxis ah, PatchAxis aw,
                                                                       const uint8_t* __restrict__ flags,
                                                                       const float* __restrict__ dj,
                                                                       const float* __restrict__ gscale, float* __restrict__ dlx,
                                                                       float* __restrict__ dly) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int T = 2 * pad + 1, CW = blockDim.x, tid = threadIdx.x, s = blockIdx.z, nP = ah.n * aw.n;
  float* sPY = lds;                        // [(CW + 2p) * KP]: Y row u - dy + p, columns c0 - p ..
  float* sPX = lds + (CW + 2 * pad) * KP;  // [(CW + 2p) * KP]: X row u + dy - p (WANT_Y only)
  const int r = blockIdx.x, n = r / H, u = r - n * H;
  const int c0 = blockIdx.y * CW, cw = min(CW, W - c0), v = c0 + tid;
  const uint8_t f = flags ? flags[n] : 0;
  const float g = gscale ? gscale[0] : 1.f;
  int kr0, kr1, kc0, kc1;
  axis_cover(ah, u, kr0, kr1);
  axis_cover(aw, min(v, W - 1), kc0, kc1);
  const int nrow = kr1 - kr0 + 1 + (u >= ah.last ? 1 : 0);
  const int ncol = kc1 - kc0 + 1 + (v >= aw.last && v < W ? 1 : 0);
  const float* djs = dj + (long)s * nP * T * T * KP * KP;
  double dX[KP], dY[KP];
  float oY[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    dX[k] = dY[k] = 0.0;
    oY[k] = 0.f;
  }
  for (int dyi = 0; dyi < T; ++dyi) {
    const int dyv = dyi - pad, ux = u + dyv, uy = u - dyv;
    const bool xin = WANT_Y && ux >= 0 && ux < H, yin = uy >= 0 && uy < H;
    if (!xin && !yin) continue;
    __syncthreads();
    for (int q = tid; q < cw + 2 * pad; q += CW) {
      const int vv = c0 + q - pad;
      const bool in = vv >= 0 && vv < W;
      stage_prob<KP>(ly, ld, H, W, n, yin ? flip_idx(uy, H, f & 1) : -1, in ? flip_idx(vv, W, f & 2) : -1, s, K, sPY + q * KP);
      if (WANT_Y) stage_prob<KP>(lx, ld, H, W, n, xin ? ux : -1, vv, s, K, sPX + q * KP);
    }
    __syncthreads();
    if (tid >= cw) continue;
    if (WANT_Y && dyv == 0) {
#pragma unroll
      for (int k = 0; k < KP; ++k) oY[k] = sPY[(tid + pad) * KP + k];
    }
    for (int qr = 0; qr < nrow; ++qr) {
      const int kr = qr < kr1 - kr0 + 1 ? kr0 + qr : ah.nreg;
      const int a = axis_start(ah, kr);
      const bool xrow = xin && ux >= a && ux < a + ah.len, yrow = yin && uy >= a && uy < a + ah.len;
      if (!xrow && !yrow) continue;
      for (int qc = 0; qc < ncol; ++qc) {
        const int kc = qc < kc1 - kc0 + 1 ? kc0 + qc : aw.nreg;
        const int b = axis_start(aw, kc);
        const float* djd = djs + (((long)kr * aw.n + kc) * T + dyi) * T * KP * KP;
        for (int dxi = 0; dxi < T; ++dxi) {
          const int vx = v + dxi - pad, vy = v - dxi + pad;
          const bool xok = xrow && vx >= b && vx < b + aw.len, yok = yrow && vy >= b && vy < b + aw.len;
          if (!xok && !yok) continue;
          const float* djt = djd + dxi * KP * KP;
          const float* pxs = sPX + (tid + dxi) * KP;          // X at (u + dy - p, v + dx - p)
          const float* pys = sPY + (tid + T - 1 - dxi) * KP;  // Y at (u - dy + p, v - dx + p)
          if (yok) {
#pragma unroll 4
            for (int j4 = 0; j4 < KP / 4; ++j4) {
              const f32x4 pv = *reinterpret_cast<const f32x4*>(pys + j4 * 4);
              const double py[4] = {(double)pv[0], (double)pv[1], (double)pv[2], (double)pv[3]};
#pragma unroll
              for (int i = 0; i < KP; ++i) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(djt + i * KP + j4 * 4);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) dX[i] = fma((double)w[jj], py[jj], dX[i]);
              }
            }
          }
          if (WANT_Y && xok) {
#pragma unroll 4
            for (int i4 = 0; i4 < KP / 4; ++i4) {
              const f32x4 pv = *reinterpret_cast<const f32x4*>(pxs + i4 * 4);
#pragma unroll
              for (int ii = 0; ii < 4; ++ii) {
                const double px = (double)pv[ii];
                const f32x4* row = reinterpret_cast<const f32x4*>(djt + (i4 * 4 + ii) * KP);
#pragma unroll
                for (int j4 = 0; j4 < KP / 4; ++j4) {
                  const f32x4 w = row[j4];
#pragma unroll
                  for (int jj = 0; jj < 4; ++jj) dY[j4 * 4 + jj] = fma((double)w[jj], px, dY[j4 * 4 + jj]);
                }
              }
            }
          }
        }
      }
    }
  }
  if (tid < cw) {
    float oX[KP];
    stage_prob<KP>(lx, ld, H, W, n, u, v, s, K, oX);
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      sx = fma((double)oX[k], dX[k], sx);
      if (WANT_Y) sy = fma((double)oY[k], dY[k], sy);
    }
    float* oxp = dlx + ((long)(n * H + u) * W + v) * ld + (long)s * K;
#pragma unroll
    for (int k = 0; k < KP; ++k)
      if (k < K) oxp[k] = g * (float)((double)oX[k] * (dX[k] - sx));
    if (WANT_Y) {
      float* oyp = dly + ((long)(n * H + flip_idx(u, H, f & 1)) * W + flip_idx(v, W, f & 2)) * ld + (long)s * K;
#pragma unroll
      for (int k = 0; k < KP; ++k)
        if (k < K) oyp[k] = g * (float)((double)oY[k] * (dY[k] - sy));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- host
struct Plan {
  PatchAxis ah, aw;
  int T, KP, nP;
  size_t jacc_bytes, partial_bytes, ws_bytes, dj_elems;
};

int make_plan(const char* name, int N, int C, int H, int W, int pad, int patch, Plan* p) {
  SPCL_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: empty input", name);
  SPCL_CHECK_ARG(C >= 2 && C <= 16, "%s: C = %d classes outside [2, 16]", name, C);
  SPCL_CHECK_ARG(pad >= 0 && pad <= 7, "%s: padding %d outside [0, 7]", name, pad);
  SPCL_CHECK_ARG(patch >= 2, "%s: patch size %d < 2 (the stride is patch / 2)", name, patch);
  SPCL_CHECK_ARG((long)N * H * W < (1L << 31) / 16, "%s: too many pixels", name);
  p->ah = make_axis(H, patch);
  p->aw = make_axis(W, patch);
  p->T = 2 * pad + 1;
  p->KP = (C + 3) / 4 * 4;
  const long nP = (long)p->ah.n * p->aw.n;
  SPCL_CHECK_ARG(nP * p->T * p->T * p->KP * p->KP < (1L << 31), "%s: %ld patches: too many", name, nP);
  p->nP = (int)nP;
  p->jacc_bytes = (size_t)nP * p->T * p->T * C * C * sizeof(long long);
  p->partial_bytes = (size_t)nP * sizeof(double);
  p->ws_bytes = p->jacc_bytes + p->partial_bytes + 64;
  p->dj_elems = (size_t)nP * p->T * p->T * p->KP * p->KP;
  return SPCL_OK;
}

template <int KP>
int launch_joint(const Plan& p, const float* lx, const float* ly, int N, int H, int W, int C, int pad, const uint8_t* flags,
                 unsigned long long* jacc, hipStream_t st) {
  const int rows = N * p.ah.len;
  int nsplit = (2048 + p.nP * p.T - 1) / (p.nP * p.T);
  nsplit = max(1, min(nsplit, rows / 4));
  spcl::prof_cost((double)(p.T + 1) * p.nP * rows * p.aw.len * C * 4.0,
                  2.0 * p.T * p.T * (double)p.nP * rows * p.aw.len * C * C);
  SPCL_LAUNCH(iic_patch_joint_kernel<KP>, dim3(p.nP * nsplit, p.T), dim3(kThreads), 0, st, lx, ly, N, H, W, C, pad, p.ah, p.aw,
              nsplit, flags, jacc);
  SPCL_LAUNCH_CHECK("iic_patch_joint_kernel");
  return SPCL_OK;
}

template <int KP>
int launch_bwd(const Plan& p, const float* lx, const float* ly, int N, int H, int W, int C, int pad, const uint8_t* flags,
               const float* dj, const float* gscale, float* dlx, float* dly, hipStream_t st) {
  const int block = min(kThreads, (W + 63) / 64 * 64);
  const int lds = 2 * (block + 2 * pad) * KP * (int)sizeof(float);  // <= 2 * 270 * 16 * 4 = 34560
  const dim3 grid(N * H, (W + block - 1) / block);
  spcl::prof_cost((double)(p.T + 2) * N * H * W * C * 4.0, (dly ? 16.0 : 8.0) * p.T * p.T * (double)N * H * W * C * C);
  if (dly) {
    SPCL_LAUNCH((iic_patch_bwd_kernel<KP, true>), grid, dim3(block), lds, st, lx, ly, N, H, W, C, pad, p.ah, p.aw, flags, dj,
                gscale, dlx, dly);
  } else {
    SPCL_LAUNCH((iic_patch_bwd_kernel<KP, false>), grid, dim3(block), lds, st, lx, ly, N, H, W, C, pad, p.ah, p.aw, flags, dj,
                gscale, dlx, dly);
  }
  SPCL_LAUNCH_CHECK("iic_patch_bwd_kernel");
  return SPCL_OK;
}

#define SPCL_IIC_PATCH_DISPATCH(fn, ...)                  \
  switch (plan.KP) {                                      \
    case 4: return fn<4>(plan, __VA_ARGS__);              \
    case 8: return fn<8>(plan, __VA_ARGS__);              \
    case 12: return fn<12>(plan, __VA_ARGS__);            \
    default: return fn<16>(plan, __VA_ARGS__);            \
  }

// ---- S subheads
struct HeadsPlan {
  PatchAxis ah, aw;
  int T, KP, nP;
  size_t jacc_bytes, partial_bytes, ws_bytes, dj_elems;
};

int make_heads_plan(const char* name, int N, int S, int K, long ld, int H, int W, int pad, int patch, HeadsPlan* p) {
  SPCL_CHECK_ARG(N > 0 && H > 0 && W > 0 && S > 0, "%s: empty input", name);
  SPCL_CHECK_ARG(K >= 2 && K <= 32, "%s: K = %d clusters outside [2, 32]", name, K);
  SPCL_CHECK_ARG(S <= 1024, "%s: S = %d subheads > 1024", name, S);
  SPCL_CHECK_ARG(ld >= (long)S * K, "%s: row pitch ld = %ld < S * K = %d", name, ld, S * K);
  SPCL_CHECK_ARG(pad >= 0 && pad <= 7, "%s: padding %d outside [0, 7]", name, pad);
  SPCL_CHECK_ARG(patch >= 2, "%s: patch size %d < 2 (the stride is patch / 2)", name, patch);
  SPCL_CHECK_ARG((double)N * H * W * (double)ld < 2147483648.0, "%s: too many logits", name);
  p->ah = make_axis(H, patch);
  p->aw = make_axis(W, patch);
  p->T = 2 * pad + 1;
  p->KP = (K + 3) / 4 * 4;
  const long nP = (long)p->ah.n * p->aw.n;
  SPCL_CHECK_ARG((double)S * nP * p->T * p->T * p->KP * p->KP < 2147483648.0,
                 "%s: %ld patches of %d subheads: too many", name, nP, S);
  p->nP = (int)nP;
  p->jacc_bytes = (size_t)S * nP * p->T * p->T * K * K * sizeof(long long);
  p->partial_bytes = (size_t)S * nP * sizeof(double);
  p->ws_bytes = p->jacc_bytes + p->partial_bytes + 64;
  p->dj_elems = (size_t)S * nP * p->T * p->T * p->KP * p->KP;
  return SPCL_OK;
}

template <int KP>
int launch_heads_joint(const HeadsPlan& p, const float* lx, const float* ly, long ld, int N, int H, int W, int S, int K, int pad,
                       const uint8_t* flags, unsigned long long* jacc, hipStream_t st) {
  const int rows = N * p.ah.len;
  const long wgs = (long)p.nP * p.T * S;
  int nsplit = (int)((2048 + wgs - 1) / wgs);
  nsplit = max(1, min(nsplit, rows / 4));
  spcl::prof_cost((double)(p.T + 1) * S * p.nP * rows * p.aw.len * K * 4.0,
                  2.0 * p.T * p.T * (double)S * p.nP * rows * p.aw.len * K * K);
  SPCL_LAUNCH(iic_patch_heads_joint_kernel<KP>, dim3(p.nP * nsplit, p.T, S), dim3(kThreads), 0, st, lx, ly, ld, N, H, W, K, pad,
              p.ah, p.aw, nsplit, flags, jacc);
  SPCL_LAUNCH_CHECK("iic_patch_heads_joint_kernel");
  return SPCL_OK;
}

template <int KP>
int launch_heads_bwd(const HeadsPlan& p, const float* lx, const float* ly, long ld, int N, int H, int W, int S, int K, int pad,
                     const uint8_t* flags, const float* dj, const float* gscale, float* dlx, float* dly, hipStream_t st) {
  const int block = min(HeadsCfg<KP>::kBwdCW, (W + 63) / 64 * 64);
  const int lds = 2 * (block + 2 * pad) * KP * (int)sizeof(float);  // <= 2 * 142 * 32 * 4 = 36352
  const dim3 grid(N * H, (W + block - 1) / block, S);
  spcl::prof_cost((double)(p.T + 2) * N * H * W * S * K * 4.0, (dly ? 16.0 : 8.0) * p.T * p.T * (double)N * H * W * S * K * K);
  if (dly) {
    SPCL_LAUNCH((iic_patch_heads_bwd_kernel<KP, true>), grid, dim3(block), lds, st, lx, ly, ld, N, H, W, K, pad, p.ah, p.aw,
                flags, dj, gscale, dlx, dly);
  } else {
    SPCL_LAUNCH((iic_patch_heads_bwd_kernel<KP, false>), grid, dim3(block), lds, st, lx, ly, ld, N, H, W, K, pad, p.ah, p.aw,
                flags, dj, gscale, dlx, dly);
  }
  SPCL_LAUNCH_CHECK("iic_patch_heads_bwd_kernel");
  return SPCL_OK;
}

#define SPCL_IIC_PATCH_HEADS_DISPATCH(fn, ...)            \
  switch (plan.KP) {                                      \
    case 4: return fn<4>(plan, __VA_ARGS__);              \
    case 8: return fn<8>(plan, __VA_ARGS__);              \
    case 12: return fn<12>(plan, __VA_ARGS__);            \
    case 16: return fn<16>(plan, __VA_ARGS__);            \
    case 20: return fn<20>(plan, __VA_ARGS__);            \
    case 24: return fn<24>(plan, __VA_ARGS__);            \
    case 28: return fn<28>(plan, __VA_ARGS__);            \
    default: return fn<32>(plan, __VA_ARGS__);            \
  }

}  // namespace

extern "C" int spcl_iic_patch_plan(int N, int C, int H, int W, int pad, int patch, int* num_patches, size_t* ws_bytes,
                                   size_t* dj_elems) {
  Plan plan;
  if (int rc = make_plan("spcl_iic_patch_plan", N, C, H, W, pad, patch, &plan)) return rc;
  if (num_patches) *num_patches = plan.nP;
  if (ws_bytes) *ws_bytes = plan.ws_bytes;
  if (dj_elems) *dj_elems = plan.dj_elems;
  return SPCL_OK;
}

extern "C" int spcl_iic_patch_forward(const float* lx, const float* ly, int N, int C, int H, int W, int pad, int patch,
                                      const uint8_t* flags_y, float scale, float* loss, float* patch_loss, int* nan_flag,
                                      float* dj, void* ws, size_t ws_bytes, void* stream) {
  Plan plan;
  if (int rc = make_plan("spcl_iic_patch_forward", N, C, H, W, pad, patch, &plan)) return rc;
  SPCL_CHECK_ARG(lx && ly && loss && nan_flag && dj && ws, "spcl_iic_patch_forward: null pointer");
  SPCL_CHECK_ARG(ws_bytes >= plan.ws_bytes, "spcl_iic_patch_forward: workspace of %zu bytes < %zu", ws_bytes, plan.ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  // the joints and, behind the partial losses, the ticket: zeroed by the call
  if (hipMemsetAsync(ws, 0, plan.ws_bytes, st) != hipSuccess) {
    spcl::set_error("spcl_iic_patch_forward: memset failed");
    return SPCL_ELAUNCH;
  }
  unsigned long long* jacc = reinterpret_cast<unsigned long long*>(ws);
  double* partial = reinterpret_cast<double*>((char*)ws + plan.jacc_bytes);
  unsigned int* ticket = reinterpret_cast<unsigned int*>((char*)ws + plan.jacc_bytes + plan.partial_bytes);
  auto joint = [&]() -> int { SPCL_IIC_PATCH_DISPATCH(launch_joint, lx, ly, N, H, W, C, pad, flags_y, jacc, st) };
  if (int rc = joint()) return rc;
  const int lds = (12 + 4 * (2 * C * C + C)) * (int)sizeof(double);  // <= 17 KiB
  SPCL_LAUNCH(iic_patch_loss_kernel<4>, dim3(plan.nP), dim3(kThreads), lds, st, reinterpret_cast<const long long*>(jacc), C,
              plan.KP, plan.T, plan.nP, plan.nP, scale, patch_loss, loss, dj, nan_flag, partial, ticket);
  SPCL_LAUNCH_CHECK("iic_patch_loss_kernel");
  return SPCL_OK;
}

extern "C" int spcl_iic_patch_backward(const float* lx, const float* ly, int N, int C, int H, int W, int pad, int patch,
                                       const uint8_t* flags_y, const float* dj, const float* gscale, float* dlx, float* dly,
                                       void* stream) {
  Plan plan;
  if (int rc = make_plan("spcl_iic_patch_backward", N, C, H, W, pad, patch, &plan)) return rc;
  SPCL_CHECK_ARG(lx && ly && dj && dlx, "spcl_iic_patch_backward: null pointer");
  hipStream_t st = (hipStream_t)stream;
  SPCL_IIC_PATCH_DISPATCH(launch_bwd, lx, ly, N, H, W, C, pad, flags_y, dj, gscale, dlx, dly, st)
}

// ---- S subheads: the decoder criterion of IICEstimator (discrete_mi_estimator.py:33-40, :53-60)
extern "C" int spcl_iic_patch_heads_plan(int N, int S, int K, long ld, int H, int W, int pad, int patch, int* num_patches,
                                         size_t* ws_bytes, size_t* dj_elems) {
  HeadsPlan plan;
  if (int rc = make_heads_plan("spcl_iic_patch_heads_plan", N, S, K, ld, H, W, pad, patch, &plan)) return rc;
  if (num_patches) *num_patches = plan.nP;
  if (ws_bytes) *ws_bytes = plan.ws_bytes;
  if (dj_elems) *dj_elems = plan.dj_elems;
  return SPCL_OK;
}

extern "C" int spcl_iic_patch_heads_forward(const float* lx, const float* ly, long ld, int N, int H, int W, int S, int K, int pad,
                                            int patch, const uint8_t* flags_y, float scale, float* loss, float* head_patch_loss,
                                            int* nan_flag, float* dj, void* ws, size_t ws_bytes, void* stream) {
  HeadsPlan plan;
  if (int rc = make_heads_plan("spcl_iic_patch_heads_forward", N, S, K, ld, H, W, pad, patch, &plan)) return rc;
  SPCL_CHECK_ARG(lx && ly && loss && nan_flag && dj && ws, "spcl_iic_patch_heads_forward: null pointer");
  SPCL_CHECK_ARG(ws_bytes >= plan.ws_bytes, "spcl_iic_patch_heads_forward: workspace of %zu bytes < %zu", ws_bytes,
                 plan.ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(ws, 0, plan.ws_bytes, st) != hipSuccess) {
    spcl::set_error("spcl_iic_patch_heads_forward: memset failed");
    return SPCL_ELAUNCH;
  }
  unsigned long long* jacc = reinterpret_cast<unsigned long long*>(ws);
  double* partial = reinterpret_cast<double*>((char*)ws + plan.jacc_bytes);
  unsigned int* ticket = reinterpret_cast<unsigned int*>((char*)ws + plan.jacc_bytes + plan.partial_bytes);
  auto joint = [&]() -> int {
    SPCL_IIC_PATCH_HEADS_DISPATCH(launch_heads_joint, lx, ly, ld, N, H, W, S, K, pad, flags_y, jacc, st)
  };
  if (int rc = joint()) return rc;
  // the S * nP joints are the criterion's "patches": sum / nP = sum_s mean_P
  const int nw = K > 24 ? 2 : 4;
  const int lds = (12 + nw * (2 * K * K + K)) * (int)sizeof(double);  // <= 39 KiB (K = 24, four waves)
  if (nw == 4) {
    SPCL_LAUNCH(iic_patch_loss_kernel<4>, dim3(S * plan.nP), dim3(kThreads), lds, st, reinterpret_cast<const long long*>(jacc),
                K, plan.KP, plan.T, S * plan.nP, plan.nP, scale, head_patch_loss, loss, dj, nan_flag, partial, ticket);
  } else {
    SPCL_LAUNCH(iic_patch_loss_kernel<2>, dim3(S * plan.nP), dim3(kThreads), lds, st, reinterpret_cast<const long long*>(jacc),
                K, plan.KP, plan.T, S * plan.nP, plan.nP, scale, head_patch_loss, loss, dj, nan_flag, partial, ticket);
  }
  SPCL_LAUNCH_CHECK("iic_patch_loss_kernel");
  return SPCL_OK;
}

extern "C" int spcl_iic_patch_heads_backward(const float* lx, const float* ly, long ld, int N, int H, int W, int S, int K, int pad,
                                             int patch, const uint8_t* flags_y, const float* dj, const float* gscale, float* dlx,
                                             float* dly, void* stream) {
  HeadsPlan plan;
  if (int rc = make_heads_plan("spcl_iic_patch_heads_backward", N, S, K, ld, H, W, pad, patch, &plan)) return rc;
  SPCL_CHECK_ARG(lx && ly && dj && dlx, "spcl_iic_patch_heads_backward: null pointer");
  hipStream_t st = (hipStream_t)stream;
  SPCL_IIC_PATCH_HEADS_DISPATCH(launch_heads_bwd, lx, ly, ld, N, H, W, S, K, pad, flags_y, dj, gscale, dlx, dly, st)
}
