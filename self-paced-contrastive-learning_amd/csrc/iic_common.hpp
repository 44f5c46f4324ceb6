// Device helpers shared by the IIC kernels (iic.hip, iic_patch.hip): the softmax applied as a logits row is staged, the
// 32.32 fixed-point scale of the joint accumulators and the float64 workgroup minimum; the per-sample flip and the float64
// workgroup sum come from pixel_criterion.hpp.
#pragma once
#include "common.hpp"
#include "pixel_criterion.hpp"

namespace {

constexpr double kFix = 4294967296.0;  // 2^32

// softmax of subhead s of the logits row at (n, u, v) into dst[KP] (pad entries 0); zeros when out of the image
template <int KP>
__device__ __forceinline__ void stage_prob(const float* __restrict__ l, long ld, int H, int W, int n, int u, int v, int s,
                                           int K, float* dst) {
  if (u < 0 || u >= H || v < 0 || v >= W) {
#pragma unroll
    for (int k = 0; k < KP; ++k) dst[k] = 0.f;
    return;
  }
  const float* p = l + ((long)(n * H + u) * W + v) * ld + (long)s * K;
  float x[KP];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    x[k] = k < K ? p[k] : -INFINITY;
    m = fmaxf(m, x[k]);
  }
  float z = 0.f;
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    x[k] = k < K ? expf(x[k] - m) : 0.f;
    z += x[k];
  }
  const float r = 1.f / z;
#pragma unroll
  for (int k = 0; k < KP; ++k) dst[k] = x[k] * r;
}

__device__ __forceinline__ double block_min_d(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = sh[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) t = fmin(t, sh[w]);
  return t;
}

}  // namespace
