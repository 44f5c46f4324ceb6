// The gradient behind BatchNorm + ReLU + 2 x 2 max-pool at one channel of one WHOLE window, pooled gradient only
// (semi_seg/arch/unet.py:75-77,118-121 and autograd): dy_k = scale dz_k + A y_k + B, dz_k = dp at the window's first maximum of
// relu(z) in scan order if that z is positive, else 0.  One expression sequence for every kernel that forms this dy --
// bn.hip bnrelu_bwd_pool_kernel<.., APPLY, FAST> writes it out, conv16_bwd.hip's POOLDY loader stages it in LDS -- so that
// they produce the same bits.
#pragma once
#include "common.hpp"

namespace spcl {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;  // (identical to the kernels' own typedef)

template <typename T> struct Word;  // one 32-bit word of a packed chunk
template <> struct Word<float> {
  static constexpr int EPW = 1;
  static __device__ __forceinline__ float get(uint32_t w, int) { return __uint_as_float(w); }
  static __device__ __forceinline__ uint32_t make(const float* v) { return __float_as_uint(v[0]); }
  // element h of the result = element h of raw word s[h]
  static __device__ __forceinline__ uint32_t merge(const uint32_t* s) { return s[0]; }
};
template <> struct Word<bf16_t> {
  static constexpr int EPW = 2;
  static __device__ __forceinline__ float get(uint32_t w, int h) {
    return __uint_as_float(h ? (w & 0xffff0000u) : (w << 16));
  }
  static __device__ __forceinline__ uint32_t make(const float* v) {
    return (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
  }
  static __device__ __forceinline__ uint32_t merge(const uint32_t* s) { return (s[0] & 0x0000ffffu) | (s[1] & 0xffff0000u); }
};

// RY[k][WI]: the raw storage word of window pixel k (scan order) that holds the channel, RDP[WI]: the pooled gradient's, H: the
// channel's half of the word -> O[k][H], unrounded (the caller rounds the words with Word<T>::make).
// Written for the instruction count (the apply kernel is the step's largest symbol): the first maximum as LANE MASKS --
// z_k > (running maximum, >= 0) for k = 1 .. 3, combined by scalar and-nots -- instead of a tracked index and four index
// compares: 30 vector instructions per (window, channel) for 44.
// A statement macro, not an inline function: as a function (inlined before the loops around it are unrolled) the apply kernel
// came out with another instruction order -- a code object that is no longer the measured one.  RY: u32x4[4], RDP: u32x4, WI /
// H: word / half indices, SC .. B: the channel's coefficients, O: float[4][EPW], written at [k][H].
#define SPCL_POOL_WINDOW_DY(T, RY, RDP, WI, H, SC, SH, A, B, O)                                          \
  {                                                                                                      \
    float yk[4], z[4];                                                                                   \
    _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                      \
      yk[k] = Word<T>::get((RY)[k][WI], H);                                                              \
      z[k] = fmaf(SC, yk[k], SH);                                                                        \
    }                                                                                                    \
    float m = fmaxf(z[0], 0.f);                                                                          \
    const bool s1 = z[1] > m;                                                                            \
    m = fmaxf(m, z[1]);                                                                                  \
    const bool s2 = z[2] > m;                                                                            \
    m = fmaxf(m, z[2]);                                                                                  \
    const bool s3 = z[3] > m;                                                                            \
    const bool b[4] = {z[0] > 0.f && !s1 && !s2 && !s3, s1 && !s2 && !s3, s2 && !s3, s3};                \
    const float dp = Word<T>::get((RDP)[WI], H);                                                         \
    _Pragma("unroll") for (int k = 0; k < 4; ++k) (O)[k][H] = fmaf(SC, b[k] ? dp : 0.f, fmaf(A, yk[k], B)); \
  }

}  // namespace spcl
