// The strong intensity view of the unlabelled pair (semi_seg/hooks/strongview.py; FixMatch, UniMatch; the op family is
// nnU-Net's): gamma, contrast about the sample's mean, multiplicative brightness, blur, additive noise -- applied in the launch
// that makes the flipped copy.
//
//   spcl_strong_view_params   one workgroup per sample: the mean of the sample's C H W source elements in float64 in a fixed
//                             association, and (thread 0) eleven hashed words from the seed word in device memory (pxs_key,
//                             pixel_key.hpp) that gate the five ops and place their values in their ranges: one f32
//                             difference, one product, one sum, each rounded once (sv_place: no fused multiply-add is
//                             formed), so the float32 host restatement is bit-equal.
//   spcl_strong_view_apply    spcl_flip_batch with the row's ops on the way (include/spcl_hip.h has the formulas).  A workgroup
//                             owns a kTH x kTW tile of one (n, c) plane.  Blur: the tile and a halo of 2 are staged in LDS in
//                             the OUTPUT frame (coordinate clamped, then flipped, then loaded: the filter is symmetric and the
//                             edges replicate, so it commutes with the flip) with gamma, contrast and brightness applied at
//                             the load; a pass along W into a second LDS plane, the pass along H per output pixel.  A sample
//                             whose five values are all neutral is a pure copy of raw storage words.
//
// The table is device data that the host never sees: no index is formed from one of its values (they only enter arithmetic
// and three uniform branches: all-neutral, blur != 0, and the skips of gamma == 1 and sigma == 0).
#include <math.h>
#include <string.h>
#include "common.hpp"
#include "pixel_key.hpp"

namespace {

constexpr int kCols = SPCL_SV_COLS;
constexpr int kTH = SPCL_SV_TILE_H, kTW = SPCL_SV_TILE_W;  // 1024 pixels: four per thread
constexpr int kHalo = 2;
constexpr int kSH = kTH + 2 * kHalo, kSW = kTW + 2 * kHalo;  // the staged plane: 20 x 68
constexpr int kSP = kSW + 1;                                 // (row pitch 69: odd)
constexpr int kOps = 5;

struct sv_cfg {
  uint32_t p16[kOps];
  float lo[kOps], hi[kOps];
};

__device__ __forceinline__ double sv_wave_sum_d(double v) {  // the xor butterfly: every lane gets the wave's sum
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ----------------------------------------------------------------------------------------------------------------- params
// lo + (hi - lo) * f, capped at hi: three roundings to nearest.  __fmul_rn / __fadd_rn are a plain `*` and `+` in this
// toolchain's headers and were fused into v_fma_f32 (seen in the ISA; one table value in some hundreds then differs from the
// float32 host restatement by a spacing): contraction is switched off for this statement block instead.
__device__ __forceinline__ float sv_place(float lo, float hi, float f) {
#pragma clang fp contract(off)
  const float d = hi - lo;
  const float p = d * f;
  const float v = lo + p;
  return fminf(hi, v);
}

template <typename T>
__global__ void __launch_bounds__(256) strong_view_params_kernel(const T* __restrict__ x, unsigned CHW,
                                                                 const uint32_t* __restrict__ seedp, const sv_cfg cfg,
                                                                 float* __restrict__ table) {
  __shared__ double s_w[4];
  const unsigned n = blockIdx.x, tid = threadIdx.x;
  const T* xs = x + (size_t)n * CHW;
  double acc = 0.0;
  // elements tid, tid + 256, ... in index order; eight loads are issued before their adds so that the chain waits for memory
  // once per eight elements, not once per element (the association is unchanged)
  unsigned i = tid;
  for (; i + 7u * 256u < CHW; i += 8u * 256u) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = spcl::Elem<T>::load(xs + i + (unsigned)k * 256u);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += (double)v[k];
  }
  for (; i < CHW; i += 256u) acc += (double)spcl::Elem<T>::load(xs + i);
  acc = sv_wave_sum_d(acc);
  if ((tid & 63u) == 0u) s_w[tid >> 6] = acc;
  __syncthreads();
  if (tid != 0u) return;
  const double total = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
  const float mean = (float)(total / (double)CHW);
  const uint32_t seed = seedp[0];
  uint32_t r[11];
#pragma unroll
  for (int j = 0; j < 11; ++j) r[j] = spcl::pxs_key(16u * n + (uint32_t)j, seed);
  const float neutral[kOps] = {1.f, 1.f, 1.f, 0.f, 0.f};
  float* row = table + (size_t)n * kCols;
  unsigned mask = 0u;
#pragma unroll
  for (int k = 0; k < kOps; ++k) {
    const bool on = (r[2 * k] & 0xFFFFu) < cfg.p16[k];
    const float f = (float)(r[2 * k + 1] >> 8) * 0x1p-24f;  // (24 bits: exact)
    const float v = sv_place(cfg.lo[k], cfg.hi[k], f);
    row[k] = on ? v : neutral[k];
    mask |= on ? (1u << k) : 0u;
  }
  row[5] = (float)mask;
  row[6] = __uint_as_float(r[10]);
  row[7] = mean;
  row[8] = (float)__popc(mask);
#pragma unroll
  for (int j = 9; j < kCols; ++j) row[j] = 0.f;
}

// ------------------------------------------------------------------------------------------------------------------ apply
struct sv_row {
  float gamma, c, b, t, sigma, m;
  uint32_t nseed;
};

// steps 1 - 2 on a stored value
__device__ __forceinline__ float sv_point(float v, const sv_row& r) {
  float a = fminf(fmaxf(v, 0.f), 1.f);
  if (r.gamma != 1.f) a = powf(a, r.gamma);
  return ((a - r.m) * r.c + r.m) * r.b;
}

// steps 4 - 5 on pixel q of the sample's output frame
__device__ __forceinline__ float sv_finish(float a, uint32_t q, const sv_row& r) {
  if (r.sigma != 0.f) {
    const uint32_t k0 = spcl::pxs_key(2u * q, r.nseed), k1 = spcl::pxs_key(2u * q + 1u, r.nseed);
    const int z = (int)((k0 & 0xFFFFu) + (k0 >> 16) + (k1 & 0xFFFFu) + (k1 >> 16)) - 131070;
    a += (r.sigma * 1.7320508075688772f) * ((float)z * 0x1p-16f);  // (the product and the sum may contract into one fma)
  }
  return fminf(fmaxf(a, 0.f), 1.f);
}

// T: the element; V: elements per access (16 bytes, or 1).  V > 1 only where W % V == 0 and both pointers are 16-byte
// aligned: kTW is a multiple of V, so a unit of V columns lies inside W or past it as a whole, and its mirrored unit starts at
// W - V - w, a multiple of V.
template <typename T, int V>
__global__ void __launch_bounds__(256) strong_view_apply_kernel(const T* __restrict__ x, T* __restrict__ out, int H, int W,
                                                                unsigned C, unsigned tiles_h, unsigned tiles_w,
                                                                const uint8_t* __restrict__ flags,
                                                                const float* __restrict__ table) {
  typedef T vec_t __attribute__((ext_vector_type(V > 1 ? V : 2)));  // (not used where V == 1)
  __shared__ float s_a[kSH * kSP];   // the image after steps 1 - 2, halo of 2, output frame
  __shared__ float s_h[kSH * kTW];   // its pass along W
  const int tid = threadIdx.x;
  unsigned bid = blockIdx.x;
  const unsigned tw = bid % tiles_w;
  bid /= tiles_w;
  const unsigned th = bid % tiles_h;
  const unsigned plane = bid / tiles_h;  // n C + c
  const unsigned n = plane / C, c = plane - n * C;
  const int h0 = (int)th * kTH, w0 = (int)tw * kTW;
  const uint8_t f = flags[n];
  const bool fh = (f & 1) != 0, fw = (f & 2) != 0;
  const float* tr = table + (size_t)n * kCols;
  sv_row r;
  r.gamma = tr[0];
  r.c = tr[1];
  r.b = tr[2];
  r.t = tr[3];
  r.sigma = tr[4];
  r.nseed = __float_as_uint(tr[6]);
  r.m = tr[7];
  const T* xp = x + (size_t)plane * H * W;
  T* op = out + (size_t)plane * H * W;
  const bool neutral = r.gamma == 1.f && r.c == 1.f && r.b == 1.f && r.t == 0.f && r.sigma == 0.f;
  const bool blur = r.t != 0.f;  // (uniform over the workgroup, as `neutral`)

  if (blur) {
    for (int i = tid; i < kSH * kSW; i += 256) {
      const int sy = i / kSW, sx = i - sy * kSW;
      int h = h0 + sy - kHalo, w = w0 + sx - kHalo;
      h = h < 0 ? 0 : (h > H - 1 ? H - 1 : h);  // replicated edges: clamp, then flip, then load
      w = w < 0 ? 0 : (w > W - 1 ? W - 1 : w);
      const int sh = fh ? H - 1 - h : h, sw = fw ? W - 1 - w : w;
      s_a[sy * kSP + sx] = sv_point(spcl::Elem<T>::load(xp + (size_t)sh * W + sw), r);
    }
    __syncthreads();
    for (int i = tid; i < kSH * kTW; i += 256) {
      const int sy = i / kTW, sx = i - sy * kTW;
      const float* p = s_a + sy * kSP + sx;  // columns sx .. sx + 4 of the staged plane: w - 2 .. w + 2
      s_h[i] = ((p[0] + p[4]) + 4.f * (p[1] + p[3]) + 6.f * p[2]) * 0.0625f;
    }
    __syncthreads();
  }

  constexpr int kUnits = kTH * kTW / V;
  constexpr int kPerRow = kTW / V;
  for (int u = tid; u < kUnits; u += 256) {
    const int ty = u / kPerRow, tx = (u - ty * kPerRow) * V;
    const int h = h0 + ty, w = w0 + tx;
    if (h >= H || w >= W) continue;
    const int sh = fh ? H - 1 - h : h;
    const int sw = fw ? W - V - w : w;  // the first source column of the unit
    const T* src = xp + (size_t)sh * W + sw;
    T* dst = op + (size_t)h * W + w;
    T raw[V];
    if constexpr (V == 1) {
      raw[0] = src[0];
    } else {
      const vec_t v = *reinterpret_cast<const vec_t*>(src);
#pragma unroll
      for (int e = 0; e < V; ++e) raw[e] = fw ? v[V - 1 - e] : v[e];
    }
    if (!neutral) {
      const uint32_t q0 = (c * (uint32_t)H + (uint32_t)h) * (uint32_t)W + (uint32_t)w;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        float a;
        if (blur) {
          const int cy = ty + kHalo, cx = tx + e;  // s_h column cx is output column w0 + cx
          const float* p = s_h + cy * kTW + cx;
          const float B = ((p[-2 * kTW] + p[2 * kTW]) + 4.f * (p[-kTW] + p[kTW]) + 6.f * p[0]) * 0.0625f;
          a = s_a[cy * kSP + cx + kHalo];
          a = a + r.t * (B - a);
        } else {
          T one = raw[e];
          a = sv_point(spcl::Elem<T>::load(&one), r);
        }
        T o;
        spcl::Elem<T>::store(&o, sv_finish(a, q0 + (uint32_t)e, r));
        raw[e] = o;
      }
    }
    if constexpr (V == 1) {
      dst[0] = raw[0];
    } else {
      vec_t v;
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = raw[e];
      *reinterpret_cast<vec_t*>(dst) = v;
    }
  }
}

template <typename T>
void sv_launch_apply(const void* x, void* out, int N, int C, int H, int W, const uint8_t* flags, const float* table,
                     hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(T);
  const bool vec = W % V == 0 && ((uintptr_t)x | (uintptr_t)out) % 16 == 0;
  const unsigned tiles_h = (unsigned)((H + kTH - 1) / kTH), tiles_w = (unsigned)((W + kTW - 1) / kTW);
  const unsigned grid = (unsigned)N * (unsigned)C * tiles_h * tiles_w;
  if (vec)
    SPCL_LAUNCH((strong_view_apply_kernel<T, V>), dim3(grid), dim3(256), 0, st, (const T*)x, (T*)out, H, W, (unsigned)C,
                tiles_h, tiles_w, flags, table);
  else
    SPCL_LAUNCH((strong_view_apply_kernel<T, 1>), dim3(grid), dim3(256), 0, st, (const T*)x, (T*)out, H, W, (unsigned)C,
                tiles_h, tiles_w, flags, table);
}

float sv_bits(int32_t w) {
  float f;
  memcpy(&f, &w, sizeof f);
  return f;
}

}  // namespace

extern "C" int spcl_strong_view_tile(int* tile_h, int* tile_w) {
  SPCL_CHECK_ARG(tile_h && tile_w, "spcl_strong_view_tile: null pointer");
  *tile_h = kTH;
  *tile_w = kTW;
  return SPCL_OK;
}

extern "C" int spcl_strong_view_params(const void* x, int dtype, int N, int C, int H, int W, const uint32_t* seed,
                                       const int32_t* cfg, float* table, void* stream) {
  SPCL_CHECK_ARG(x && seed && cfg && table, "spcl_strong_view_params: null pointer");
  SPCL_CHECK_ARG(dtype == SPCL_F32 || dtype == SPCL_BF16, "spcl_strong_view_params: bad dtype %d", dtype);
  SPCL_CHECK_ARG(N >= 1 && N <= (1 << 20), "spcl_strong_view_params: N = %d (1 .. 2^20)", N);
  SPCL_CHECK_ARG(C > 0 && H > 0 && W > 0, "spcl_strong_view_params: bad shape");
  SPCL_CHECK_ARG((long)C * H * W < (1L << 31), "spcl_strong_view_params: too many elements per sample");
  static const char* const names[kOps] = {"gamma", "contrast", "brightness", "blur", "noise"};
  sv_cfg k{};
  for (int i = 0; i < kOps; ++i) {
    const int32_t p = cfg[3 * i];
    const float lo = sv_bits(cfg[3 * i + 1]), hi = sv_bits(cfg[3 * i + 2]);
    SPCL_CHECK_ARG(p >= 0 && p <= 65536, "spcl_strong_view_params: %s p16 = %d outside [0, 65536]", names[i], p);
    SPCL_CHECK_ARG(lo <= hi && hi < INFINITY, "spcl_strong_view_params: %s range [%g, %g] (lo <= hi, finite)", names[i],
                   (double)lo, (double)hi);  // (a NaN fails the compare)
    if (i == 0 || i == 2) SPCL_CHECK_ARG(lo > 0.f, "spcl_strong_view_params: %s lo = %g (must be > 0)", names[i], (double)lo);
    else SPCL_CHECK_ARG(lo >= 0.f, "spcl_strong_view_params: %s lo = %g (must be >= 0)", names[i], (double)lo);
    if (i == 3) SPCL_CHECK_ARG(hi <= 1.f, "spcl_strong_view_params: blur hi = %g (the range lies in [0, 1])", (double)hi);
    k.p16[i] = (uint32_t)p;
    k.lo[i] = lo;
    k.hi[i] = hi;
  }
  hipStream_t st = (hipStream_t)stream;
  const unsigned CHW = (unsigned)((long)C * H * W);
  spcl::prof_cost((double)N * CHW * (dtype == SPCL_F32 ? 4.0 : 2.0) + 64.0 * N, (double)N * CHW);
  if (dtype == SPCL_F32)
    SPCL_LAUNCH(strong_view_params_kernel<float>, dim3((unsigned)N), dim3(256), 0, st, (const float*)x, CHW, seed, k, table);
  else
    SPCL_LAUNCH(strong_view_params_kernel<bf16_t>, dim3((unsigned)N), dim3(256), 0, st, (const bf16_t*)x, CHW, seed, k, table);
  SPCL_LAUNCH_CHECK("spcl_strong_view_params");
  return SPCL_OK;
}

extern "C" int spcl_strong_view_apply(const void* x, void* out, int dtype, int N, int C, int H, int W, const uint8_t* flags,
                                      const float* table, void* stream) {
  SPCL_CHECK_ARG(x && out && flags && table, "spcl_strong_view_apply: null pointer");
  SPCL_CHECK_ARG(dtype == SPCL_F32 || dtype == SPCL_BF16, "spcl_strong_view_apply: bad dtype %d", dtype);
  SPCL_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0, "spcl_strong_view_apply: bad shape");
  SPCL_CHECK_ARG((long)C * H * W < (1L << 31), "spcl_strong_view_apply: too many elements per sample");
  SPCL_CHECK_ARG(out != x, "spcl_strong_view_apply: out and x are one buffer (the flip and the blur read neighbours)");
  const long tiles = (long)N * C * ((H + kTH - 1) / kTH) * ((W + kTW - 1) / kTW);
  SPCL_CHECK_ARG(tiles < (1L << 31), "spcl_strong_view_apply: too many tiles (%ld)", tiles);
  hipStream_t st = (hipStream_t)stream;
  spcl::prof_cost(2.0 * N * C * H * W * (dtype == SPCL_F32 ? 4.0 : 2.0), 60.0 * N * C * H * W);
  if (dtype == SPCL_F32) sv_launch_apply<float>(x, out, N, C, H, W, flags, table, st);
  else sv_launch_apply<bf16_t>(x, out, N, C, H, W, flags, table, st);
  SPCL_LAUNCH_CHECK("spcl_strong_view_apply");
  return SPCL_OK;
}
