// CutMix for cross pseudo supervision (semi_seg/hooks/cps.py; French et al., BMVC 2020; Chen et al., CVPR 2021): one box per
// sample, drawn on the device; inside box n the mixed sample n shows sample (n + roll) mod N, elsewhere itself.
//
//   spcl_cutmix_boxes           one tiny launch: thread n hashes four words from the seed word in device memory (pxs_key,
//                               pixel_key.hpp) and forms box n by an integer-only rule (include/spcl_hip.h), products in 64
//                               bits: the Python restatement is exact.
//   spcl_cutmix_images          out[n, :, h, w] = x[src(n, h, w), :, h, w], src = (n + roll) mod N inside box n and n elsewhere.
//                               A pure copy of 2- or 4-byte elements; a sample is [R][L] with L contiguous elements per image
//                               row (NCHW: R = C H, L = W; channels-last: R = H, L = W C), 16-byte accesses where L allows.
//   spcl_cross_pseudo_ce_mixed  cross_pseudo.hip's criterion with the labels read THROUGH the boxes: the students s_a, s_b saw
//                               the mixed images, the teachers t_a, t_b the unmixed ones; pixel (n, h, w) takes its labels and
//                               confidences from the teachers' pixel (src(n, h, w), h, w).  No mixed teacher map is ever
//                               written.  Each of the four maps is read once, each soft-max is formed once.
//
// The boxes are device data that the host never sees: no index is formed from a box extent.  A pixel is inside iff
// (unsigned)(h - y0) < (unsigned)bh && (unsigned)(w - x0) < (unsigned)bw, and the sample read is n or (n + roll) mod N whatever
// the four numbers hold.
//
// The criterion is laid out as its sibling: a workgroup owns a slab of kSlab = 1024 pixels (thread t: pixels t, t + 256,
// t + 512, t + 768, added in that order; the xor butterfly of the wave; the four waves in order) and hands in a row of 2
// doubles and 4 C + 2 integers (wave-uniform: popcount(ballot)).  The last workgroup to take its ticket adds the rows: the two
// doubles in EXACTLY the sibling's association (groups of consecutive rows cut by the sibling's column count 4 C + 3, rows in
// order, groups in order), so that without boxes and with t = s the loss is the sibling's to the bit; the extra integer column
// (pixels inside a box) rides with the thread of the agreement column.  No floating-point atomics and no memset: the workspace
// arrives zero-filled once, the close resets the ticket.
#include "common.hpp"
#include "pixel_criterion.hpp"
#include "pixel_key.hpp"

namespace {

// ------------------------------------------------------------------------------------------------------------------ boxes
__global__ void __launch_bounds__(256) cutmix_boxes_kernel(const uint32_t* __restrict__ seedp, int N, int H, int W,
                                                           uint32_t lo16, uint32_t hi16, int32_t* __restrict__ boxes) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const uint32_t seed = seedp[0];
  uint64_t r[4], u[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r[j] = spcl::pxs_key(4u * (uint32_t)n + (uint32_t)j, seed);
    u[j] = r[j] >> 8;
  }
  const uint64_t P = lo16 + (((uint64_t)(hi16 - lo16) * u[0]) >> 24);  // the area share, 1 <= P <= 65536
  const uint64_t S = P + (((65536ull - P) * u[1]) >> 24);              // P <= S <= 65536
  const uint64_t T = (P * 65536ull) / S;                               // S T ~ P 65536
  const bool tall = (r[1] & 1ull) != 0ull;
  const uint64_t sh = tall ? S : T, sw = tall ? T : S;
  uint64_t bh = ((uint64_t)H * sh + 32768ull) >> 16, bw = ((uint64_t)W * sw + 32768ull) >> 16;
  bh = bh < 1ull ? 1ull : bh;
  bw = bw < 1ull ? 1ull : bw;
  bh = bh > (uint64_t)H ? (uint64_t)H : bh;
  bw = bw > (uint64_t)W ? (uint64_t)W : bw;
  const uint64_t y0 = (((uint64_t)H - bh + 1ull) * u[2]) >> 24, x0 = (((uint64_t)W - bw + 1ull) * u[3]) >> 24;
  int32_t* o = boxes + (size_t)n * 4;
  o[0] = (int32_t)y0;
  o[1] = (int32_t)x0;
  o[2] = (int32_t)bh;
  o[3] = (int32_t)bw;
}

// is (h, w) inside the box (y0, x0, bh, bw)?  Unsigned range compares on 32-bit words (the differences wrap, they never
// overflow): a negative or huge entry only changes the answer.
__device__ __forceinline__ bool in_box(int h, int w, int y0, int x0, int bh, int bw) {
  return (unsigned)h - (unsigned)y0 < (unsigned)bh && (unsigned)w - (unsigned)x0 < (unsigned)bw;
}

// ------------------------------------------------------------------------------------------------------------------ images
// E: an element as an unsigned integer of its size; V: elements per access (16 bytes, or 1).  A sample is [R][L] elements;
// element (r, l) lies in image row h = r % H and image column w = l / K (NCHW: R = C H, K = 1; channels-last: R = H, K = C).
// One thread per access: unit q of sample n, q < R * (L / V).
template <class E, int V>
__global__ void __launch_bounds__(256) cutmix_images_kernel(const E* __restrict__ x, E* __restrict__ out, unsigned N, unsigned R,
                                                            unsigned L, unsigned H, unsigned K,
                                                            const int32_t* __restrict__ boxes, unsigned roll,
                                                            unsigned units_per_sample, unsigned total_units) {
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  if (q >= total_units) return;
  const unsigned n = q / units_per_sample, rem = q - n * units_per_sample;
  const unsigned per_row = L / (unsigned)V;
  const unsigned r = rem / per_row, l0 = (rem - r * per_row) * (unsigned)V;
  const int h = (int)(r % H);
  const int y0 = boxes[n * 4u + 0u], x0 = boxes[n * 4u + 1u], bh = boxes[n * 4u + 2u], bw = boxes[n * 4u + 3u];
  unsigned m = n + roll;  // (roll < N: m < 2 N)
  if (m >= N) m -= N;
  const size_t sample = (size_t)R * L, at = (size_t)r * L + l0;
  const E* own = x + (size_t)n * sample + at;
  const E* other = x + (size_t)m * sample + at;
  E* dst = out + (size_t)n * sample + at;
  if (V == 1) {
    dst[0] = in_box(h, (int)(l0 / K), y0, x0, bh, bw) ? other[0] : own[0];
  } else {
    typedef E vec_t __attribute__((ext_vector_type(V)));
    vec_t a = *reinterpret_cast<const vec_t*>(own);
    bool any = false;
#pragma unroll
    for (int e = 0; e < V; ++e) any = any || in_box(h, (int)((l0 + (unsigned)e) / K), y0, x0, bh, bw);
    if (any) {
      const vec_t b = *reinterpret_cast<const vec_t*>(other);
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (in_box(h, (int)((l0 + (unsigned)e) / K), y0, x0, bh, bw)) a[e] = b[e];
    }
    *reinterpret_cast<vec_t*>(dst) = a;
  }
}

// --------------------------------------------------------------------------------------------------------------- criterion
constexpr int kSlab = 1024;  // pixels per workgroup (4 per thread)
constexpr int kND = 2;       // doubles per row: the term of a <- b, the term of b <- a
constexpr int kMaxC = 66;    // 4 C + 2 integers per row

struct cmx_args {
  const float* sa;
  const float* sb;
  const float* ta;
  const float* tb;
  const int32_t* boxes;  // (NULL: no mix)
  const float* tau;      // (NULL: every pixel is kept)
  double scale;          // weight / M
  float gs;              // (float)scale
  float* loss;
  float* parts;
  float* da;
  float* db;
  unsigned long long* hist;
  uint8_t* label_a;
  uint8_t* label_b;
  double* partial;  // [nblk][2]
  unsigned int* ticket;
  unsigned int* counts;  // [nblk][4 C + 2]
  long M;
  unsigned int HW;
  unsigned int W;
  unsigned int N;
  unsigned int roll;
  int C;
};

// a teacher's pixel: its label and whether it teaches (conf = 1 / z, the confidence of pseudo_label.hip and cross_pseudo.hip:
// the same helper, the same bits; a NaN confidence keeps nothing)
template <int CT>
__device__ __forceinline__ void cmx_teacher(const float* __restrict__ p, int C, const float* s_tau, int& y, bool& keep) {
  float t[16];
  load_pixel<CT>(p, C, t);
  y = argmax_logits(t, C);
  const float z = softmax_numerators(t, C);
  const float conf = 1.f / z;
  keep = conf >= s_tau[y];
}

// a student's pixel towards the label y: its own maximum and its logit at the label are taken before the logits become
// numerators, then cross_term (pixel_criterion.hpp: the sibling's arithmetic) gives the term and stores the gradient row
template <int CT>
__device__ __forceinline__ double cmx_student(const float* __restrict__ p, int y, bool keep, float gs, int C,
                                              float* __restrict__ dst) {
  float x[16];
  load_pixel<CT>(p, C, x);
  float xy = x[0], m = x[0];
#pragma unroll
  for (int k = 1; k < 16; ++k)
    if (k < C) {
      m = fmaxf(m, x[k]);
      if (k == y) xy = x[k];
    }
  const float z = softmax_numerators(x, C);
  return cross_term<CT>(x, z, m, xy, y, keep, gs, C, dst);
}

// CT = 4: C == 4 and the six maps 16-byte aligned (vector accesses); CT = 0: any C <= 16
template <int CT>
__global__ void __launch_bounds__(256) cross_pseudo_mixed_kernel(const cmx_args a) {
  const int C = CT ? CT : a.C;
  const int NC = 4 * C + 2;
  __shared__ float s_tau[16];
  __shared__ double s_wd[4][kND];
  __shared__ unsigned int s_wc[4][kMaxC];
  __shared__ double s_gd[256];
  __shared__ unsigned long long s_gc[256];
  __shared__ unsigned long long s_gi[256];
  __shared__ double s_tot[kND];
  __shared__ unsigned int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // no thresholds: conf >= 0 keeps every pixel whose confidence is a number
  if (tid < 16) s_tau[tid] = (a.tau && tid < C) ? a.tau[tid] : 0.f;
  __syncthreads();

  double ta = 0.0, tb = 0.0;
  unsigned int na[16], nb[16], ka[16], kb[16], agree = 0u, mixed = 0u;  // (wave-uniform)
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    na[k] = 0u;
    nb[k] = 0u;
    ka[k] = 0u;
    kb[k] = 0u;
  }
  const long base = (long)blockIdx.x * kSlab;
#pragma clang loop unroll_count(CT == 4 ? 4 : 1)
  for (int i = 0; i < kSlab / 256; ++i) {
    const long pix = base + i * 256 + tid;
    int yA = -1, yB = -2;
    bool keepA = false, keepB = false, inside = false;
    if (pix < a.M) {
      long tpix = pix;  // the teachers' pixel: the same position in sample n or (n + roll) mod N
      if (a.boxes) {
        const unsigned int p = (unsigned int)pix;  // (M < 2^31)
        const unsigned int n = p / a.HW, rem = p - n * a.HW;
        const unsigned int h = rem / a.W, w = rem - h * a.W;
        const int32_t* bx = a.boxes + (size_t)n * 4;
        inside = in_box((int)h, (int)w, bx[0], bx[1], bx[2], bx[3]);
        unsigned int m = n + a.roll;  // (roll < N: m < 2 N)
        if (m >= a.N) m -= a.N;
        if (inside) tpix = (long)m * a.HW + rem;
      }
      cmx_teacher<CT>(a.ta + tpix * C, C, s_tau, yA, keepA);
      cmx_teacher<CT>(a.tb + tpix * C, C, s_tau, yB, keepB);
      ta += cmx_student<CT>(a.sa + pix * C, yB, keepB, a.gs, C, a.da + pix * C);
      tb += cmx_student<CT>(a.sb + pix * C, yA, keepA, a.gs, C, a.db + pix * C);
      if (a.label_a) a.label_a[pix] = keepA ? (uint8_t)yA : (uint8_t)255;
      if (a.label_b) a.label_b[pix] = keepB ? (uint8_t)yB : (uint8_t)255;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < C) {
        na[k] += (unsigned int)__popcll(__ballot(yA == k));
        nb[k] += (unsigned int)__popcll(__ballot(yB == k));
        ka[k] += (unsigned int)__popcll(__ballot(keepA && yA == k));
        kb[k] += (unsigned int)__popcll(__ballot(keepB && yB == k));
      }
    agree += (unsigned int)__popcll(__ballot(yA == yB));  // (a thread past the end holds -1 and -2)
    mixed += (unsigned int)__popcll(__ballot(inside));
  }

  // wave -> workgroup: the butterfly gives every lane the wave's sum; lane 0 files it, one thread per statistic adds the waves
  ta = wave_butterfly_sum_d(ta);
  tb = wave_butterfly_sum_d(tb);
  if (lane == 0) {
    s_wd[wave][0] = ta;
    s_wd[wave][1] = tb;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < C) {
        s_wc[wave][k] = na[k];
        s_wc[wave][C + k] = nb[k];
        s_wc[wave][2 * C + k] = ka[k];
        s_wc[wave][3 * C + k] = kb[k];
      }
    s_wc[wave][4 * C] = agree;
    s_wc[wave][4 * C + 1] = mixed;
  }
  __syncthreads();
  if (tid < kND) {
    a.partial[(size_t)blockIdx.x * kND + tid] = ((s_wd[0][tid] + s_wd[1][tid]) + s_wd[2][tid]) + s_wd[3][tid];
  } else if (tid >= 64 && tid < 64 + NC) {
    const int j = tid - 64;
    a.counts[(size_t)blockIdx.x * NC + j] = s_wc[0][j] + s_wc[1][j] + s_wc[2][j] + s_wc[3][j];
  }
  // publish the row, then take a ticket (pixel_criterion.hpp)
  if (!rows_take_ticket(a.ticket, &s_last)) return;  // (uniform over the workgroup)

  // ------------------------------------------------------------------------------------------------------------ the close
  // rows_grouped_total's association with the SIBLING's column count 2 + 4 C + 1 (rows_grouped_total_x<true>: the inside-a-box
  // column rides with the thread of the agreement column and does not enter the grouping)
  double tot;
  unsigned long long n, nin;
  rows_grouped_total_x<true>(a.partial, a.counts, kND, NC - 1, s_gd, s_gc, s_gi, tot, n, nin);
  if (tid < kND + NC - 1) {
    if (tid < kND) {
      s_tot[tid] = tot;
      a.parts[tid] = (float)(tot * a.scale);
    } else {
      a.hist[tid - kND] = n;
      if (tid == kND + NC - 2) a.hist[NC - 1] = nin;
    }
  }
  __syncthreads();
  if (tid == 0) {
    a.loss[0] = (float)((s_tot[0] + s_tot[1]) * a.scale);
    *a.ticket = 0u;
  }
}

inline size_t cmx_nblk(long M) { return (size_t)((M + kSlab - 1) / kSlab); }

}  // namespace

extern "C" int spcl_cutmix_boxes(const uint32_t* seed, int N, int H, int W, int lo16, int hi16, int32_t* boxes, void* stream) {
  SPCL_CHECK_ARG(seed && boxes, "spcl_cutmix_boxes: null pointer");
  SPCL_CHECK_ARG(N >= 1 && N <= (1 << 20), "spcl_cutmix_boxes: N = %d (1 .. 2^20)", N);
  SPCL_CHECK_ARG(H > 0 && W > 0, "spcl_cutmix_boxes: bad shape (%d x %d)", H, W);
  SPCL_CHECK_ARG(1 <= lo16 && lo16 <= hi16 && hi16 <= 65536,
                 "spcl_cutmix_boxes: bad range (1 <= lo16 <= hi16 <= 65536, given %d, %d)", lo16, hi16);
  hipStream_t st = (hipStream_t)stream;
  spcl::prof_cost(16.0 * N + 4.0, 100.0 * N);
  SPCL_LAUNCH(cutmix_boxes_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, seed, N, H, W, (uint32_t)lo16,
              (uint32_t)hi16, boxes);
  SPCL_LAUNCH_CHECK("spcl_cutmix_boxes");
  return SPCL_OK;
}

extern "C" int spcl_cutmix_images(const void* x, void* out, int dtype, int N, int C, int H, int W, int channels_last,
                                  const int32_t* boxes, int roll, void* stream) {
  SPCL_CHECK_ARG(x && out && boxes, "spcl_cutmix_images: null pointer");
  SPCL_CHECK_ARG(dtype == SPCL_F32 || dtype == SPCL_BF16, "spcl_cutmix_images: bad dtype %d", dtype);
  SPCL_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0, "spcl_cutmix_images: bad shape");
  SPCL_CHECK_ARG((long)N * C * H * W < (1L << 31), "spcl_cutmix_images: too many elements");
  SPCL_CHECK_ARG(out != x, "spcl_cutmix_images: out and x are one buffer (an in-place gather races)");
  SPCL_CHECK_ARG(roll >= 1 && roll <= N - 1, "spcl_cutmix_images: roll = %d outside 1 .. N - 1 = %d", roll, N - 1);
  const unsigned es = dtype == SPCL_F32 ? 4u : 2u, vmax = 16u / es;
  const unsigned R = channels_last ? (unsigned)H : (unsigned)C * (unsigned)H;
  const unsigned L = channels_last ? (unsigned)W * (unsigned)C : (unsigned)W;
  const unsigned K = channels_last ? (unsigned)C : 1u;
  const bool vec = L % vmax == 0u && ((uintptr_t)x | (uintptr_t)out) % 16 == 0;
  const unsigned V = vec ? vmax : 1u;
  const unsigned per_sample = R * (L / V), total = (unsigned)N * per_sample;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((total + 255u) / 256u), block(256);
  spcl::prof_cost(2.0 * N * C * H * W * es, 0.0);
  if (dtype == SPCL_F32) {
    if (vec)
      SPCL_LAUNCH((cutmix_images_kernel<uint32_t, 4>), grid, block, 0, st, (const uint32_t*)x, (uint32_t*)out, (unsigned)N, R, L,
                  (unsigned)H, K, boxes, (unsigned)roll, per_sample, total);
    else
      SPCL_LAUNCH((cutmix_images_kernel<uint32_t, 1>), grid, block, 0, st, (const uint32_t*)x, (uint32_t*)out, (unsigned)N, R, L,
                  (unsigned)H, K, boxes, (unsigned)roll, per_sample, total);
  } else {
    if (vec)
      SPCL_LAUNCH((cutmix_images_kernel<uint16_t, 8>), grid, block, 0, st, (const uint16_t*)x, (uint16_t*)out, (unsigned)N, R, L,
                  (unsigned)H, K, boxes, (unsigned)roll, per_sample, total);
    else
      SPCL_LAUNCH((cutmix_images_kernel<uint16_t, 1>), grid, block, 0, st, (const uint16_t*)x, (uint16_t*)out, (unsigned)N, R, L,
                  (unsigned)H, K, boxes, (unsigned)roll, per_sample, total);
  }
  SPCL_LAUNCH_CHECK("spcl_cutmix_images");
  return SPCL_OK;
}

// [partials: nblk x 2 doubles][ticket, 64 bytes][counts: nblk x (4 C + 2) unsigned ints], nblk = ceil(N H W / 1024)
extern "C" size_t spcl_cross_pseudo_mixed_workspace_bytes(int N, int C, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0 || C < 1 || C > 16) return 0;
  if ((long)N * H * W >= (1L << 31)) return 0;
  const size_t nblk = cmx_nblk((long)N * H * W);
  return nblk * (size_t)kND * sizeof(double) + 64 + nblk * (size_t)(4 * C + 2) * sizeof(unsigned int);
}

extern "C" int spcl_cross_pseudo_ce_mixed(const float* s_a, const float* s_b, const float* t_a, const float* t_b, int N, int C,
                                          int H, int W, const int32_t* boxes, int roll, const float* tau, float weight,
                                          float* loss, float* parts, float* da, float* db, unsigned long long* hist,
                                          uint8_t* label_a, uint8_t* label_b, void* ws, size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(s_a && s_b && t_a && t_b && loss && parts && da && db && hist && ws, "spcl_cross_pseudo_ce_mixed: null pointer");
  SPCL_CHECK_ARG(N > 0 && H > 0 && W > 0 && C >= 1 && C <= 16, "spcl_cross_pseudo_ce_mixed: bad shape (C <= 16)");
  SPCL_CHECK_ARG((long)N * H * W < (1L << 31), "spcl_cross_pseudo_ce_mixed: too many pixels");
  SPCL_CHECK_ARG(da != db, "spcl_cross_pseudo_ce_mixed: da and db are one buffer");
  SPCL_CHECK_ARG(!boxes || (roll >= 1 && roll <= N - 1), "spcl_cross_pseudo_ce_mixed: roll = %d outside 1 .. N - 1 = %d", roll,
                 N - 1);
  const long M = (long)N * H * W;
  SPCL_CHECK_ARG(ws_bytes >= spcl_cross_pseudo_mixed_workspace_bytes(N, C, H, W),
                 "spcl_cross_pseudo_ce_mixed: workspace too small");
  SPCL_CHECK_ARG((uintptr_t)ws % 8 == 0, "spcl_cross_pseudo_ce_mixed: workspace not 8-byte aligned");
  const size_t nblk = cmx_nblk(M);
  hipStream_t st = (hipStream_t)stream;
  cmx_args a{};
  a.sa = s_a;
  a.sb = s_b;
  a.ta = t_a;
  a.tb = t_b;
  a.boxes = boxes;
  a.tau = tau;
  a.scale = (double)weight / (double)M;
  a.gs = (float)a.scale;
  a.loss = loss;
  a.parts = parts;
  a.da = da;
  a.db = db;
  a.hist = hist;
  a.label_a = label_a;
  a.label_b = label_b;
  a.partial = (double*)ws;
  a.ticket = (unsigned int*)((char*)ws + nblk * (size_t)kND * sizeof(double));
  a.counts = (unsigned int*)((char*)a.ticket + 64);
  a.M = M;
  a.HW = (unsigned int)H * (unsigned int)W;
  a.W = (unsigned int)W;
  a.N = (unsigned int)N;
  a.roll = boxes ? (unsigned int)roll : 0u;
  a.C = C;
  // No memset of the ticket (cross_pseudo.hip): the caller's workspace was zero-filled before its first use and the
  // closing workgroup leaves the ticket at zero.
  const bool vec = C == 4 && ((uintptr_t)s_a | (uintptr_t)s_b | (uintptr_t)t_a | (uintptr_t)t_b | (uintptr_t)da |
                              (uintptr_t)db) % 16 == 0;
  spcl::prof_cost(6.0 * M * C * 4 + (label_a ? (double)M : 0.0) + (label_b ? (double)M : 0.0), 100.0 * M * C);
  if (vec) SPCL_LAUNCH(cross_pseudo_mixed_kernel<4>, dim3((unsigned)nblk), dim3(256), 0, st, a);
  else SPCL_LAUNCH(cross_pseudo_mixed_kernel<0>, dim3((unsigned)nblk), dim3(256), 0, st, a);
  SPCL_LAUNCH_CHECK("spcl_cross_pseudo_ce_mixed");
  return SPCL_OK;
}
