// Boundary loss (Kervadec et al., MIDL 2019): signed Euclidean distance maps of the label batch, formed on the device inside
// the step (the labelled batch is rotated, cropped and flipped there: a precomputed map would be the map of other labels), and
// the criterion that consumes them (contrastyou/losses/boundary.py; not in the reference).
//
// For sample n and listed class c, m = (labels[n] == c).  d2(x) = the smallest integer (dy)^2 + (dx)^2 from pixel x to a pixel of
// the same slice whose membership in m differs from x's;
//   phi = +sqrt(d2) outside m, 1 - sqrt(d2) inside m (float64 square root, one rounding to f32; object pixels that touch the
//   background get 0), and 0 on the whole slice where no pixel of the opposite membership exists.
// The transform is surface.hip's separable one with every pixel a query:
//   1. columns  per (plane, column), plane = (n, class): TWO uint16 planes, the vertical distance to the nearest pixel inside m
//               and to the nearest pixel outside m (0xFFFF = the column has none), from 64-bit membership masks of column
//               segments (boundary_columns_kernel).
//   2. rows     one wave per (plane, row): both rows are staged in LDS as integer squares; every lane takes the minimum over
//               x' of (x - x')^2 + g(x')^2 against the plane OPPOSITE to its own membership, sweeping the whole row with
//               broadcast reads (boundary_rows_kernel has the three forms that were measured; the plain sweep ships).  A row
//               whose staged minimum of either plane is still "none" belongs to a slice without that membership (every
//               column lacks it): it is written as zeros without a search -- the absent / full rule, decided on the device.
// Exact integers (below 2^21), no atomics, nothing read back: the same input gives the same bits.
//
//   L_B = 1 / (N S H W) sum_{n, s, x} softmax(logits)[n, classes[s], x] phi[n, s, x];  loss = alpha L_B, alpha a device scalar
// forward: one thread per pixel (grid-stride), the C <= 16 logits in registers, float64 terms, one float64 partial per
// workgroup stored as a row; a second launch adds the rows in a fixed order (thread t its k consecutive rows in index order,
// thread 0 the 256 thread sums in index order) -- no ticket, no fence in the workgroups of the first launch (sup_dice).
// backward: one launch, dlogits = g p_k (a_k - sum_c a_c p_c), a_c = alpha phi_c / (N S H W) on a listed class, else 0.
#include "pixel_criterion.hpp"

#include <math.h>

namespace {

constexpr int BD_MAX_HW = 1024;      // uint16 column distances, int32 squares: (H-1)^2 + (W-1)^2 < 2^21 (surface.hip)
constexpr int BD_MAX_N = 1024;
constexpr int BD_MAX_CLASSES = 16;
constexpr int BD_NONE = 0xFFFF;      // "no such pixel in this column"
constexpr int BD_BIG = 1 << 30;      // its square: + (W-1)^2 stays below 2^31
constexpr int BD_BATCH = 8;          // label loads a thread issues together in the columns kernel
constexpr int BD_ROWS_PER_WG = 4;    // rows kernel: one wave per row
constexpr int BD_MAX_PARTIALS = 2048;  // workgroups of the forward's first launch

// which form of the row search ships (boundary_rows_kernel: 0 plain, 1 per-lane early exit, 2 chunk window; DESIGN.md
// "Boundary loss" has the three times)
#ifndef SPCL_BOUNDARY_ROWS_FORM
#define SPCL_BOUNDARY_ROWS_FORM 0
#endif

struct BdClasses {
  int c[BD_MAX_CLASSES];
};

static inline size_t bd_round256(size_t v) { return (v + 255) / 256 * 256; }

// ---- 1. the two vertical distances of every pixel
// grid (N S, ceil(W / 64)), block (64, BD_SEGS): plane p = n S + s writes uint16 planes 2 p (to the nearest pixel inside m) and
// 2 p + 1 (outside m).  A column is cut into BD_SEGS segments of T = ceil(H / BD_SEGS) <= 64 rows; thread (x, segment) loads its
// T labels -- independent loads, all of a column in flight at once -- into one 64-bit membership mask, the segments exchange
// the rows of their first and last pixel inside / outside m through LDS, and every row's two distances are bit scans of the
// mask (nearest set bit at or below, at or above) or the neighbouring segments' rows: no scan along the column, no value read
// back.  (The first version scanned the column down and up as surface_columns_kernel does, one thread per column with
// batches of 8 loads: 2 H / 8 dependent round trips to memory, 62 - 77 us at 224 rows whatever the batch; DESIGN.md.)
constexpr int BD_SEGS = 16;
constexpr int BD_FAR = 1 << 20;  // "no such row" (a distance from it is >= 2^20 - 1023: stored as BD_NONE)

__device__ __forceinline__ int bd_vertical(unsigned long long bits, int k, int y, int y0, int prev, int next) {
  const unsigned long long lo = bits & ((2ull << k) - 1ull), hi = bits >> k;
  const int below = lo ? y0 + 63 - __clzll((long long)lo) : prev;
  const int above = hi ? y + __ffsll((long long)hi) - 1 : next;
  const int d = y - below < above - y ? y - below : above - y;
  return d < BD_NONE ? d : BD_NONE;
}

__global__ __launch_bounds__(64 * BD_SEGS) void boundary_columns_kernel(const int64_t* __restrict__ labels, int S, int H, int W,
                                                                        BdClasses classes, uint16_t* __restrict__ planes) {
  __shared__ int last_in[BD_SEGS][64], first_in[BD_SEGS][64], last_out[BD_SEGS][64], first_out[BD_SEGS][64];
  const int p = blockIdx.x, tx = threadIdx.x, ty = threadIdx.y, x = blockIdx.y * 64 + tx;
  const int xc = x < W ? x : W - 1;  // (every thread reaches the barrier; the stores are masked)
  const int n = p / S, s = p - n * S;
  const int64_t c = classes.c[s];
  const size_t hw = (size_t)H * W;
  const int64_t* __restrict__ m = labels + (size_t)n * hw;
  const int T = (H + BD_SEGS - 1) / BD_SEGS;
  const int y0 = ty * T, cnt = y0 >= H ? 0 : (H - y0 < T ? H - y0 : T);
  unsigned long long in = 0ull;
  for (int k0 = 0; k0 < cnt; k0 += BD_BATCH) {
    bool b[BD_BATCH];
#pragma unroll
    for (int k = 0; k < BD_BATCH; ++k) b[k] = m[(size_t)(y0 + k0 + k < H ? y0 + k0 + k : H - 1) * W + xc] == c;
#pragma unroll
    for (int k = 0; k < BD_BATCH; ++k)
      if (k0 + k < cnt && b[k]) in |= 1ull << ((k0 + k) & 63);
  }
  const unsigned long long valid = cnt >= 64 ? ~0ull : (1ull << cnt) - 1ull, out = ~in & valid;
  last_in[ty][tx] = in ? y0 + 63 - __clzll((long long)in) : -BD_FAR;
  first_in[ty][tx] = in ? y0 + __ffsll((long long)in) - 1 : BD_FAR;
  last_out[ty][tx] = out ? y0 + 63 - __clzll((long long)out) : -BD_FAR;
  first_out[ty][tx] = out ? y0 + __ffsll((long long)out) - 1 : BD_FAR;
  __syncthreads();
  if (x >= W || cnt == 0) return;
  int prev_in = -BD_FAR, next_in = BD_FAR, prev_out = -BD_FAR, next_out = BD_FAR;
  for (int t = 0; t < BD_SEGS; ++t) {  // (rows grow with the segment: the last hit below, the first hit above)
    if (t < ty) {
      prev_in = last_in[t][tx] > prev_in ? last_in[t][tx] : prev_in;
      prev_out = last_out[t][tx] > prev_out ? last_out[t][tx] : prev_out;
    } else if (t > ty) {
      next_in = first_in[t][tx] < next_in ? first_in[t][tx] : next_in;
      next_out = first_out[t][tx] < next_out ? first_out[t][tx] : next_out;
    }
  }
  uint16_t* __restrict__ gin = planes + (size_t)p * 2 * hw;
  uint16_t* __restrict__ gout = gin + hw;
  for (int k = 0; k < cnt; ++k) {
    const int y = y0 + k;
    gin[(size_t)y * W + x] = (uint16_t)bd_vertical(in, k, y, y0, prev_in, next_in);
    gout[(size_t)y * W + x] = (uint16_t)bd_vertical(out, k, y, y0, prev_out, next_out);
  }
}

// ---- 2. row minima, the square root and the sign
__device__ __forceinline__ int bd_wave_min(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}
__device__ __forceinline__ int bd_wave_max(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

// grid (N S, ceil(H / 4)), 256 threads: wave w takes row blockIdx.y * 4 + w of plane blockIdx.x.  tin[w][x] / tout[w][x] = the
// square of the vertical distance to the nearest pixel inside / outside m; entries W .. round_up(W, 4) are "none" (the sweeps
// read four x' at a time).  A lane inside m searches tout, a lane outside m searches tin.
// kForm: BD_PLAIN every lane sweeps the whole row, 16-byte broadcast reads of four x': the plane(s) the 64-pixel chunk needs --
// a chunk whose lanes all have one membership (most of a slice) sweeps one plane, a mixed chunk both, and the lane picks its
// own at the end; BD_LANE_EXIT a lane walks outwards from its own column and stops at the first dx with dx^2 >= best (per-lane
// addresses, a divergent trip count: the wave runs as long as its farthest lane); BD_WINDOW the plain sweeps over the x' that
// can matter to SOME lane of the chunk: a lane's own column bounds its result, best <= t(x), so no x' with (x - x')^2 >= max
// over the chunk of t(x) changes any lane -- uniform loop bounds, the reads stay broadcasts.
enum { BD_PLAIN = 0, BD_LANE_EXIT = 1, BD_WINDOW = 2 };

// min over x' in [4 j0, 4 j1) of (x - x')^2 + t[x']
__device__ __forceinline__ int bd_sweep(const int* __restrict__ t, int x, int j0, int j1, int best) {
  const int4* __restrict__ t4 = reinterpret_cast<const int4*>(t);
  for (int j = j0; j < j1; ++j) {  // (the same address in every lane: a broadcast read)
    const int4 v = t4[j];
    const int d = x - 4 * j;
    const int a = __mul24(d, d) + v.x, b = __mul24(d - 1, d - 1) + v.y, c = __mul24(d - 2, d - 2) + v.z,
              e = __mul24(d - 3, d - 3) + v.w;
    const int ab = a < b ? a : b, ce = c < e ? c : e;
    best = ab < best ? ab : best;
    best = ce < best ? ce : best;
  }
  return best;
}

template <int kForm>
__global__ __launch_bounds__(256) void boundary_rows_kernel(const uint16_t* __restrict__ planes, int S, int H, int W,
                                                            float* __restrict__ phi) {
  __shared__ __attribute__((aligned(16))) int tin[BD_ROWS_PER_WG][BD_MAX_HW];
  __shared__ __attribute__((aligned(16))) int tout[BD_ROWS_PER_WG][BD_MAX_HW];
  const int p = blockIdx.x, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int y = blockIdx.y * BD_ROWS_PER_WG + w;
  const size_t hw = (size_t)H * W;
  const int W4 = (W + 3) & ~3;  // (<= BD_MAX_HW)
  int mn_in = BD_BIG, mn_out = BD_BIG;
  if (y < H) {
    const uint16_t* __restrict__ gin = planes + (size_t)p * 2 * hw + (size_t)y * W;
    const uint16_t* __restrict__ gout = gin + hw;
    for (int x = l; x < W4; x += 64) {
      const int a = x < W ? gin[x] : BD_NONE, b = x < W ? gout[x] : BD_NONE;
      const int qa = a == BD_NONE ? BD_BIG : a * a, qb = b == BD_NONE ? BD_BIG : b * b;
      tin[w][x] = qa;
      tout[w][x] = qb;
      mn_in = qa < mn_in ? qa : mn_in;
      mn_out = qb < mn_out ? qb : mn_out;
    }
  }
  __syncthreads();
  if (y >= H) return;
  mn_in = bd_wave_min(mn_in);
  mn_out = bd_wave_min(mn_out);
  const int n = p / S, s = p - n * S;
  float* __restrict__ out = phi + (((size_t)n * H + y) * W) * S + s;
  if (mn_in == BD_BIG || mn_out == BD_BIG) {  // (uniform over the wave) the slice has no pixel inside m, or none outside
    for (int x = l; x < W; x += 64) out[(size_t)x * S] = 0.f;
    return;
  }
  const int* __restrict__ ti = tin[w];
  const int* __restrict__ to = tout[w];
  for (int x0 = 0; x0 < W; x0 += 64) {
    const int x = x0 + l;
    const bool live = x < W;
    const int xc = live ? x : W - 1;
    const bool inside = ti[xc] == 0;  // the nearest pixel inside m is the pixel itself
    const int t0 = live ? (inside ? to[xc] : ti[xc]) : 0;  // the own column's candidate
    int best;
    if (kForm == BD_LANE_EXIT) {
      // clamped addresses: a clamped read is a real pixel at a lateral distance <= dx, so its candidate never undercuts
      // the true minimum, and every x' within the stopping radius is visited
      const int* __restrict__ t = inside ? to : ti;
      best = t0;
      const int reach = x > W - 1 - x ? x : W - 1 - x;
      for (int dx = 1; dx <= reach && dx * dx < best; ++dx) {
        const int q = dx * dx, va = q + t[x - dx > 0 ? x - dx : 0], vb = q + t[x + dx < W ? x + dx : W - 1];
        best = va < best ? va : best;
        best = vb < best ? vb : best;
      }
    } else {
      int j0 = 0, j1 = W4 >> 2;  // groups of four x'
      if (kForm == BD_WINDOW) {
        const int bound = bd_wave_max(t0);
        if (bound < BD_BIG) {  // (else a column without the opposite membership: the whole row)
          const int rad = (int)sqrtf((float)bound) + 1;  // rad^2 >= bound (bound < 2^21: the float square root is off by < 1)
          const int lo = x0 - rad > 0 ? x0 - rad : 0, hi = x0 + 63 + rad < W - 1 ? x0 + 63 + rad : W - 1;
          j0 = lo >> 2;
          j1 = (hi >> 2) + 1;
        }
      }
      const unsigned long long in_lanes = __ballot(live && inside), out_lanes = __ballot(live && !inside);
      const int start = kForm == BD_WINDOW ? t0 : BD_BIG;
      const int b_out = in_lanes ? bd_sweep(to, x, j0, j1, start) : BD_BIG;   // (uniform branches)
      const int b_in = out_lanes ? bd_sweep(ti, x, j0, j1, start) : BD_BIG;
      best = inside ? b_out : b_in;
    }
    if (live) {
      const double d = sqrt((double)best);
      out[(size_t)x * S] = best >= BD_BIG ? 0.f : (float)(inside ? 1.0 - d : d);
    }
  }
}

// ---- the criterion
struct boundary_args {
  const float* x;      // [M][C] logits
  const float* phi;    // [M][S]
  const float* alpha;  // device scalar
  const float* gscale; // nullable (backward)
  int slot[16];        // class k -> its column of phi, -1: not listed
  int C, S;
  long M;
  double inv;          // 1 / (N S H W)
  double* partial;     // [gridDim.x] (forward)
  float* dx;           // [M][C] (backward)
};

template <int CT>
__global__ void __launch_bounds__(256) boundary_sums_kernel(const boundary_args a) {
  __shared__ double sh[4];
  const int C = CT == 4 ? 4 : a.C, S = a.S;
  double term = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.M; i += (long)gridDim.x * 256) {
    float v[16];
    load_pixel<CT>(a.x + (size_t)i * C, C, v);
    const float z = softmax_numerators(v, C);
    const float* __restrict__ ph = a.phi + (size_t)i * S;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < C && a.slot[k] >= 0) term += (double)(v[k] / z) * (double)ph[a.slot[k]];
  }
  term = block_sum_d(term, sh);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = term;
}

// one workgroup: thread t adds rows [t k, (t + 1) k) in index order, thread 0 the 256 thread sums in index order
__global__ void __launch_bounds__(256) boundary_finish_kernel(const double* __restrict__ partial, int nblk, double inv,
                                                              const float* __restrict__ alpha, float* __restrict__ loss,
                                                              float* __restrict__ lb) {
  __shared__ double sums[256];
  const int k = (nblk + 255) / 256, t = threadIdx.x;
  double s = 0.0;
  for (int j = 0; j < k; ++j) {
    const int q = t * k + j;
    if (q < nblk) s += partial[q];
  }
  sums[t] = s;
  __syncthreads();
  if (t == 0) {
    double tot = 0.0;
    for (int j = 0; j < 256; ++j) tot += sums[j];
    const double v = tot * inv;
    lb[0] = (float)v;
    loss[0] = (float)((double)alpha[0] * v);
  }
}

template <int CT>
__global__ void __launch_bounds__(256) boundary_grad_kernel(const boundary_args a) {
  const int C = CT == 4 ? 4 : a.C, S = a.S;
  const float coef = (float)((double)a.alpha[0] * a.inv);
  const float gs = a.gscale ? a.gscale[0] : 1.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.M; i += (long)gridDim.x * 256) {
    float v[16], g[16];
    load_pixel<CT>(a.x + (size_t)i * C, C, v);
    const float z = softmax_numerators(v, C);
    const float* __restrict__ ph = a.phi + (size_t)i * S;
    float sgp = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < C) {
        v[k] /= z;
        g[k] = a.slot[k] >= 0 ? coef * ph[a.slot[k]] : 0.f;
        sgp = fmaf(g[k], v[k], sgp);
      }
    softmax_jacobian(v, sgp, g, C);
    if (a.gscale) {
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < C) g[k] *= gs;
    }
    store_pixel<CT>(a.dx + (size_t)i * C, C, g);
  }
}

inline bool sdm_shape_ok(int N, int H, int W, int S) {
  return N > 0 && N <= BD_MAX_N && H > 0 && W > 0 && H <= BD_MAX_HW && W <= BD_MAX_HW && S > 0 && S <= BD_MAX_CLASSES;
}

inline bool boundary_shape_ok(int N, int C, int H, int W) {
  return N > 0 && N <= BD_MAX_N && C >= 1 && C <= 16 && H > 0 && W > 0 && (long)N * H * W < (1L << 31);
}

inline int boundary_nblk(long M) {
  const long g = (M + 255) / 256;
  return (int)(g < BD_MAX_PARTIALS ? g : BD_MAX_PARTIALS);
}

// the class list -> slot[k]; refuses a class outside [0, C) or one listed twice
inline int boundary_slots(const char* name, const int* classes, int n_classes, int C, boundary_args* a) {
  SPCL_CHECK_ARG(classes && n_classes > 0 && n_classes <= C, "%s: 1 to C listed classes (got %d, C = %d)", name, n_classes, C);
  for (int k = 0; k < 16; ++k) a->slot[k] = -1;
  for (int s = 0; s < n_classes; ++s) {
    SPCL_CHECK_ARG(classes[s] >= 0 && classes[s] < C, "%s: class %d is not in [0, %d)", name, classes[s], C);
    SPCL_CHECK_ARG(a->slot[classes[s]] < 0, "%s: class %d is listed twice", name, classes[s]);
    a->slot[classes[s]] = s;
  }
  return SPCL_OK;
}

}  // namespace

extern "C" size_t spcl_signed_distance_workspace_bytes(int N, int H, int W, int n_classes) {
  if (!sdm_shape_ok(N, H, W, n_classes)) return 0;
  return bd_round256((size_t)N * n_classes * 2 * H * W * sizeof(uint16_t));
}

extern "C" int spcl_signed_distance_maps(const int64_t* labels, int N, int H, int W, const int* classes, int n_classes,
                                         float* phi, void* ws, size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(sdm_shape_ok(N, H, W, n_classes),
                 "signed_distance_maps: bad shape (N %d <= %d, H %d, W %d <= %d, %d classes <= %d)", N, BD_MAX_N, H, W,
                 BD_MAX_HW, n_classes, BD_MAX_CLASSES);
  SPCL_CHECK_ARG(labels && classes && phi && ws, "signed_distance_maps: null pointer");
  BdClasses cl;
  for (int s = 0; s < BD_MAX_CLASSES; ++s) cl.c[s] = -1;
  for (int s = 0; s < n_classes; ++s) {
    SPCL_CHECK_ARG(classes[s] >= 0, "signed_distance_maps: class %d is negative", classes[s]);
    for (int t = 0; t < s; ++t) SPCL_CHECK_ARG(classes[t] != classes[s], "signed_distance_maps: class %d is listed twice", classes[s]);
    cl.c[s] = classes[s];
  }
  SPCL_CHECK_ARG((uintptr_t)ws % 16 == 0 && ws_bytes >= spcl_signed_distance_workspace_bytes(N, H, W, n_classes),
                 "signed_distance_maps: workspace of %zu bytes, 16-byte aligned",
                 spcl_signed_distance_workspace_bytes(N, H, W, n_classes));
  hipStream_t st = (hipStream_t)stream;
  const int planes = N * n_classes;
  uint16_t* g = (uint16_t*)ws;
  SPCL_LAUNCH(boundary_columns_kernel, dim3(planes, spcl::cdiv(W, 64)), dim3(64, BD_SEGS), 0, st, labels, n_classes, H, W, cl,
              g);
  const dim3 grid(planes, spcl::cdiv(H, BD_ROWS_PER_WG));
  const int form = spcl::lab_env("SPCL_BOUNDARY_ROWS_FORM", SPCL_BOUNDARY_ROWS_FORM);
  if (form == BD_LANE_EXIT)
    SPCL_LAUNCH(boundary_rows_kernel<BD_LANE_EXIT>, grid, dim3(256), 0, st, (const uint16_t*)g, n_classes, H, W, phi);
  else if (form == BD_PLAIN)
    SPCL_LAUNCH(boundary_rows_kernel<BD_PLAIN>, grid, dim3(256), 0, st, (const uint16_t*)g, n_classes, H, W, phi);
  else
    SPCL_LAUNCH(boundary_rows_kernel<BD_WINDOW>, grid, dim3(256), 0, st, (const uint16_t*)g, n_classes, H, W, phi);
  SPCL_LAUNCH_CHECK("signed_distance_maps");
  return SPCL_OK;
}

extern "C" size_t spcl_boundary_workspace_bytes(int N, int H, int W) {
  if (!boundary_shape_ok(N, 1, H, W)) return 0;
  return bd_round256((size_t)boundary_nblk((long)N * H * W) * sizeof(double));
}

extern "C" int spcl_boundary_forward(const float* logits, const float* phi, const int* classes, int n_classes, int N, int C,
                                     int H, int W, const float* alpha, float* loss, float* lb, void* ws, size_t ws_bytes,
                                     void* stream) {
  SPCL_CHECK_ARG(logits && phi && alpha && loss && lb && ws, "spcl_boundary_forward: null pointer");
  SPCL_CHECK_ARG(boundary_shape_ok(N, C, H, W), "spcl_boundary_forward: bad shape (N <= 1024, C <= 16)");
  boundary_args a;
  if (int rc = boundary_slots("spcl_boundary_forward", classes, n_classes, C, &a)) return rc;
  SPCL_CHECK_ARG((uintptr_t)ws % 8 == 0 && ws_bytes >= spcl_boundary_workspace_bytes(N, H, W),
                 "spcl_boundary_forward: workspace too small or not 8-byte aligned");
  a.x = logits, a.phi = phi, a.alpha = alpha, a.gscale = nullptr;
  a.C = C, a.S = n_classes, a.M = (long)N * H * W;
  a.inv = 1.0 / ((double)a.M * (double)n_classes);
  a.partial = (double*)ws, a.dx = nullptr;
  const int nblk = boundary_nblk(a.M);
  hipStream_t st = (hipStream_t)stream;
  spcl::prof_cost((double)a.M * (C + n_classes) * 4.0, 0.0);
  if (C == 4 && (uintptr_t)logits % 16 == 0) SPCL_LAUNCH(boundary_sums_kernel<4>, dim3(nblk), dim3(256), 0, st, a);
  else SPCL_LAUNCH(boundary_sums_kernel<0>, dim3(nblk), dim3(256), 0, st, a);
  SPCL_LAUNCH(boundary_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)a.partial, nblk, a.inv, alpha, loss, lb);
  SPCL_LAUNCH_CHECK("spcl_boundary_forward");
  return SPCL_OK;
}

extern "C" int spcl_boundary_backward(const float* logits, const float* phi, const int* classes, int n_classes, int N, int C,
                                      int H, int W, const float* alpha, const float* gscale, float* dlogits, void* stream) {
  SPCL_CHECK_ARG(logits && phi && alpha && dlogits, "spcl_boundary_backward: null pointer");
  SPCL_CHECK_ARG(boundary_shape_ok(N, C, H, W), "spcl_boundary_backward: bad shape (N <= 1024, C <= 16)");
  boundary_args a;
  if (int rc = boundary_slots("spcl_boundary_backward", classes, n_classes, C, &a)) return rc;
  a.x = logits, a.phi = phi, a.alpha = alpha, a.gscale = gscale;
  a.C = C, a.S = n_classes, a.M = (long)N * H * W;
  a.inv = 1.0 / ((double)a.M * (double)n_classes);
  a.partial = nullptr, a.dx = dlogits;
  const long g = (a.M + 255) / 256;
  const int gx = (int)(g < 4096 ? g : 4096);
  spcl::prof_cost((double)a.M * (2 * C + n_classes) * 4.0, 0.0);
  if (C == 4 && ((uintptr_t)logits | (uintptr_t)dlogits) % 16 == 0)
    SPCL_LAUNCH(boundary_grad_kernel<4>, dim3(gx), dim3(256), 0, (hipStream_t)stream, a);
  else
    SPCL_LAUNCH(boundary_grad_kernel<0>, dim3(gx), dim3(256), 0, (hipStream_t)stream, a);
  SPCL_LAUNCH_CHECK("spcl_boundary_backward");
  return SPCL_OK;
}
