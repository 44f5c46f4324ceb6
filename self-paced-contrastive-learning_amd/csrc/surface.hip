// Surface-distance metrics of class-coded segmentation maps (SurfaceMeter: Hausdorff, percentile Hausdorff, average
// surface distance) as an exact separable Euclidean distance transform -- replaces contrastyou/meters/surface_meter.py:109-128
// (`_evalue`: one medpy call per (slice, class), each a host erosion + exact distance transform + gather) and
// contrastyou/meters/surface_distance.py (hausdorff_distance / mod_hausdorff_distance / average_surface_distance).
//
// Per (sample b, reported class c) there are two border sets, S0 = border(pred[b] == c) and S1 = border(target[b] == c), and
// two DIRECTED problems: dir 0 holds, for every pixel of S0, the distance to the nearest pixel of S1; dir 1 the converse.
// Four launches, nothing read back, cost independent of how many border pixels there are:
//   1. columns  one thread per (plane, column): a down and an up scan leave, for every pixel, the vertical distance to the
//               nearest border pixel of its column (uint16, 0xFFFF = none) -- plane (b, r, s) is built from S_s.  A pixel is
//               a border pixel iff it equals c and a 4-neighbour differs from c or lies outside the image (no one-hot).
//   2. rows     one wave per (directed problem, row): the row of the OTHER set's plane is staged in LDS as squared vertical
//               distances g(x')^2; for every border pixel x of the row (own plane == 0) the minimum over x' of
//               (x - x')^2 + g(x')^2 -- exact integers under unit spacing, (dx sx)^2 + (dy sy)^2 in float64 otherwise -- goes
//               to a dense float64 plane of squared distances (-1 where the pixel is no border pixel).  A 64-pixel chunk with
//               many border pixels gives every lane its own x (LDS reads broadcast); one with few splits x' over the lanes
//               and takes the minimum by wave shuffles.  Worst case H W W steps per problem.
//   3. reduce   one workgroup per directed problem over its dense plane: count, maximum (of the squares), the sum of the
//               distances in a FIXED order (same input, same bits), and the two order statistics of the percentile by an
//               exact radix select over the bit patterns of the non-negative float64 squares; the virtual index
//               (n - 1) * (q / 100) is formed here, n being known on the device only.
//   4. finish   one thread per (b, r): hd = sqrt(max), mhd = max of the two percentiles, asd = mean of the two directed means,
//               empty = a set has no pixel (the three values are NaN there).
//
// Volumes (spcl_surface_distances_3d: one problem per (scan, reported class), the n-D call surface_meter.py:118-127 makes when
// it is handed a [B, C, D, H, W] pair) run the same launches with a third axis: the column scan goes slice by slice with the
// 6-neighbour border test, one more pass ("depth") combines the squared in-slice column distances along z,
//   G(z, y, x) = min over z' of ((z - z') sz)^2 + (g(z', y, x) sy)^2,
// and the rows kernel reads a row of G instead of squaring g.  The squared distance is ((dz sz)^2 + (dy sy)^2) + (dx sx)^2,
// every product and sum rounded once (no FMA contraction on that path): rounding is monotone, so the separable minima equal
// the all-pairs minimum of that expression bit for bit.
#include "common.hpp"

#include <math.h>

namespace spcl {

constexpr int SURF_MAX_HW = 1024;    // uint16 column distances, int32 squared distances: (H-1)^2 + (W-1)^2 < 2^21
                                     // (volumes: D too, (D-1)^2 + (H-1)^2 + (W-1)^2 < 2^22)
constexpr int SURF_MAX_REPORT = 64;
constexpr int SURF_NONE = 0xFFFF;    // "no border pixel in this column"
constexpr int SURF_ROWS_PER_WG = 4;  // rows kernel: one wave per row
constexpr int SURF_SPARSE_MAX = 8;   // a 64-pixel chunk with at most this many border pixels splits x' over the lanes
constexpr int SURF_RED_THREADS = 1024;
constexpr int SURF_BATCH = 8;         // loads a thread keeps in flight in the column scan and in the reductions
constexpr int SURF_ZT = 8;           // depth pass (volumes): slices per thread
constexpr int SURF_STATS = 4;        // per directed problem: n, max of the squares, sum of the distances, percentile

struct SurfClasses {
  int c[SURF_MAX_REPORT];
};

static inline size_t surf_round256(size_t v) { return (v + 255) / 256 * 256; }

// ---- 1. vertical distance to the nearest border pixel of the column
// grid (planes, ceil(W / 64)), 64 threads: plane = (b * R + r) * 2 + s, s = 0: pred, 1: target
// kVolume: grid (planes * D, ceil(W / 64)), blockIdx.x = plane * D + z: slice z of volume b, a voxel is a border voxel iff it
// equals c and one of its SIX neighbours differs from c or lies outside the volume (D = 1: every voxel of the object)
template <bool kVolume>
__global__ __launch_bounds__(64) void surface_columns_kernel(const int64_t* __restrict__ pred,
                                                             const int64_t* __restrict__ target, int R, int D, int H, int W,
                                                             SurfClasses classes, uint16_t* __restrict__ planes) {
  const int plane = kVolume ? blockIdx.x / D : blockIdx.x, z = kVolume ? blockIdx.x % D : 0;
  const int x = blockIdx.y * 64 + threadIdx.x;
  if (x >= W) return;
  const int s = plane & 1, r = (plane >> 1) % R, b = (plane >> 1) / R;
  const int64_t c = classes.c[r];
  const size_t hw = (size_t)H * W;
  const int64_t* __restrict__ m = (s ? target : pred) + ((size_t)b * D + z) * hw;
  uint16_t* __restrict__ g = planes + ((size_t)plane * D + z) * hw;
  // the slices in front and behind (clamped into the volume, the flags masked below)
  const int64_t* __restrict__ mf = kVolume && z > 0 ? m - hw : m;
  const int64_t* __restrict__ mb = kVolume && z + 1 < D ? m + hw : m;
  const bool inner_z = kVolume && z > 0 && z + 1 < D;
  // rows go in batches of SURF_BATCH: the loads of a batch are independent and in flight together (addresses clamped into the
  // map, the flags masked afterwards), the scan over the batch then runs on registers -- one load per scan step would make
  // the launch a chain of memory latencies
  const int xl = x > 0 ? x - 1 : 0, xr = x + 1 < W ? x + 1 : W - 1;
  bool up = false, cur = m[x] == c;  // (outside the image counts as background)
  int d = SURF_NONE;
  for (int y0 = 0; y0 < H; y0 += SURF_BATCH) {
    bool down[SURF_BATCH], left[SURF_BATCH], right[SURF_BATCH], depth[SURF_BATCH];
#pragma unroll
    for (int k = 0; k < SURF_BATCH; ++k) {
      const int y = y0 + k < H ? y0 + k : H - 1, yd = y + 1 < H ? y + 1 : H - 1;
      down[k] = m[(size_t)yd * W + x] == c;
      left[k] = m[(size_t)y * W + xl] == c;
      right[k] = m[(size_t)y * W + xr] == c;
      depth[k] = !kVolume || ((mf[(size_t)y * W + x] == c) & (mb[(size_t)y * W + x] == c) & inner_z);  // (loads unconditional)
    }
#pragma unroll
    for (int k = 0; k < SURF_BATCH; ++k) {
      const int y = y0 + k;
      if (y < H) {
        const bool dn = y + 1 < H && down[k];
        const bool border = cur && !(up && dn && x > 0 && left[k] && x + 1 < W && right[k] && depth[k]);
        d = border ? 0 : (d + 1 < SURF_NONE ? d + 1 : SURF_NONE);
        g[(size_t)y * W + x] = (uint16_t)d;
        up = cur;
        cur = dn;
      }
    }
  }
  d = SURF_NONE;
  for (int y0 = H - 1; y0 >= 0; y0 -= SURF_BATCH) {
    int down_d[SURF_BATCH];
#pragma unroll
    for (int k = 0; k < SURF_BATCH; ++k) down_d[k] = g[(size_t)(y0 - k > 0 ? y0 - k : 0) * W + x];
#pragma unroll
    for (int k = 0; k < SURF_BATCH; ++k) {
      const int y = y0 - k;
      if (y >= 0) {
        d = down_d[k] == 0 ? 0 : (d + 1 < SURF_NONE ? d + 1 : SURF_NONE);
        if (d < down_d[k]) g[(size_t)y * W + x] = (uint16_t)d;
      }
    }
  }
}

// ---- 2. row minima
template <typename T> struct SurfDist;
template <> struct SurfDist<int> {  // unit spacing: exact integers
  static constexpr int kBig = 1 << 30;  // + (W-1)^2 (volumes: + (D-1)^2 + (W-1)^2) stays below 2^31
  __device__ static __forceinline__ int vertical(int g, double) { return g == SURF_NONE ? kBig : g * g; }
  __device__ static __forceinline__ int with(int dx, double, int v) { return dx * dx + v; }
  __device__ static __forceinline__ int plus(int d, double, int v) { return d * d + v; }
  __device__ static __forceinline__ int min(int a, int b) { return a < b ? a : b; }
  __device__ static __forceinline__ int big() { return kBig; }
};
template <> struct SurfDist<double> {
  __device__ static __forceinline__ double vertical(int g, double sy) {
    const double t = (double)g * sy;
    return g == SURF_NONE ? HUGE_VAL : t * t;
  }
  __device__ static __forceinline__ double with(int dx, double sx, double v) {
    const double t = (double)dx * sx;
    return t * t + v;
  }
  // volumes: (d s)^2 + v with the square and the sum rounded one after the other, never contracted to an FMA -- the all-pairs
  // expression ((dz sz)^2 + (dy sy)^2) + (dx sx)^2 in that order, bit for bit
  __device__ static __forceinline__ double plus(int d, double s, double v) {
#pragma clang fp contract(off)
    const double t = (double)d * s;
    const double q = t * t;
    return q + v;
  }
  __device__ static __forceinline__ double min(double a, double b) { return a < b ? a : b; }
  __device__ static __forceinline__ double big() { return HUGE_VAL; }
};
template <typename T, bool kVolume> __device__ __forceinline__ T surf_lateral(int dx, double sx, T v) {
  if constexpr (kVolume) return SurfDist<T>::plus(dx, sx, v);
  else return SurfDist<T>::with(dx, sx, v);
}

template <typename T> __device__ __forceinline__ T surf_wave_min(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = SurfDist<T>::min(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- 1b. volumes: combine the in-slice column distances along z
// grid (planes, ceil(HW / 256), ceil(D / SURF_ZT)), 256 threads: thread = one (y, x) of SURF_ZT consecutive slices -- lanes run
// along x, so every load and store of a wave is one contiguous segment whatever the stride between slices; the z' loop keeps
// SURF_BATCH independent loads in flight and the SURF_ZT running minima in registers (no LDS).  D steps per voxel.
template <typename T>
__global__ __launch_bounds__(256) void surface_depth_kernel(const uint16_t* __restrict__ planes, int D, int HW, double sz,
                                                            double sy, T* __restrict__ G) {
  const int plane = blockIdx.x;
  const int i = blockIdx.y * 256 + threadIdx.x;
  if (i >= HW) return;
  const int z0 = blockIdx.z * SURF_ZT;
  const uint16_t* __restrict__ g = planes + (size_t)plane * D * HW + i;
  T acc[SURF_ZT];
#pragma unroll
  for (int j = 0; j < SURF_ZT; ++j) acc[j] = SurfDist<T>::big();
  for (int zp0 = 0; zp0 < D; zp0 += SURF_BATCH) {
    int gv[SURF_BATCH];
#pragma unroll
    for (int k = 0; k < SURF_BATCH; ++k) gv[k] = g[(size_t)(zp0 + k < D ? zp0 + k : D - 1) * HW];
#pragma unroll
    for (int k = 0; k < SURF_BATCH; ++k) {
      const int zp = zp0 + k;
      if (zp < D) {
        const T v = SurfDist<T>::vertical(gv[k], sy);
#pragma unroll
        for (int j = 0; j < SURF_ZT; ++j) acc[j] = SurfDist<T>::min(acc[j], SurfDist<T>::plus(z0 + j - zp, sz, v));
      }
    }
  }
#pragma unroll
  for (int j = 0; j < SURF_ZT; ++j)
    if (z0 + j < D) G[((size_t)plane * D + z0 + j) * HW + i] = acc[j];
}

// grid (problems, ceil(H / 4)), 256 threads: wave w takes row blockIdx.y * 4 + w of directed problem (b, r, dir);
// its own border set is plane (b, r, dir), the other set's column distances are plane (b, r, 1 - dir)
// kVolume: grid (problems * ceil(H / 4)), H = D * H rows per problem; the other set's row comes from G (squared distances
// over z and y already) instead of being squared here
template <typename T, bool kVolume>
__global__ __launch_bounds__(256) void surface_rows_kernel(const uint16_t* __restrict__ planes, const T* __restrict__ G, int H,
                                                           int W, double sy, double sx, double* __restrict__ dense) {
  __shared__ T row[SURF_ROWS_PER_WG][SURF_MAX_HW];
  const int row_blocks = (H + SURF_ROWS_PER_WG - 1) / SURF_ROWS_PER_WG;
  const int p = kVolume ? blockIdx.x / row_blocks : blockIdx.x, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int y = (kVolume ? blockIdx.x % row_blocks : blockIdx.y) * SURF_ROWS_PER_WG + w;
  const size_t hw = (size_t)H * W;
  const uint16_t* __restrict__ own = planes + (size_t)p * hw;
  const uint16_t* __restrict__ other = planes + (size_t)(p ^ 1) * hw;
  if (y < H)
    for (int x = l; x < W; x += 64) {
      if constexpr (kVolume) row[w][x] = G[(size_t)(p ^ 1) * hw + (size_t)y * W + x];
      else row[w][x] = SurfDist<T>::vertical(other[(size_t)y * W + x], sy);
    }
  __syncthreads();
  if (y >= H) return;
  double* __restrict__ out = dense + (size_t)p * hw + (size_t)y * W;
  for (int x0 = 0; x0 < W; x0 += 64) {
    const int x = x0 + l;
    const bool isb = x < W && own[(size_t)y * W + x] == 0;
    unsigned long long mask = __ballot(isb);
    T best = SurfDist<T>::big();
    if (__popcll(mask) > SURF_SPARSE_MAX) {
      if (isb)
        for (int xp = 0; xp < W; ++xp) best = SurfDist<T>::min(best, surf_lateral<T, kVolume>(x - xp, sx, row[w][xp]));
    } else {
      while (mask) {
        const int j = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        T mn = SurfDist<T>::big();
        for (int xp = l; xp < W; xp += 64) mn = SurfDist<T>::min(mn, surf_lateral<T, kVolume>(x0 + j - xp, sx, row[w][xp]));
        mn = surf_wave_min(mn);
        if (l == j) best = mn;
      }
    }
    if (x < W) out[x] = isb ? (double)best : -1.0;
  }
}

// ---- 3. per directed problem: count, maximum, ordered sum, exact percentile
__device__ __forceinline__ unsigned long long surf_wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the bit patterns of entries i0, i0 + blockDim.x, ... of d[0 .. N) (all ones, a negative number, past the end): SURF_BATCH
// independent loads in flight per thread
__device__ __forceinline__ void surf_load_keys(const double* __restrict__ d, int N, int i0, unsigned long long* keys) {
#pragma unroll
  for (int u = 0; u < SURF_BATCH; ++u) {
    const int i = i0 + u * (int)blockDim.x;
    keys[u] = i < N ? (unsigned long long)__double_as_longlong(d[i]) : ~0ull;
  }
}

// the key (bit pattern) of the element of 0-based rank k among the non-negative entries of d[0 .. N): most significant byte
// first, one 256-bin histogram of the entries that share the prefix found so far per pass
__device__ unsigned long long surf_radix_select(const double* __restrict__ d, int N, unsigned long long k,
                                                unsigned* hist, unsigned long long* pick) {
  unsigned long long prefix = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0u;
    __syncthreads();
    const unsigned long long himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
    int run_digit = -1;
    unsigned run = 0u;  // equal digits in a row are counted in a register: the high bytes of near values are all alike
    for (int i0 = threadIdx.x; i0 < N; i0 += blockDim.x * SURF_BATCH) {
      unsigned long long keys[SURF_BATCH];
      surf_load_keys(d, N, i0, keys);
#pragma unroll
      for (int u = 0; u < SURF_BATCH; ++u) {
        const unsigned long long key = keys[u];
        if ((key >> 63) || ((key ^ prefix) & himask)) continue;
        const int digit = (int)((key >> shift) & 255ull);
        if (digit != run_digit) {
          if (run) atomicAdd(&hist[run_digit], run);
          run_digit = digit;
          run = 0u;
        }
        ++run;
      }
    }
    if (run) atomicAdd(&hist[run_digit], run);
    __syncthreads();
    if (threadIdx.x < 64) {  // lane l owns bins 4 l .. 4 l + 3
      const int l = threadIdx.x;
      const unsigned h0 = hist[4 * l], h1 = hist[4 * l + 1], h2 = hist[4 * l + 2], h3 = hist[4 * l + 3];
      unsigned long long incl = (unsigned long long)h0 + h1 + h2 + h3;
      const unsigned long long own = incl;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(incl, o, 64);
        if (l >= o) incl += t;
      }
      unsigned long long below = incl - own;
      if (below <= k && k < incl) {
        int bin = 4 * l;
        if (k >= below + h0) { below += h0; ++bin;
          if (k >= below + h1) { below += h1; ++bin;
            if (k >= below + h2) { below += h2; ++bin; } } }
        pick[0] = (unsigned long long)bin;
        pick[1] = k - below;
      }
    }
    __syncthreads();
    prefix |= pick[0] << shift;
    k = pick[1];
    __syncthreads();
  }
  return prefix;
}

// grid (problems), 1024 threads.  stats[p] = {n, max of the squares, sum of the distances, percentile of the distances}
__global__ __launch_bounds__(SURF_RED_THREADS) void surface_reduce_kernel(const double* __restrict__ dense, int N, double q,
                                                                          double* __restrict__ stats) {
  __shared__ unsigned hist[256];
  __shared__ unsigned long long pick[2];
  __shared__ double red_sum[SURF_RED_THREADS / 64], red_max[SURF_RED_THREADS / 64];
  __shared__ unsigned long long red_a[SURF_RED_THREADS / 64], red_b[SURF_RED_THREADS / 64];
  __shared__ double total[3];
  const int p = blockIdx.x, t = threadIdx.x, w = t >> 6, l = t & 63, nw = blockDim.x >> 6;
  const double* __restrict__ d = dense + (size_t)p * N;
  // count, maximum, sum: thread t adds its strided entries in index order, the wave a fixed butterfly, thread 0 the waves
  double sum = 0.0, mx = 0.0;
  unsigned long long cnt = 0ull;
  for (int i0 = t; i0 < N; i0 += blockDim.x * SURF_BATCH) {
    unsigned long long keys[SURF_BATCH];
    surf_load_keys(d, N, i0, keys);
#pragma unroll
    for (int u = 0; u < SURF_BATCH; ++u) {
      const double v = __longlong_as_double((long long)keys[u]);
      if (!(keys[u] >> 63)) {
        sum += sqrt(v);
        mx = v > mx ? v : mx;
        ++cnt;
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    const double m2 = __shfl_xor(mx, o, 64);
    mx = m2 > mx ? m2 : mx;
  }
  cnt = surf_wave_sum_u64(cnt);
  if (l == 0) { red_sum[w] = sum; red_max[w] = mx; red_a[w] = cnt; }
  __syncthreads();
  if (t == 0) {
    double s = 0.0, m = 0.0;
    unsigned long long c = 0ull;
    for (int i = 0; i < nw; ++i) { s += red_sum[i]; m = red_max[i] > m ? red_max[i] : m; c += red_a[i]; }
    total[0] = (double)c; total[1] = m; total[2] = s;
  }
  __syncthreads();
  const unsigned long long n = (unsigned long long)total[0];
  double* __restrict__ st = stats + (size_t)p * SURF_STATS;
  if (n == 0ull) {
    if (t == 0) { st[0] = 0.0; st[1] = 0.0; st[2] = 0.0; st[3] = 0.0; }
    return;
  }
  // numpy's linear percentile: virtual index (n - 1) * (q / 100), the two neighbouring order statistics, lerp
  const double vidx = (double)(n - 1ull) * (q / 100.0);
  unsigned long long lo = (unsigned long long)floor(vidx);
  if (lo > n - 1ull) lo = n - 1ull;
  const double frac = vidx - (double)lo;
  const unsigned long long hi = lo + 1ull < n ? lo + 1ull : n - 1ull;
  const unsigned long long key_lo = surf_radix_select(d, N, lo, hist, pick);
  // rank lo + 1: the same value when more than lo + 1 entries are <= it, else the smallest larger entry
  unsigned long long le = 0ull, next = ~0ull;
  for (int i0 = t; i0 < N; i0 += blockDim.x * SURF_BATCH) {
    unsigned long long keys[SURF_BATCH];
    surf_load_keys(d, N, i0, keys);
#pragma unroll
    for (int u = 0; u < SURF_BATCH; ++u) {
      if (keys[u] >> 63) continue;
      if (keys[u] <= key_lo) ++le;
      else if (keys[u] < next) next = keys[u];
    }
  }
  le = surf_wave_sum_u64(le);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long o2 = __shfl_xor(next, o, 64);
    next = o2 < next ? o2 : next;
  }
  if (l == 0) { red_a[w] = le; red_b[w] = next; }
  __syncthreads();
  if (t == 0) {
    unsigned long long c = 0ull, m = ~0ull;
    for (int i = 0; i < nw; ++i) { c += red_a[i]; m = red_b[i] < m ? red_b[i] : m; }
    const unsigned long long key_hi = (hi == lo || c > hi) ? key_lo : m;
    const double a = sqrt(__longlong_as_double((long long)key_lo)), b = sqrt(__longlong_as_double((long long)key_hi));
    const double diff = b - a;
    double pv = a + diff * frac;
    if (frac >= 0.5) pv = b - diff * (1.0 - frac);
    st[0] = total[0]; st[1] = total[1]; st[2] = total[2]; st[3] = pv;
  }
}

// ---- 4. the symmetric values of (b, r) from its two directed problems
__global__ __launch_bounds__(256) void surface_finish_kernel(const double* __restrict__ stats, int BR, double* __restrict__ hd,
                                                             double* __restrict__ mhd, double* __restrict__ asd,
                                                             uint8_t* __restrict__ empty) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= BR) return;
  const double* a = stats + (size_t)(2 * i) * SURF_STATS;
  const double* b = a + SURF_STATS;
  const bool none = a[0] == 0.0 || b[0] == 0.0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  empty[i] = none ? 1 : 0;
  hd[i] = none ? nan : sqrt(a[1] > b[1] ? a[1] : b[1]);
  mhd[i] = none ? nan : (a[3] > b[3] ? a[3] : b[3]);
  asd[i] = none ? nan : (a[2] / a[0] + b[2] / b[0]) / 2.0;
}

}  // namespace spcl

using namespace spcl;

extern "C" size_t spcl_surface_workspace_bytes(int B, int H, int W, int n_report) {
  if (B <= 0 || H <= 0 || W <= 0 || H > SURF_MAX_HW || W > SURF_MAX_HW || n_report <= 0 || n_report > SURF_MAX_REPORT) return 0;
  const size_t problems = (size_t)B * n_report * 2, hw = (size_t)H * W;
  return surf_round256(problems * hw * sizeof(uint16_t)) + surf_round256(problems * hw * sizeof(double)) +
         surf_round256(problems * SURF_STATS * sizeof(double));
}

extern "C" int spcl_surface_distances(const int64_t* pred, const int64_t* target, int B, int H, int W, int C, const int* report,
                                      int n_report, double sy, double sx, double percentile, double* hd, double* mhd,
                                      double* asd, uint8_t* empty, void* ws, size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0, "surface_distances: bad shape (B %d, H %d, W %d, C %d)", B, H, W, C);
  SPCL_CHECK_ARG(H <= SURF_MAX_HW && W <= SURF_MAX_HW, "surface_distances: maps of at most %d x %d (got %d x %d)", SURF_MAX_HW,
                 SURF_MAX_HW, H, W);
  SPCL_CHECK_ARG(report && n_report > 0 && n_report <= SURF_MAX_REPORT,
                 "surface_distances: 1 to %d reported classes (got %d)", SURF_MAX_REPORT, n_report);
  SurfClasses classes;
  for (int r = 0; r < n_report; ++r) {
    SPCL_CHECK_ARG(report[r] >= 0 && report[r] < C, "surface_distances: reported class %d is not in [0, %d)", report[r], C);
    classes.c[r] = report[r];
  }
  for (int r = n_report; r < SURF_MAX_REPORT; ++r) classes.c[r] = -1;
  SPCL_CHECK_ARG((long)B * n_report * 2 < (1L << 31), "surface_distances: too many (sample, class) pairs");
  SPCL_CHECK_ARG(sy > 0.0 && sx > 0.0 && sy < HUGE_VAL && sx < HUGE_VAL, "surface_distances: spacing must be positive and finite");
  SPCL_CHECK_ARG(percentile >= 0.0 && percentile <= 100.0, "surface_distances: percentile in [0, 100]");
  SPCL_CHECK_ARG(pred && target && hd && mhd && asd && empty && ws, "surface_distances: null pointer");
  SPCL_CHECK_ARG((uintptr_t)ws % 16 == 0 && ws_bytes >= spcl_surface_workspace_bytes(B, H, W, n_report),
                 "surface_distances: workspace of %zu bytes, 16-byte aligned", spcl_surface_workspace_bytes(B, H, W, n_report));
  hipStream_t st = (hipStream_t)stream;
  const int problems = B * n_report * 2;
  const size_t hw = (size_t)H * W;
  uint16_t* planes = (uint16_t*)ws;
  double* dense = (double*)((char*)ws + surf_round256((size_t)problems * hw * sizeof(uint16_t)));
  double* stats = (double*)((char*)dense + surf_round256((size_t)problems * hw * sizeof(double)));
  SPCL_LAUNCH(surface_columns_kernel<false>, dim3(problems, cdiv(W, 64)), dim3(64), 0, st, pred, target, n_report, 1, H, W,
              classes, planes);
  if (sy == 1.0 && sx == 1.0)
    SPCL_LAUNCH((surface_rows_kernel<int, false>), dim3(problems, cdiv(H, SURF_ROWS_PER_WG)), dim3(256), 0, st,
                (const uint16_t*)planes, (const int*)nullptr, H, W, sy, sx, dense);
  else
    SPCL_LAUNCH((surface_rows_kernel<double, false>), dim3(problems, cdiv(H, SURF_ROWS_PER_WG)), dim3(256), 0, st,
                (const uint16_t*)planes, (const double*)nullptr, H, W, sy, sx, dense);
  SPCL_LAUNCH(surface_reduce_kernel, dim3(problems), dim3(SURF_RED_THREADS), 0, st, (const double*)dense, (int)hw, percentile,
              stats);
  SPCL_LAUNCH(surface_finish_kernel, dim3(cdiv(B * n_report, 256)), dim3(256), 0, st, (const double*)stats, B * n_report, hd,
              mhd, asd, empty);
  SPCL_LAUNCH_CHECK("surface_distances");
  return SPCL_OK;
}

// ---- volumes
extern "C" size_t spcl_surface_3d_workspace_bytes(int V, int D, int H, int W, int n_report) {
  if (V <= 0 || D <= 0 || H <= 0 || W <= 0 || D > SURF_MAX_HW || H > SURF_MAX_HW || W > SURF_MAX_HW || n_report <= 0 ||
      n_report > SURF_MAX_REPORT)
    return 0;
  const size_t problems = (size_t)V * n_report * 2, n = (size_t)D * H * W;
  if (n >= ((size_t)1 << 31)) return 0;
  // column distances (u16), G (int32 under unit spacing, else f64: sized for f64), dense squared distances (f64), stats
  return surf_round256(problems * n * sizeof(uint16_t)) + 2 * surf_round256(problems * n * sizeof(double)) +
         surf_round256(problems * SURF_STATS * sizeof(double));
}

extern "C" int spcl_surface_distances_3d(const int64_t* pred, const int64_t* target, int V, int D, int H, int W, int C,
                                         const int* report, int n_report, double sz, double sy, double sx, double percentile,
                                         double* hd, double* mhd, double* asd, uint8_t* empty, void* ws, size_t ws_bytes,
                                         void* stream) {
  SPCL_CHECK_ARG(V > 0 && D > 0 && H > 0 && W > 0 && C > 0, "surface_distances_3d: bad shape (V %d, D %d, H %d, W %d, C %d)", V, D,
                 H, W, C);
  SPCL_CHECK_ARG(D <= SURF_MAX_HW && H <= SURF_MAX_HW && W <= SURF_MAX_HW,
                 "surface_distances_3d: volumes of at most %d x %d x %d (got %d x %d x %d)", SURF_MAX_HW, SURF_MAX_HW, SURF_MAX_HW,
                 D, H, W);
  SPCL_CHECK_ARG((long)D * H * W < (1L << 31), "surface_distances_3d: fewer than 2^31 voxels per volume (got %ld)",
                 (long)D * H * W);
  SPCL_CHECK_ARG(report && n_report > 0 && n_report <= SURF_MAX_REPORT,
                 "surface_distances_3d: 1 to %d reported classes (got %d)", SURF_MAX_REPORT, n_report);
  SurfClasses classes;
  for (int r = 0; r < n_report; ++r) {
    SPCL_CHECK_ARG(report[r] >= 0 && report[r] < C, "surface_distances_3d: reported class %d is not in [0, %d)", report[r], C);
    classes.c[r] = report[r];
  }
  for (int r = n_report; r < SURF_MAX_REPORT; ++r) classes.c[r] = -1;
  const long row_blocks = ((long)D * H + SURF_ROWS_PER_WG - 1) / SURF_ROWS_PER_WG;
  const long nproblems = (long)V * n_report * 2;  // (blockIdx.x holds problem * D + slice and problem * row_blocks + block)
  SPCL_CHECK_ARG(nproblems * D < (1L << 31) && nproblems * row_blocks < (1L << 31),
                 "surface_distances_3d: too many (volume, class) pairs");
  SPCL_CHECK_ARG(sz > 0.0 && sy > 0.0 && sx > 0.0 && sz < HUGE_VAL && sy < HUGE_VAL && sx < HUGE_VAL,
                 "surface_distances_3d: spacing must be positive and finite");
  SPCL_CHECK_ARG(percentile >= 0.0 && percentile <= 100.0, "surface_distances_3d: percentile in [0, 100]");
  SPCL_CHECK_ARG(pred && target && hd && mhd && asd && empty && ws, "surface_distances_3d: null pointer");
  SPCL_CHECK_ARG((uintptr_t)ws % 16 == 0 && ws_bytes >= spcl_surface_3d_workspace_bytes(V, D, H, W, n_report),
                 "surface_distances_3d: workspace of %zu bytes, 16-byte aligned",
                 spcl_surface_3d_workspace_bytes(V, D, H, W, n_report));
  hipStream_t st = (hipStream_t)stream;
  const int problems = (int)nproblems, rows = D * H, HW = H * W;
  const size_t n = (size_t)rows * W;
  uint16_t* planes = (uint16_t*)ws;
  void* G = (char*)ws + surf_round256((size_t)problems * n * sizeof(uint16_t));
  double* dense = (double*)((char*)G + surf_round256((size_t)problems * n * sizeof(double)));
  double* stats = (double*)((char*)dense + surf_round256((size_t)problems * n * sizeof(double)));
  SPCL_LAUNCH(surface_columns_kernel<true>, dim3(problems * D, cdiv(W, 64)), dim3(64), 0, st, pred, target, n_report, D, H, W,
              classes, planes);
  const dim3 depth_grid(problems, cdiv(HW, 256), cdiv(D, SURF_ZT)), rows_grid(problems * (int)row_blocks);
  if (sz == 1.0 && sy == 1.0 && sx == 1.0) {
    SPCL_LAUNCH(surface_depth_kernel<int>, depth_grid, dim3(256), 0, st, (const uint16_t*)planes, D, HW, sz, sy, (int*)G);
    SPCL_LAUNCH((surface_rows_kernel<int, true>), rows_grid, dim3(256), 0, st, (const uint16_t*)planes, (const int*)G, rows, W,
                sy, sx, dense);
  } else {
    SPCL_LAUNCH(surface_depth_kernel<double>, depth_grid, dim3(256), 0, st, (const uint16_t*)planes, D, HW, sz, sy, (double*)G);
    SPCL_LAUNCH((surface_rows_kernel<double, true>), rows_grid, dim3(256), 0, st, (const uint16_t*)planes, (const double*)G,
                rows, W, sy, sx, dense);
  }
  SPCL_LAUNCH(surface_reduce_kernel, dim3(problems), dim3(SURF_RED_THREADS), 0, st, (const double*)dense, (int)n, percentile,
              stats);
  SPCL_LAUNCH(surface_finish_kernel, dim3(cdiv(V * n_report, 256)), dim3(256), 0, st, (const double*)stats, V * n_report, hd,
              mhd, asd, empty);
  SPCL_LAUNCH_CHECK("surface_distances_3d");
  return SPCL_OK;
}
