// Largest connected component of every listed foreground class of class-coded label maps, per volume -- the post-processing
// step segmentation results are usually reported after (it is not in the reference; inference opts into it).  A component is a
// maximal set of voxels of ONE label value joined through 6-neighbour steps (+-z, +-y, +-x; D = 1: 4-neighbour per slice).
//
// Label equivalence (union-find) over parent[V * D*H*W] (uint32, linear voxel index INSIDE the volume, (z*H + y)*W + x).  A union
// always links the larger root under the smaller, so parents only decrease, every find loop ends, and the root of a component is
// its smallest linear index -- the tie-break key.  Five launches, integer atomics only, nothing read back, no allocation:
//   1. tiles    one workgroup per 32 x 64 tile of one slice, the tile's parents in LDS.  A wave holds one tile row: every voxel
//               starts at the first voxel of its horizontal run (one ballot), so only the vertical joins are unions (LDS
//               atomicMin).  The tile leaves flat: parent[i] = the smallest index of i's component inside the tile.  Voxels whose
//               label is not listed get the NONE mark and take no further part.  count[i] = 0 for the listed ones.
//   2. borders  one thread per voxel: joins across the tiles' left and top edges and across z.  Workgroups on different XCDs
//               work on the same trees here, so EVERY access to parent in this launch is an agent-scope atomic (relaxed load in
//               find, atomicMin in union); labels are only read.  A z join is skipped where the voxel to the left or the voxel
//               above has the label and the same label behind it: that neighbour is joined to this voxel in its slice, its partner
//               to this voxel's partner in theirs, so its join (made or, in turn, implied) implies this one -- a blob that
//               overlaps its continuation in the next slice costs a few joins, not one per voxel.
//   3. flatten  root[i] = find(i) (plain loads: parent is not written any more) and the components' sizes.  A workgroup of 2048
//               consecutive voxels first joins equal roots of neighbouring lanes (one ballot), then adds the runs into an LDS
//               hash table of its roots, then issues ONE global atomicAdd per (workgroup, root).  Roots (root == own index) are
//               counted per class the same way: one atomicAdd per (workgroup, class).
//   4. select   every root voxel offers (size << 32) | ~root for its class: maximum in LDS per workgroup, one global atomicMax
//               per (workgroup, class).  Largest size wins, equal sizes go to the smallest root.
//   5. write    out = label where the label is not listed (one read, one write) or the voxel's root won, else 0; kept_size.
// The result is a function of the input alone: integer min / add / max commute, so arrival order changes nothing.
#include "common.hpp"

namespace spcl {

constexpr int LCC_MAX_CLASSES = 15;
constexpr int LCC_TH = 32, LCC_TW = 64;            // the LDS tile: one wave = one tile row
constexpr int LCC_THREADS = 256;
constexpr int LCC_ROWS_PER_WAVE = LCC_TH / (LCC_THREADS / 64);
constexpr int LCC_CHUNK = 2048, LCC_PER_THREAD = LCC_CHUNK / LCC_THREADS;  // launches 3 to 5: voxels per workgroup
constexpr int LCC_HASH = 4096;                     // > 2 x the roots a chunk can hold: the probe always ends
constexpr uint32_t LCC_NONE = 0xFFFFFFFFu;         // parent of a voxel whose label is not listed; an empty hash slot

struct LccClasses {
  int n;
  int c[LCC_MAX_CLASSES];
};

static inline size_t lcc_round256(size_t v) { return (v + 255) / 256 * 256; }

__device__ __forceinline__ int lcc_class_of(const LccClasses& cl, int64_t label) {
  int k = -1;
#pragma unroll
  for (int j = 0; j < LCC_MAX_CLASSES; ++j)
    if (j < cl.n && label == (int64_t)cl.c[j]) k = j;
  return k;
}

// ---- union-find in LDS (launch 1): workgroup-scope atomics
__device__ __forceinline__ uint32_t lcc_lds_find(uint32_t* L, uint32_t a) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(L + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == a) return a;
    a = p;  // (p < a: parents only decrease)
  }
}
__device__ __forceinline__ void lcc_lds_union(uint32_t* L, uint32_t a, uint32_t b) {
  for (;;) {
    a = lcc_lds_find(L, a);
    b = lcc_lds_find(L, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == a) return;  // a was a root and now hangs under b
    a = old;               // somebody linked a under old (< a) first: old and b are still to be joined
  }
}

// ---- the same on the global array (launch 2): agent-scope atomics, nothing else touches parent in that launch
__device__ __forceinline__ uint32_t lcc_find_atomic(uint32_t* P, uint32_t a) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(P + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == a) return a;
    a = p;
  }
}
__device__ __forceinline__ void lcc_union_atomic(uint32_t* P, uint32_t a, uint32_t b) {
  for (;;) {
    a = lcc_find_atomic(P, a);
    b = lcc_find_atomic(P, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
}

// ---- 1. one tile of one slice
// grid (V * D * tiles_y * tiles_x), 256 threads: wave w holds tile rows w, w + 4, ..., lane = column
__global__ __launch_bounds__(LCC_THREADS) void lcc_tiles_kernel(const int64_t* __restrict__ labels, int D, int H, int W,
                                                                int tiles_y, int tiles_x, LccClasses cl, int n_outputs,
                                                                uint32_t* __restrict__ parent, uint32_t* __restrict__ count,
                                                                unsigned long long* __restrict__ best,
                                                                int32_t* __restrict__ n_components) {
  __shared__ uint32_t L[LCC_TH * LCC_TW];
  __shared__ uint8_t code[LCC_TH * LCC_TW];  // 1 + index in the class list, 0: not listed or outside the slice
  // (the per-(volume, class) words the later launches add into)
  const size_t gid = (size_t)blockIdx.x * LCC_THREADS + threadIdx.x;
  if (gid < (size_t)n_outputs) {
    best[gid] = 0ull;
    n_components[gid] = 0;
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int b = blockIdx.x;
  const int tx = b % tiles_x; b /= tiles_x;
  const int ty = b % tiles_y; b /= tiles_y;  // b = v * D + z
  const int z = b % D;
  const int x = tx * LCC_TW + lane, y0 = ty * LCC_TH;
  const size_t hw = (size_t)H * W;
  const size_t slice = (size_t)b * hw;             // offset of the slice in labels / parent / count
  const uint32_t zbase = (uint32_t)((size_t)z * hw);  // linear index of the slice's first voxel inside its volume
  uint8_t mine[LCC_ROWS_PER_WAVE];
  bool same_left[LCC_ROWS_PER_WAVE];
#pragma unroll
  for (int k = 0; k < LCC_ROWS_PER_WAVE; ++k) {
    const int ly = w + 4 * k, y = y0 + ly;
    int c = 0;
    if (y < H && x < W) c = lcc_class_of(cl, labels[slice + (size_t)y * W + x]) + 1;
    const int cleft = __shfl_up(c, 1, 64);
    same_left[k] = lane > 0 && c != 0 && c == cleft;
    const unsigned long long starts = __ballot(!same_left[k]);  // (bit 0 is always set)
    const int start = 63 - __clzll((long long)(starts & (~0ull >> (63 - lane))));
    mine[k] = (uint8_t)c;
    code[ly * LCC_TW + lane] = (uint8_t)c;
    L[ly * LCC_TW + lane] = c ? (uint32_t)(ly * LCC_TW + start) : LCC_NONE;
  }
  __syncthreads();
  // vertical joins: where the voxel above has the label, except where the voxel to the left makes the same join
#pragma unroll
  for (int k = 0; k < LCC_ROWS_PER_WAVE; ++k) {
    const int ly = w + 4 * k;
    const bool same_up = ly > 0 && mine[k] != 0 && code[(ly > 0 ? ly - 1 : 0) * LCC_TW + lane] == mine[k];
    const bool left_up = __shfl_up((int)same_up, 1, 64) != 0;
    if (same_up && !(same_left[k] && left_up)) lcc_lds_union(L, (uint32_t)(ly * LCC_TW + lane), (uint32_t)((ly - 1) * LCC_TW + lane));
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < LCC_ROWS_PER_WAVE; ++k) {
    const int ly = w + 4 * k, y = y0 + ly;
    if (y >= H || x >= W) continue;
    const size_t g = slice + (size_t)y * W + x;
    if (mine[k] == 0) {
      parent[g] = LCC_NONE;
      continue;
    }
    // local raster order inside a tile is the order of the linear indices: the smallest local index is the smallest global one
    const uint32_t r = lcc_lds_find(L, (uint32_t)(ly * LCC_TW + lane));
    parent[g] = zbase + (uint32_t)(y0 + (int)(r / LCC_TW)) * (uint32_t)W + (uint32_t)(tx * LCC_TW + (int)(r % LCC_TW));
    count[g] = 0u;
  }
}

// ---- 2. joins across tile edges and across z
// grid-stride over the V * N voxels, consecutive lanes = consecutive voxels
__global__ __launch_bounds__(LCC_THREADS) void lcc_borders_kernel(const int64_t* __restrict__ labels, int D, int H, int W,
                                                                  size_t total, LccClasses cl, uint32_t* parent) {
  const size_t hw = (size_t)H * W, N = hw * D;
  const size_t stride = (size_t)gridDim.x * LCC_THREADS;
  const int lane = threadIdx.x & 63;
  for (size_t base = (size_t)blockIdx.x * LCC_THREADS; base < total; base += stride) {  // (uniform over the workgroup)
    const size_t i = base + threadIdx.x;
    const bool valid = i < total;
    const size_t ic = valid ? i : total - 1;
    const size_t v = ic / N;
    const uint32_t idx = (uint32_t)(ic - v * N);
    const int z = (int)(idx / hw);
    const uint32_t rem = (uint32_t)(idx - (size_t)z * hw);
    const int y = (int)(rem / (uint32_t)W), x = (int)(rem - (uint32_t)y * (uint32_t)W);
    const int64_t lab = labels[ic];
    const bool listed = valid && lcc_class_of(cl, lab) >= 0;
    const bool same_z = listed && z > 0 && labels[ic - hw] == lab;
    // the lane to the left holds voxel i - 1: in the same row when x > 0 (lane 0 asks nobody and joins)
    const bool left_z = __shfl_up((int)same_z, 1, 64) != 0;
    const long long left_lab = __shfl_up((long long)lab, 1, 64);
    if (!listed) continue;
    uint32_t* P = parent + v * N;
    if (x > 0 && x % LCC_TW == 0 && labels[ic - 1] == lab) lcc_union_atomic(P, idx, idx - 1u);
    if (y > 0 && y % LCC_TH == 0 && labels[ic - W] == lab) lcc_union_atomic(P, idx, idx - (uint32_t)W);
    if (same_z && !(lane > 0 && x > 0 && left_z && (int64_t)left_lab == lab) &&
        !(y > 0 && labels[ic - W] == lab && labels[ic - W - hw] == lab))
      lcc_union_atomic(P, idx, idx - (uint32_t)hw);
  }
}

// ---- 3. roots and sizes
// grid (V * chunks), 256 threads, LCC_CHUNK consecutive voxels of one volume
__global__ __launch_bounds__(LCC_THREADS) void lcc_flatten_kernel(const int64_t* __restrict__ labels, size_t N, int chunks,
                                                                  LccClasses cl, const uint32_t* __restrict__ parent,
                                                                  uint32_t* __restrict__ root, uint32_t* __restrict__ count,
                                                                  int32_t* __restrict__ n_components) {
  __shared__ uint32_t keys[LCC_HASH];
  __shared__ uint32_t sums[LCC_HASH];
  __shared__ uint32_t roots_of[LCC_MAX_CLASSES + 1];
  for (int e = threadIdx.x; e < LCC_HASH; e += LCC_THREADS) {
    keys[e] = LCC_NONE;
    sums[e] = 0u;
  }
  if (threadIdx.x <= LCC_MAX_CLASSES) roots_of[threadIdx.x] = 0u;
  __syncthreads();
  const size_t v = blockIdx.x / chunks;
  const size_t first = (size_t)(blockIdx.x % chunks) * LCC_CHUNK;
  const uint32_t* __restrict__ P = parent + v * N;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < LCC_PER_THREAD; ++k) {
    const size_t idx = first + (size_t)k * LCC_THREADS + threadIdx.x;
    uint32_t r = LCC_NONE;
    if (idx < N) {
      r = P[idx];
      if (r != LCC_NONE) {
        for (uint32_t p = P[r]; p != r; p = P[r]) r = p;
        root[v * N + idx] = r;
        if (r == (uint32_t)idx) {
          const int c = lcc_class_of(cl, labels[v * N + idx]);
          atomicAdd(&roots_of[c < 0 ? LCC_MAX_CLASSES : c], 1u);
        }
      }
    }
    // neighbouring lanes with one root add as one
    const uint32_t prev = __shfl_up(r, 1, 64);
    const bool head = lane == 0 || r != prev;
    const unsigned long long heads = __ballot(head);
    if (head && r != LCC_NONE) {
      const unsigned long long after = lane < 63 ? heads >> (lane + 1) : 0ull;
      const uint32_t len = after ? (uint32_t)__ffsll((long long)after) : (uint32_t)(64 - lane);
      uint32_t h = (r * 2654435761u) >> 20;  // 12 bits
      for (;;) {
        const uint32_t old = atomicCAS(&keys[h], LCC_NONE, r);
        if (old == LCC_NONE || old == r) {
          atomicAdd(&sums[h], len);
          break;
        }
        h = (h + 1u) & (LCC_HASH - 1);
      }
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < LCC_HASH; e += LCC_THREADS)
    if (keys[e] != LCC_NONE) atomicAdd(&count[v * N + keys[e]], sums[e]);
  if (threadIdx.x < cl.n && roots_of[threadIdx.x] != 0u)
    atomicAdd(&n_components[v * cl.n + threadIdx.x], (int32_t)roots_of[threadIdx.x]);
}

// ---- 4. the winner of every (volume, class)
__global__ __launch_bounds__(LCC_THREADS) void lcc_select_kernel(const int64_t* __restrict__ labels, size_t N, int chunks,
                                                                 LccClasses cl, const uint32_t* __restrict__ parent,
                                                                 const uint32_t* __restrict__ count,
                                                                 unsigned long long* __restrict__ best) {
  __shared__ unsigned long long top[LCC_MAX_CLASSES + 1];
  if (threadIdx.x <= LCC_MAX_CLASSES) top[threadIdx.x] = 0ull;
  __syncthreads();
  const size_t v = blockIdx.x / chunks;
  const size_t first = (size_t)(blockIdx.x % chunks) * LCC_CHUNK;
#pragma unroll
  for (int k = 0; k < LCC_PER_THREAD; ++k) {
    const size_t idx = first + (size_t)k * LCC_THREADS + threadIdx.x;
    if (idx < N && parent[v * N + idx] == (uint32_t)idx) {  // a root (NONE is no index: N < 2^31)
      const int c = lcc_class_of(cl, labels[v * N + idx]);
      if (c >= 0)
        atomicMax(&top[c], ((unsigned long long)count[v * N + idx] << 32) | (unsigned long long)(~(uint32_t)idx));
    }
  }
  __syncthreads();
  if (threadIdx.x < cl.n && top[threadIdx.x] != 0ull) atomicMax(&best[v * cl.n + threadIdx.x], top[threadIdx.x]);
}

// ---- 5. the processed map
__global__ __launch_bounds__(LCC_THREADS) void lcc_write_kernel(const int64_t* __restrict__ labels, size_t N, int chunks,
                                                                LccClasses cl, const uint32_t* __restrict__ root,
                                                                const unsigned long long* __restrict__ best,
                                                                int64_t* __restrict__ out, int64_t* __restrict__ kept_size) {
  __shared__ uint32_t winner[LCC_MAX_CLASSES + 1];
  const size_t v = blockIdx.x / chunks;
  const int chunk = blockIdx.x % chunks;
  if (threadIdx.x < cl.n) {
    const unsigned long long b = best[v * cl.n + threadIdx.x];
    winner[threadIdx.x] = b ? ~(uint32_t)b : LCC_NONE;  // (no component: no voxel asks)
    if (chunk == 0) kept_size[v * cl.n + threadIdx.x] = (int64_t)(b >> 32);
  }
  __syncthreads();
  const size_t first = (size_t)chunk * LCC_CHUNK;
#pragma unroll
  for (int k = 0; k < LCC_PER_THREAD; ++k) {
    const size_t idx = first + (size_t)k * LCC_THREADS + threadIdx.x;
    if (idx >= N) continue;
    const int64_t lab = labels[v * N + idx];
    const int c = lcc_class_of(cl, lab);
    out[v * N + idx] = (c < 0 || root[v * N + idx] == winner[c]) ? lab : (int64_t)0;
  }
}

}  // namespace spcl

using namespace spcl;

static bool lcc_shape_ok(int V, int D, int H, int W, int n_classes) {
  if (V <= 0 || D <= 0 || H <= 0 || W <= 0 || n_classes < 1 || n_classes > LCC_MAX_CLASSES) return false;
  const long n = (long)D * H * W;
  if ((long)D * H >= (1L << 31) || n >= (1L << 31)) return false;
  const long tiles = (long)D * cdiv(H, LCC_TH) * cdiv(W, LCC_TW), chunks = (n + LCC_CHUNK - 1) / LCC_CHUNK;
  return (long)V * tiles < (1L << 31) && (long)V * chunks < (1L << 31) && (long)V * n_classes < (1L << 31);
}

extern "C" size_t spcl_largest_component_workspace_bytes(int V, int D, int H, int W, int n_classes) {
  if (!lcc_shape_ok(V, D, H, W, n_classes)) return 0;
  const size_t total = (size_t)V * D * H * W;
  return 3 * lcc_round256(total * sizeof(uint32_t)) + lcc_round256((size_t)V * n_classes * sizeof(unsigned long long));
}

extern "C" int spcl_largest_component(const int64_t* labels, int V, int D, int H, int W, int C, const int* classes,
                                      int n_classes, int64_t* out, int64_t* kept_size, int32_t* n_components, void* ws,
                                      size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(V > 0 && D > 0 && H > 0 && W > 0, "largest_component: bad shape (V %d, D %d, H %d, W %d)", V, D, H, W);
  SPCL_CHECK_ARG((long)D * H < (1L << 31) && (long)D * H * W < (1L << 31),
                 "largest_component: fewer than 2^31 voxels per volume (got %d x %d x %d)", D, H, W);
  SPCL_CHECK_ARG(C >= 2, "largest_component: at least two classes (background and one foreground class), got C = %d", C);
  SPCL_CHECK_ARG(classes && n_classes >= 1 && n_classes <= LCC_MAX_CLASSES, "largest_component: 1 to %d listed classes (got %d)",
                 LCC_MAX_CLASSES, n_classes);
  LccClasses cl;
  cl.n = n_classes;
  for (int k = 0; k < LCC_MAX_CLASSES; ++k) cl.c[k] = -1;
  for (int k = 0; k < n_classes; ++k) {
    SPCL_CHECK_ARG(classes[k] >= 1 && classes[k] < C, "largest_component: listed class %d is not in [1, %d) (0 is the fill value)",
                   classes[k], C);
    for (int j = 0; j < k; ++j) SPCL_CHECK_ARG(classes[j] != classes[k], "largest_component: class %d is listed twice", classes[k]);
    cl.c[k] = classes[k];
  }
  SPCL_CHECK_ARG(lcc_shape_ok(V, D, H, W, n_classes), "largest_component: too many volumes for one call (V %d)", V);
  SPCL_CHECK_ARG(labels && out && kept_size && n_components && ws, "largest_component: null pointer");
  const size_t N = (size_t)D * H * W, total = (size_t)V * N;
  {
    const uintptr_t a = (uintptr_t)labels, b = (uintptr_t)out, bytes = total * sizeof(int64_t);
    SPCL_CHECK_ARG(a + bytes <= b || b + bytes <= a, "largest_component: `out` may not alias `labels`");
  }
  SPCL_CHECK_ARG((uintptr_t)ws % 16 == 0 && ws_bytes >= spcl_largest_component_workspace_bytes(V, D, H, W, n_classes),
                 "largest_component: workspace of %zu bytes, 16-byte aligned",
                 spcl_largest_component_workspace_bytes(V, D, H, W, n_classes));
  hipStream_t st = (hipStream_t)stream;
  const size_t words = lcc_round256(total * sizeof(uint32_t));
  uint32_t* parent = (uint32_t*)ws;
  uint32_t* root = (uint32_t*)((char*)ws + words);
  uint32_t* count = (uint32_t*)((char*)ws + 2 * words);
  unsigned long long* best = (unsigned long long*)((char*)ws + 3 * words);
  const int tiles_y = cdiv(H, LCC_TH), tiles_x = cdiv(W, LCC_TW);
  const int tiles = V * D * tiles_y * tiles_x;  // (>= V: its 256 threads each cover the V * n_classes <= 15 V output words)
  const int chunks = (int)((N + LCC_CHUNK - 1) / LCC_CHUNK);
  const size_t border_blocks = (total + LCC_THREADS - 1) / LCC_THREADS;
  SPCL_LAUNCH(lcc_tiles_kernel, dim3(tiles), dim3(LCC_THREADS), 0, st, labels, D, H, W, tiles_y, tiles_x, cl, V * n_classes,
              parent, count, best, n_components);
  SPCL_LAUNCH(lcc_borders_kernel, dim3((unsigned)(border_blocks < (1u << 20) ? border_blocks : (1u << 20))), dim3(LCC_THREADS), 0,
              st, labels, D, H, W, total, cl, parent);
  SPCL_LAUNCH(lcc_flatten_kernel, dim3(V * chunks), dim3(LCC_THREADS), 0, st, labels, N, chunks, cl, (const uint32_t*)parent, root,
              count, n_components);
  SPCL_LAUNCH(lcc_select_kernel, dim3(V * chunks), dim3(LCC_THREADS), 0, st, labels, N, chunks, cl, (const uint32_t*)parent,
              (const uint32_t*)count, best);
  SPCL_LAUNCH(lcc_write_kernel, dim3(V * chunks), dim3(LCC_THREADS), 0, st, labels, N, chunks, cl, (const uint32_t*)root,
              (const unsigned long long*)best, out, kept_size);
  SPCL_LAUNCH_CHECK("largest_component");
  return SPCL_OK;
}
