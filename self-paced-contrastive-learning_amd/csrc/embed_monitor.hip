// Pre-training monitor: k-nearest neighbours, label votes, instance retrieval, alignment and uniformity of N embeddings in one
// sweep over the N x N similarity matrix, which is never stored (spcl_embed_monitor).  NOT in the reference.
//
// With zh_i = z_i / max(|z_i|, 1e-12) (F.normalize) and s_ij = zh_i . zh_j, the candidates of row i are all j != i (and
// j != pair[i] with exclude_pair).  Candidate a BEATS b when s_a > s_b, or s_a == s_b and a < b.
//   knn         the k candidates no other candidate beats, in that order
//   pred        the majority label among them; equal counts go to the label whose best-ranked neighbour comes first
//   pair_rank   the number of j not in {i, pair[i]} that beat pair[i]
// spcl_embed_monitor_grouped: with group[i] >= 0 the candidates of row i also leave out every j with group[j] == group[i]
// (a scan's cells are near-duplicates of each other); the groups enter the neighbour lists and nothing else.  The sweep tests
// one more predicate per candidate; spcl_embed_monitor is the same code with group == NULL.
//   alignment   the mean over paired rows of 2 - 2 s_i,pair;  uniformity  log mean_{i != j} exp(-4 (1 - s_ij))
//
// Four launches and (L > 0) one memset of `correct`:
//   emon_norm_kernel   one wave per row: |z_i| from a double sum of squares, zh into the workspace as [NP][DP] (NP, DP = N, d
//                      rounded up to 64, the padding zero: the tile loaders need no bounds);
//   emon_pair_kernel   s_i,pair for the 64 rows of a row block: the rows against their gathered pairs through the SAME MFMA
//                      chain as the sweep (only the diagonal 16 x 16 blocks), so that the sweep can count who beats the pair
//                      with the very bits it will meet at column pair[i];
//   emon_sweep_kernel  workgroup (row block rb, column split c): 64 x 64 tiles of S on the exact-f32 MFMA
//                      (v_mfma_f32_16x16x4_f32, as supcon_weighted.hip), contraction in the order 0 .. DP-1 of the padded
//                      row whatever the tile: s_ij == s_ji bitwise, and two equal rows give equal bits against any third.
//                      Each wave owns 16 rows; the running top-k of a row lives in registers, entry l in lane l (k <= 32):
//                      a tile's 64 candidates of the row are tested against the k-th entry, one per lane, and the few that
//                      pass are inserted in column order (one ballot for the position, one DPP lane shift).  The same pass adds
//                      exp(4 s - 4) into one double per lane and counts the candidates that beat the pair;
//   emon_close_kernel  one wave per row: the splits' lists merged by rank, the votes (lane t holds neighbour t's label),
//                      `correct` (integer atomics), pair_rank; workgroup 0 adds the uniformity partials, the alignment and the smallest norm in index order.
// Every floating-point sum runs in a fixed order: two runs give the same bits.  Nothing is read back or allocated.
#include <limits.h>
#include "common.hpp"

namespace spcl {

constexpr int EMON_MAX_N = 8192, EMON_MAX_D = 512, EMON_MAX_K = 32, EMON_MAX_L = 4, EMON_MAX_SPLIT = 8;
constexpr int EMON_SP = 65;        // row pitch of the S tile in LDS (reads of one row by 64 lanes, writes of the MFMA layout)
constexpr int EMON_EMPTY = INT_MAX;  // the index of an empty list entry (with -inf): every real candidate beats it

// (bitwise on purpose: no short-circuit branches inside the insertion loop)
__device__ __forceinline__ bool emon_beats(float sa, int ja, float sb, int jb) {
  return (sa > sb) | ((sa == sb) & (ja < jb));
}
// the row's other view, or -1 (a value outside [0, N) counts as none: nothing is indexed with it)
__device__ __forceinline__ int emon_pair_of(const int32_t* pair, int i, int N) {
  if (pair == nullptr) return -1;
  const int p = pair[i];
  return (p >= 0 && p < N) ? p : -1;
}

// into how many column splits a row block's sweep is dealt: until the grid has 768 workgroups (three per CU fit by their
// LDS, and the staging of one hides behind the products of the others), 8 at the most
static int emon_split(int N) {
  const int rb = cdiv(N, 64);
  int cs = 1;
  while (cs < EMON_MAX_SPLIT && 2 * cs <= rb && rb * cs < 768) cs *= 2;
  return cs;
}

struct EmonWs {
  double* usum;   // [RB][CS] partial sums of exp(4 s - 4)
  float* zh;      // [NP][DP]
  float* norm;    // [NP]
  float* spair;   // [NP]
  float* pl_s;    // [CS][NP][k]
  int* pl_j;      // [CS][NP][k]
  int* prank;     // [CS][NP]
  size_t bytes;
};
static EmonWs emon_ws(void* ws, int N, int d, int k) {
  const size_t NP = round_up(N, 64), DP = round_up(d, 64), RB = NP / 64, CS = emon_split(N);
  EmonWs w;
  char* p = (char*)ws;
  w.usum = (double*)p;  p += round_up((int)(RB * CS * sizeof(double)), 16);
  w.zh = (float*)p;     p += NP * DP * sizeof(float);
  w.norm = (float*)p;   p += NP * sizeof(float);
  w.spair = (float*)p;  p += NP * sizeof(float);
  w.pl_s = (float*)p;   p += CS * NP * k * sizeof(float);
  w.pl_j = (int*)p;     p += CS * NP * k * sizeof(int);
  w.prank = (int*)p;    p += CS * NP * sizeof(int);
  w.bytes = (size_t)(p - (char*)ws);
  return w;
}

// ------------------------------------------------------------------------------------------------ rows to unit length
__global__ __launch_bounds__(256) void emon_norm_kernel(const float* __restrict__ z, int64_t ldz, int N, int d, int DP,
                                                       float* __restrict__ zh, float* __restrict__ norm) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);  // row < NP (NP is a multiple of 4)
  const float* src = z + (size_t)row * ldz;
  double s2 = 0.0;
  if (row < N)
    for (int e = lane; e < d; e += 64) {
      const double v = (double)src[e];
      s2 = fma(v, v, s2);
    }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) s2 += __shfl_xor(s2, m, 64);
  const float nrm = (float)sqrt(s2);
  const float den = fmaxf(nrm, 1e-12f);
  for (int e = lane; e < DP; e += 64) zh[(size_t)row * DP + e] = (row < N && e < d) ? src[e] / den : 0.f;
  if (lane == 0) norm[row] = nrm;
}

// ------------------------------------------------------------------------------------------------ the tile product
// 64 rows x 64 features of zh into LDS, swizzled in 16-byte groups as supcon_weighted.hip's tiles; rows[r] < 0: a zero row
template <bool GATHER>
__device__ __forceinline__ void emon_stage(float* dst, const float* __restrict__ zh, int DP, int row0, const int* rows,
                                           int kc) {
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int idx = threadIdx.x + 256 * it, r = idx >> 4, q = idx & 15;
    const int row = GATHER ? rows[r] : row0 + r;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!GATHER || row >= 0) v = *(const f32x4*)(zh + (size_t)row * DP + kc + 4 * q);
    *(f32x4*)(dst + r * 64 + ((q ^ (r & 15)) << 2)) = v;
  }
}
// one 64-feature chunk: acc[c] += A rows 16 w .. x B rows 16 ct .. (ct = c, or ct0 with NCT == 1).  The ONE statement of the
// contraction order: both kernels go through it, chunk after chunk
template <int NCT>
__device__ __forceinline__ void emon_mma(const float* As, const float* Bs, int w, int r16, int g, int ct0, f32x4 (&acc)[NCT]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const f32x4 a4 = *(const f32x4*)(As + (16 * w + r16) * 64 + (((4 * s + g) ^ r16) << 2));
    f32x4 b4[NCT];
#pragma unroll
    for (int c = 0; c < NCT; ++c)
      b4[c] = *(const f32x4*)(Bs + (16 * (NCT == 1 ? ct0 : c) + r16) * 64 + (((4 * s + g) ^ r16) << 2));
    // (u outside c: the accumulators take turns, a chain's next product issues after the others' -- the order INSIDE every
    // chain, which is all the result depends on, stays s, then u)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int c = 0; c < NCT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u], b4[c][u], acc[c], 0, 0, 0);
  }
}

// ------------------------------------------------------------------------------------------------ s_i,pair
__global__ __launch_bounds__(256) void emon_pair_kernel(const float* __restrict__ zh, int DP, int N,
                                                       const int32_t* __restrict__ pair, float* __restrict__ spair) {
  __shared__ __attribute__((aligned(16))) float As[64 * 64];
  __shared__ __attribute__((aligned(16))) float Bs[64 * 64];
  __shared__ int prow[64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
  const int I0 = 64 * blockIdx.x;
  if (threadIdx.x < 64) prow[threadIdx.x] = I0 + threadIdx.x < N ? emon_pair_of(pair, I0 + threadIdx.x, N) : -1;
  __syncthreads();
  f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
  for (int kc = 0; kc < DP; kc += 64) {
    emon_stage<false>(As, zh, DP, I0, nullptr, kc);
    emon_stage<true>(Bs, zh, DP, 0, prow, kc);
    __syncthreads();
    emon_mma<1>(As, Bs, w, r16, g, w, acc);
    __syncthreads();
  }
  // acc[0][r] = (row 16 w + 4 g + r) . (pair of row 16 w + r16): the diagonal lies in the lanes with g == r16 / 4
  const int r = r16 & 3;
  const float v = r == 0 ? acc[0][0] : (r == 1 ? acc[0][1] : (r == 2 ? acc[0][2] : acc[0][3]));
  if (g == (r16 >> 2)) spair[I0 + 16 * w + r16] = prow[16 * w + r16] >= 0 ? v : 0.f;
}

// ------------------------------------------------------------------------------------------------ the sweep
struct EmonSweep {
  const float* zh;
  const int32_t* pair;
  const float* spair;
  const int32_t* group;  // [N] or NULL (spcl_embed_monitor): rows of one non-negative id are no candidates of each other
  float* pl_s;
  int* pl_j;
  int* prank;
  double* usum;
  int N, NP, DP, k, excl, tps;  // tps: column tiles per split
};

__global__ __launch_bounds__(256) void emon_sweep_kernel(EmonSweep a) {
  __shared__ __attribute__((aligned(16))) float As[64 * 64];
  __shared__ __attribute__((aligned(16))) float Bs[64 * 64];
  __shared__ float Ss[64 * EMON_SP];
  __shared__ int prow[64];
  __shared__ float sprow[64];
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
  const int I0 = 64 * blockIdx.x, cs = blockIdx.y;
  const int t0 = cs * a.tps, t1 = min(a.NP / 64, t0 + a.tps);
  if (threadIdx.x < 64) {
    const int i = I0 + threadIdx.x;
    prow[threadIdx.x] = i < a.N ? emon_pair_of(a.pair, i, a.N) : -1;
    sprow[threadIdx.x] = a.spair[i];
  }
  // the group id of row 16 w + (lane & 15): row R's id is one readlane away (an SGPR).  A row that leaves no group out
  // (a negative id, no group vector) holds INT_MIN, which no column holds -- theirs are clamped to >= -1 --, so that the
  // whole rule is ONE comparison per candidate
  int grow = (a.group != nullptr && I0 + 16 * w + r16 < a.N) ? a.group[I0 + 16 * w + r16] : -1;
  grow = grow < 0 ? INT_MIN : grow;
  float ls[16];  // entry `lane` of the top-k list of row 16 w + R
  int lj[16];
#pragma unroll
  for (int R = 0; R < 16; ++R) {
    ls[R] = -INFINITY;
    lj[R] = EMON_EMPTY;
  }
  int cnt = 0;      // lane R < 16: the candidates that beat the pair of row 16 w + R
  double us = 0.0;  // this lane's share of sum exp(4 s - 4)
  const int klast = a.k - 1;
  for (int t = t0; t < t1; ++t) {
    const int J0 = 64 * t;
    f32x4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // the group id of the tile's column `lane`, asked for with the tile: one value per lane, as the candidate is, and here
    // before the products (a copy in LDS read after them costs the kernel 17 VGPRs and its third wave per SIMD)
    const int gj = (a.group != nullptr && J0 + lane < a.N) ? max(a.group[J0 + lane], -1) : -1;
    for (int kc = 0; kc < a.DP; kc += 64) {
      emon_stage<false>(As, a.zh, a.DP, I0, nullptr, kc);
      emon_stage<false>(Bs, a.zh, a.DP, J0, nullptr, kc);
      __syncthreads();
      emon_mma<4>(As, Bs, w, r16, g, 0, acc);
      __syncthreads();
    }
    // acc[c][r] = S[16 w + 4 g + r][16 c + r16]: the wave's strip into LDS, then one row at a time, one column per lane
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) Ss[(16 * w + 4 * g + r) * EMON_SP + 16 * c + r16] = acc[c][r];
    __syncthreads();
    const int j = J0 + lane;
#pragma unroll
    for (int R = 0; R < 16; ++R) {
      const int i = I0 + 16 * w + R;
      if (i >= a.N) continue;  // (uniform in the wave)
      const float s = Ss[(16 * w + R) * EMON_SP + lane];
      const int p = prow[16 * w + R];
      const float sp = sprow[16 * w + R];
      const int gi = __builtin_amdgcn_readlane(grow, R);
      const bool real = j < a.N && j != i;
      const bool cand = gj != gi;  // (groups enter the neighbour lists only: not uniformity, not pair_rank)
      us += real ? (double)expf(fmaf(4.f, s, -4.f)) : 0.0;
      const bool notp = j != p;
      if (p >= 0) {
        const int nb = __popcll(__ballot(real && notp && emon_beats(s, j, sp, p)));
        cnt += lane == R ? nb : 0;
      }
      const float ks = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ls[R]), klast));
      const int kj = __builtin_amdgcn_readlane(lj[R], klast);
      unsigned long long m = __ballot(real && (notp || !a.excl) && cand && emon_beats(s, j, ks, kj));
      while (m != 0) {  // (uniform) the candidates that beat the k-th entry as it stood, in column order
        const int src = __builtin_ctzll(m);
        m &= m - 1;
        const float cv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s), src));
        const int cj = J0 + src;
        // the entries the candidate does not beat form a prefix of the sorted list: its length is the position
        const int pos = __popcll(__ballot((lane <= klast) & !emon_beats(cv, cj, ls[R], lj[R])));
        // entry l - 1 into lane l: one DPP move across the whole wave (wave_shr:1; lane 0 keeps its own).  pos == k (the
        // candidate no longer beats the k-th entry) only moves lanes past the list, which nobody reads
        const int up_j = __builtin_amdgcn_update_dpp(lj[R], lj[R], 0x138, 0xF, 0xF, false);
        const float up_s = __builtin_bit_cast(
            float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, ls[R]), __builtin_bit_cast(int, ls[R]), 0x138, 0xF, 0xF, false));
        ls[R] = lane > pos ? up_s : (lane == pos ? cv : ls[R]);
        lj[R] = lane > pos ? up_j : (lane == pos ? cj : lj[R]);
      }
    }
  }
#pragma unroll
  for (int R = 0; R < 16; ++R) {
    const int i = I0 + 16 * w + R;
    if (i < a.N && lane <= klast) {
      const size_t o = ((size_t)cs * a.NP + i) * a.k + lane;
      a.pl_s[o] = ls[R];
      a.pl_j[o] = lj[R];
    }
  }
  if (lane < 16) a.prank[(size_t)cs * a.NP + I0 + 16 * w + lane] = cnt;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) us += __shfl_xor(us, m, 64);
  if (lane == 0) red[w] = us;
  __syncthreads();
  if (threadIdx.x == 0) a.usum[(size_t)blockIdx.x * gridDim.y + cs] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ------------------------------------------------------------------------------------------------ the close
struct EmonClose {
  const float* pl_s;
  const int* pl_j;
  const int* prank;
  const double* usum;
  const float* norm;
  const float* spair;
  const int32_t* pair;
  const int32_t* labels;
  int N, NP, k, L, CS, nparts;
  int32_t* knn_idx;
  float* knn_sim;
  int32_t* pred;
  int32_t* correct;
  int32_t* pair_rank;
  double* scalars;
};

constexpr int EMON_CLOSE_ROWS = 16;  // rows (waves) per workgroup of the close

static __device__ double emon_block_sum(double v, double* red) {  // 16 waves, fixed order
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red[0];
  for (int q = 1; q < EMON_CLOSE_ROWS; ++q) t += red[q];
  return t;
}

// one wave per row.  The splits' lists (CS k <= 256 entries, column ranges disjoint, so no index twice) are merged by rank: an
// entry's place is the number of entries that beat it.  Then the vote, lane t holding the label of neighbour t.
__global__ __launch_bounds__(64 * EMON_CLOSE_ROWS) void emon_close_kernel(EmonClose a) {
  __shared__ float es[EMON_CLOSE_ROWS][256];
  __shared__ int ej[EMON_CLOSE_ROWS][256];
  __shared__ int nbl[EMON_CLOSE_ROWS][EMON_MAX_K];
  __shared__ int okc[EMON_MAX_L];
  __shared__ double red[EMON_CLOSE_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i = blockIdx.x * EMON_CLOSE_ROWS + w;
  const bool act = i < a.N;  // (uniform in the wave)
  const int ii = act ? i : 0;
  const int E = a.CS * a.k;
  if (tid < EMON_MAX_L) okc[tid] = 0;
  float s[4];
  int j[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = lane + 64 * q;
    s[q] = -INFINITY;
    j[q] = EMON_EMPTY;
    if (e < E) {
      const int c = e / a.k, h = e - c * a.k;
      const size_t o = ((size_t)c * a.NP + ii) * a.k + h;
      s[q] = a.pl_s[o];
      j[q] = a.pl_j[o];
    }
    es[w][e] = s[q];
    ej[w][e] = j[q];
  }
  if (lane < EMON_MAX_K) nbl[w][lane] = 0;
  __syncthreads();
  int rank[4] = {0, 0, 0, 0};
  for (int t = 0; t < E; ++t) {
    const float ts = es[w][t];
    const int tj = ej[w][t];
#pragma unroll
    for (int q = 0; q < 4; ++q) rank[q] += emon_beats(ts, tj, s[q], j[q]) ? 1 : 0;
  }
  int n_real = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool real = j[q] != EMON_EMPTY;
    n_real += __popcll(__ballot(real));
    if (real && rank[q] < a.k) {
      nbl[w][rank[q]] = j[q];
      if (act) {
        a.knn_idx[(size_t)i * a.k + rank[q]] = j[q];
        a.knn_sim[(size_t)i * a.k + rank[q]] = s[q];
      }
    }
  }
  const int kn = min(n_real, a.k);  // valid neighbours
  if (act && lane >= kn && lane < a.k) {
    a.knn_idx[(size_t)i * a.k + lane] = -1;
    a.knn_sim[(size_t)i * a.k + lane] = -INFINITY;
  }
  {
    int rk = lane < a.CS ? a.prank[(size_t)lane * a.NP + ii] : 0;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) rk += __shfl_xor(rk, m, 64);
    if (act && lane == 0) a.pair_rank[i] = emon_pair_of(a.pair, i, a.N) >= 0 ? rk : -1;
  }
  __syncthreads();
  for (int l = 0; l < a.L; ++l) {
    const int32_t* lb = a.labels + (size_t)l * a.N;
    const int my = lane < kn ? lb[nbl[w][lane]] : -1;
    int c = 0;
    bool first = true;
    for (int u = 0; u < kn; ++u) {
      const bool same = __shfl(my, u, 64) == my;
      c += same ? 1 : 0;
      first = first && !(same && u < lane);
    }
    // a label is scored at its best-ranked neighbour: the count, then the earlier rank
    int score = (lane < kn && first) ? c * 64 + (63 - lane) : -1;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) score = max(score, __shfl_xor(score, m, 64));
    const int best = kn > 0 ? __shfl(my, 63 - (score & 63), 64) : -1;
    if (act && lane == 0) {
      a.pred[(size_t)l * a.N + i] = best;
      if (kn > 0 && best == lb[i]) atomicAdd(&okc[l], 1);
    }
  }
  __syncthreads();
  if (tid < a.L && okc[tid] > 0) atomicAdd(&a.correct[tid], okc[tid]);
  if (blockIdx.x != 0) return;
  // the scalars: strided double sums, then the fixed tree
  constexpr int NT = 64 * EMON_CLOSE_ROWS;
  double u = 0.0, al = 0.0, np = 0.0;
  float mn = INFINITY;
  for (int q = tid; q < a.nparts; q += NT) u += a.usum[q];
  for (int r = tid; r < a.N; r += NT) {
    if (emon_pair_of(a.pair, r, a.N) >= 0) {
      al += 2.0 - 2.0 * (double)a.spair[r];
      np += 1.0;
    }
    mn = fminf(mn, a.norm[r]);
  }
  u = emon_block_sum(u, red);
  al = emon_block_sum(al, red);
  np = emon_block_sum(np, red);
  double mnd = (double)mn;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) mnd = fmin(mnd, __shfl_xor(mnd, m, 64));
  __syncthreads();
  if (lane == 0) red[w] = mnd;
  __syncthreads();
  if (tid == 0) {
    for (int q = 1; q < EMON_CLOSE_ROWS; ++q) mnd = fmin(mnd, red[q]);
    a.scalars[0] = np > 0.0 ? al / np : __builtin_nan("");
    a.scalars[1] = log(u / ((double)a.N * (double)(a.N - 1)));
    a.scalars[2] = np;
    a.scalars[3] = fmin(mnd, red[0]);
  }
}

// ------------------------------------------------------------------------------------------------ the label of a pooled cell
// spcl_cell_majority: the majority class of every window of nn.AdaptiveAvgPool2d((sh, sw)) over uint8 label maps -- the label
// of a row of DenseProjectionHead's output.  One wave per cell: 64 pixels of the window at a time, a class's count grows by the
// popcount of one ballot, so the C counts are wave-uniform integers (no atomics, no floating-point sum, the same bits every run).
constexpr int CMAJ_MAX_C = 16, CMAJ_MAX_HW = 32768;  // ((u + 1) H + sh - 1 <= H^2 + H stays an int)

__global__ __launch_bounds__(256) void cmaj_kernel(const uint8_t* __restrict__ labels, int cells, int H, int W, int C, int sh,
                                                  int sw, int32_t* __restrict__ cell_label, float* __restrict__ purity) {
  const int lane = threadIdx.x & 63, cell = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cell >= cells) return;  // (uniform in the wave)
  const int v = cell % sw, u = (cell / sw) % sh, n = cell / (sw * sh);
  const int r0 = (u * H) / sh, r1 = ((u + 1) * H + sh - 1) / sh, c0 = (v * W) / sw, c1 = ((v + 1) * W + sw - 1) / sw;
  const int ww = c1 - c0, size = (r1 - r0) * ww;  // rows r0 .. r1 - 1, columns c0 .. c1 - 1, all inside the map
  const uint8_t* src = labels + (size_t)n * H * W;
  int cnt[CMAJ_MAX_C];
#pragma unroll
  for (int c = 0; c < CMAJ_MAX_C; ++c) cnt[c] = 0;
  for (int e0 = 0; e0 < size; e0 += 64) {
    const int e = e0 + lane;
    int val = 255;  // (a lane past the window: counted for no class, as every value >= C is)
    if (e < size) {
      const int r = e / ww;
      val = src[(size_t)(r0 + r) * W + c0 + (e - r * ww)];
    }
#pragma unroll
    for (int c = 0; c < CMAJ_MAX_C; ++c) cnt[c] += __popcll(__ballot(val == c));
  }
  int best = -1, most = 0;
#pragma unroll
  for (int c = 0; c < CMAJ_MAX_C; ++c)
    if (c < C && cnt[c] > most) {  // (strict: equal counts stay with the lower class)
      most = cnt[c];
      best = c;
    }
  if (lane == 0) {
    cell_label[cell] = best;
    if (purity != nullptr) purity[cell] = __fdiv_rn((float)most, (float)size);
  }
}

}  // namespace spcl

using namespace spcl;

static bool emon_shape_ok(int N, int d, int k) {
  return N >= 2 && N <= EMON_MAX_N && d >= 1 && d <= EMON_MAX_D && k >= 1 && k <= EMON_MAX_K;
}

extern "C" size_t spcl_embed_monitor_workspace_bytes(int N, int d, int k) {
  if (!emon_shape_ok(N, d, k)) return 0;
  return emon_ws(nullptr, N, d, k).bytes;
}

// the one code path of both entries: `what` names the entry in the messages, `group` is NULL for spcl_embed_monitor
static int emon_run(const char* what, const float* z, int64_t ldz, const int32_t* labels, int L, const int32_t* pair,
                    const int32_t* group, int N, int d, int k, int exclude_pair, int32_t* knn_idx, float* knn_sim, int32_t* pred,
                    int32_t* correct, int32_t* pair_rank, double* scalars, void* ws, size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(emon_shape_ok(N, d, k), "%s: N = %d (2 .. %d), d = %d (1 .. %d), k = %d (1 .. %d)", what, N,
                 EMON_MAX_N, d, EMON_MAX_D, k, EMON_MAX_K);
  SPCL_CHECK_ARG(L >= 0 && L <= EMON_MAX_L, "%s: L = %d label kinds (0 .. %d)", what, L, EMON_MAX_L);
  SPCL_CHECK_ARG(ldz >= d, "%s: row pitch %ld below d = %d", what, (long)ldz, d);
  SPCL_CHECK_ARG(z && knn_idx && knn_sim && pair_rank && scalars && ws, "%s: null pointer", what);
  SPCL_CHECK_ARG(L == 0 || (labels && pred && correct), "%s: null pointer (labels, pred or correct with L = %d)", what,
                 L);
  SPCL_CHECK_ARG((uintptr_t)ws % 16 == 0 && (uintptr_t)scalars % 8 == 0, "%s: misaligned workspace or scalars", what);
  const EmonWs w = emon_ws(ws, N, d, k);
  SPCL_CHECK_ARG(ws_bytes >= w.bytes, "%s: workspace of %zu bytes, %zu needed", what, ws_bytes, w.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int NP = round_up(N, 64), DP = round_up(d, 64), RB = NP / 64, CS = emon_split(N);
  if (L > 0 && hipMemsetAsync(correct, 0, (size_t)L * sizeof(int32_t), st) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: memset failed", what);
    return SPCL_ELAUNCH;
  }
  SPCL_LAUNCH(emon_norm_kernel, dim3(NP / 4), dim3(256), 0, st, z, ldz, N, d, DP, w.zh, w.norm);
  SPCL_LAUNCH(emon_pair_kernel, dim3(RB), dim3(256), 0, st, (const float*)w.zh, DP, N, pair, w.spair);
  const EmonSweep sw{w.zh, pair, w.spair, group, w.pl_s, w.pl_j, w.prank, w.usum, N, NP, DP, k, exclude_pair ? 1 : 0, cdiv(RB, CS)};
  prof_cost((double)RB * NP * DP * 8.0, 2.0 * NP * NP * DP);
  SPCL_LAUNCH(emon_sweep_kernel, dim3(RB, CS), dim3(256), 0, st, sw);
  const EmonClose cl{w.pl_s, w.pl_j, w.prank, w.usum, w.norm, w.spair, pair, labels, N, NP, k, L, CS, RB * CS,
                     knn_idx, knn_sim, pred, correct, pair_rank, scalars};
  SPCL_LAUNCH(emon_close_kernel, dim3(cdiv(N, EMON_CLOSE_ROWS)), dim3(64 * EMON_CLOSE_ROWS), 0, st, cl);
  SPCL_LAUNCH_CHECK(what);
  return SPCL_OK;
}

extern "C" int spcl_embed_monitor(const float* z, int64_t ldz, const int32_t* labels, int L, const int32_t* pair, int N, int d,
                                  int k, int exclude_pair, int32_t* knn_idx, float* knn_sim, int32_t* pred,
                                  int32_t* correct, int32_t* pair_rank, double* scalars, void* ws, size_t ws_bytes,
                                  void* stream) {
  return emon_run("spcl_embed_monitor", z, ldz, labels, L, pair, nullptr, N, d, k, exclude_pair, knn_idx, knn_sim, pred, correct,
                  pair_rank, scalars, ws, ws_bytes, stream);
}

// (the workspace is that of spcl_embed_monitor: the group ids are read where they lie)
extern "C" int spcl_embed_monitor_grouped(const float* z, int64_t ldz, const int32_t* labels, int L, const int32_t* pair,
                                          const int32_t* group, int N, int d, int k, int exclude_pair, int32_t* knn_idx,
                                          float* knn_sim, int32_t* pred, int32_t* correct, int32_t* pair_rank, double* scalars,
                                          void* ws, size_t ws_bytes, void* stream) {
  return emon_run("spcl_embed_monitor_grouped", z, ldz, labels, L, pair, group, N, d, k, exclude_pair, knn_idx, knn_sim, pred,
                  correct, pair_rank, scalars, ws, ws_bytes, stream);
}

extern "C" int spcl_cell_majority(const uint8_t* labels, int N, int H, int W, int C, int sh, int sw, int32_t* cell_label,
                                  float* purity, void* stream) {
  SPCL_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && H <= CMAJ_MAX_HW && W <= CMAJ_MAX_HW,
                 "spcl_cell_majority: N = %d (>= 1), H = %d, W = %d (1 .. %d)", N, H, W, CMAJ_MAX_HW);
  SPCL_CHECK_ARG(C >= 2 && C <= CMAJ_MAX_C, "spcl_cell_majority: C = %d classes (2 .. %d)", C, CMAJ_MAX_C);
  SPCL_CHECK_ARG(sh >= 1 && sh <= H && sw >= 1 && sw <= W, "spcl_cell_majority: grid %d x %d for maps of %d x %d", sh, sw, H, W);
  SPCL_CHECK_ARG((int64_t)N * sh * sw <= INT_MAX - 4, "spcl_cell_majority: %d x %d x %d cells (at most 2^31 - 5)", N, sh, sw);
  SPCL_CHECK_ARG(labels && cell_label, "spcl_cell_majority: null pointer");
  const int cells = N * sh * sw;
  SPCL_LAUNCH(cmaj_kernel, dim3(cdiv(cells, 4)), dim3(256), 0, (hipStream_t)stream, labels, cells, H, W, C, sh, sw, cell_label,
              purity);
  SPCL_LAUNCH_CHECK("spcl_cell_majority");
  return SPCL_OK;
}
