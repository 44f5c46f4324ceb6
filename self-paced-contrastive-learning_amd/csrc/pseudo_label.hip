// Self-training with confidence-thresholded pseudo-labels (semi_seg/hooks/pseudolabel.py): FixMatch's masked cross-entropy
// and FreeMatch's self-adaptive per-class thresholds (Wang et al., ICLR 2023, Algorithm 1) in ONE launch.
//
//   spcl_pseudo_label_ce: per pixel of the student's frame  q = softmax(flip(teacher)), y = argmax of the teacher's LOGITS
//                         (lowest class on a tie), conf = 1 / z (the soft-max's largest numerator is exp(0) = 1),
//                         keep = conf >= tau[y], term = keep ? -log softmax(student)_y : 0.  loss = weight / M * sum term,
//                         dstudent = keep ? weight / M * (p - onehot(y)) : 0.  Beside the loss the launch sums conf and q_c over
//                         ALL pixels (double), counts the pixels and the kept pixels of every class (integers) and, with a
//                         state, moves the thresholds: the closing workgroup computes FreeMatch's two moving averages and the
//                         next launch's tau in double.  Two maps read (the student's only where a pixel is kept), one written.
//
// The skeleton of pixel_criterion.hpp hands one double per 256 pixels to a close in which thread 0 adds them all; this
// kernel carries 2 + C doubles and 2 C integers, so it is laid out for the close instead:
//   - a workgroup owns a fixed slab of kSlab = 1024 pixels (thread t: pixels t, t + 256, t + 512, t + 768 of the slab, added
//     in that order; then the xor butterfly of the wave, then the four waves in order): 490 rows at 10 x 224 x 224 where the
//     skeleton has 1960;
//   - the per-class counts are wave-uniform: popcount(ballot(y == c)), no shared-memory traffic and no atomics;
//   - in the closing workgroup the rows are cut into G = 256 / (2 + 3 C) groups of consecutive rows; thread (group, statistic)
//     adds its column over its group in row order, with every load of the table in flight at once, then ONE THREAD PER
//     STATISTIC adds the G group sums in group order.
// Every sum has one fixed association: the bits do not depend on scheduling.  No floating-point atomics; the one memset is
// the ticket's.
#include "common.hpp"
#include "pixel_criterion.hpp"

// timing experiments only (tools/diag/pseudo_label_step_time.py --lib): a build with -DSPCL_PSEUDO_LABEL_CLOSE=0 skips the
// sums of the close (every output is then zero); the difference between the two builds is what the close costs
#ifndef SPCL_PSEUDO_LABEL_CLOSE
#define SPCL_PSEUDO_LABEL_CLOSE 1
#endif

namespace {

constexpr int kSlab = 1024;  // pixels per workgroup (4 per thread)
constexpr int kMaxD = 18;    // 2 + C doubles per row: term, conf, q_0 .. q_{C-1}
constexpr int kMaxC = 32;    // 2 C integers per row: pixels per class, kept pixels per class

struct pl_args {
  const float* teacher;
  const float* student;
  const uint8_t* flags;
  float* tau;
  double* state;
  double momentum;
  double scale;  // weight / M
  float gs;      // (float)scale
  float* loss;
  float* dstudent;
  double* stats;
  unsigned long long* hist;
  uint8_t* label;
  double* partial;       // [nblk][2 + C]
  unsigned int* ticket;
  unsigned int* counts;  // [nblk][2 C]
  long M;
  int C, H, W;
};

__device__ __forceinline__ double wave_sum_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// CT = 4: C == 4 and the three maps 16-byte aligned (vector accesses); CT = 0: any C <= 16
template <int CT>
__global__ void __launch_bounds__(256) pseudo_label_kernel(const pl_args a) {
  const int C = CT ? CT : a.C;
  const int ND = C + 2, NC = 2 * C;
  __shared__ float s_tau[16];
  __shared__ double s_wd[4][kMaxD];
  __shared__ unsigned int s_wc[4][kMaxC];
  __shared__ double s_gd[256];
  __shared__ unsigned long long s_gc[256];
  __shared__ double s_tot[kMaxD];
  __shared__ unsigned int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the thresholds of THIS launch: read before anything else, long before the workgroup's ticket
  if (tid < C) s_tau[tid] = a.tau[tid];
  __syncthreads();

  double aterm = 0.0, aconf = 0.0, aq[16];
  unsigned int ca[16], ck[16];  // (wave-uniform)
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    aq[k] = 0.0;
    ca[k] = 0u;
    ck[k] = 0u;
  }
  const long base = (long)blockIdx.x * kSlab;
#pragma clang loop unroll_count(CT == 4 ? 4 : 1)
  for (int i = 0; i < kSlab / 256; ++i) {
    const long pix = base + i * 256 + tid;
    int y = -1;
    bool keep = false;
    if (pix < a.M) {
      float q[16];
      load_pixel<CT>(a.teacher + flipped_pixel(pix, a.H, a.W, a.flags) * C, C, q);
      y = 0;
      float best = q[0];
#pragma unroll
      for (int k = 1; k < 16; ++k)
        if (k < C && q[k] > best) {  // (strictly greater: a tie stays with the lower class)
          best = q[k];
          y = k;
        }
      const float z = softmax_numerators(q, C);
      const float conf = 1.f / z;
      aconf += (double)conf;
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < C) aq[k] += (double)(q[k] / z);
      keep = conf >= s_tau[y];  // (a NaN confidence keeps nothing)
      float g[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) g[k] = 0.f;
      if (keep) {
        float p[16];
        load_pixel<CT>(a.student + pix * C, C, p);
        float xy = p[0], m = p[0];
#pragma unroll
        for (int k = 1; k < 16; ++k)
          if (k < C) {
            m = fmaxf(m, p[k]);
            if (k == y) xy = p[k];
          }
        const float zs = softmax_numerators(p, C);
        aterm += (double)(logf(zs) - (xy - m));  // -log p_y, with no quotient that could underflow
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (k < C) g[k] = a.gs * (p[k] / zs - (k == y ? 1.f : 0.f));
      }
      store_pixel<CT>(a.dstudent + pix * C, C, g);  // exact zeros where the pixel is dropped
      if (a.label) a.label[pix] = keep ? (uint8_t)y : (uint8_t)255;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < C) {
        ca[k] += (unsigned int)__popcll(__ballot(y == k));
        ck[k] += (unsigned int)__popcll(__ballot(keep && y == k));
      }
  }

  // wave -> workgroup: the butterfly gives every lane the wave's sum; lane 0 files it, one thread per statistic adds the waves
  aterm = wave_sum_d(aterm);
  aconf = wave_sum_d(aconf);
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (k < C) aq[k] = wave_sum_d(aq[k]);
  if (lane == 0) {
    s_wd[wave][0] = aterm;
    s_wd[wave][1] = aconf;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < C) {
        s_wd[wave][2 + k] = aq[k];
        s_wc[wave][k] = ca[k];
        s_wc[wave][C + k] = ck[k];
      }
  }
  __syncthreads();
  if (tid < ND) {
    a.partial[(size_t)blockIdx.x * ND + tid] = ((s_wd[0][tid] + s_wd[1][tid]) + s_wd[2][tid]) + s_wd[3][tid];
  } else if (tid >= 64 && tid < 64 + NC) {
    const int j = tid - 64;
    a.counts[(size_t)blockIdx.x * NC + j] = s_wc[0][j] + s_wc[1][j] + s_wc[2][j] + s_wc[3][j];
  }
  // publish the row, then take a ticket: every storing wave drains its stores, one thread releases at device scope.  The
  // fence also stands between this workgroup's reads of tau (above) and its ticket.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = atomicAdd(a.ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;  // (uniform over the workgroup)

  // ------------------------------------------------------------------------------------------------------------ the close
  // ncol = 2 + C + 2 C statistics, G = 256 / ncol groups of R = ceil(nblk / G) consecutive rows: thread (group, column) adds
  // its column over its group's rows in row order -- all of a thread's loads are independent, the whole table is in flight at
  // once instead of one staged round after the other --, then one thread per column adds the G group sums in group order.
  // G and R follow from the grid and C alone: one fixed association.
  __threadfence();
  const int nblk = (int)gridDim.x;
  const int ncol = ND + NC, G = 256 / ncol, R = (nblk + G - 1) / G;
  const int col = tid % ncol, grp = tid / ncol;
  double tot = 0.0;
  unsigned long long n = 0ull;
  if (SPCL_PSEUDO_LABEL_CLOSE && grp < G) {
    const int r0 = grp * R, r1 = r0 + R < nblk ? r0 + R : nblk;
    if (col < ND) {
      const volatile double* src = (const volatile double*)a.partial + col;
#pragma unroll 8
      for (int r = r0; r < r1; ++r) tot += src[(size_t)r * ND];
    } else {
      const volatile unsigned int* src = (const volatile unsigned int*)a.counts + (col - ND);
#pragma unroll 8
      for (int r = r0; r < r1; ++r) n += src[(size_t)r * NC];
    }
  }
  s_gd[tid] = tot;
  s_gc[tid] = n;
  __syncthreads();
  if (tid < ncol) {
    tot = 0.0;
    n = 0ull;
    for (int g = 0; g < G; ++g) {
      tot += s_gd[g * ncol + tid];
      n += s_gc[g * ncol + tid];
    }
    if (tid < ND) {
      s_tot[tid] = tot;
      if (tid >= 1) a.stats[tid - 1] = tot;
    } else {
      a.hist[tid - ND] = n;
    }
  }
  __syncthreads();
  if (tid == 0) {
    a.loss[0] = (float)(s_tot[0] * a.scale);
    if (a.state) {
      // The in-place store races with nothing: every workgroup copied tau to its shared memory before it took its ticket,
      // this workgroup holds the LAST ticket, so no read of tau (or of state, which only this thread ever touches) by this
      // launch is still to come; the next launch on the stream starts after this one has ended.
      const double mo = a.momentum, om = 1.0 - mo, Md = (double)a.M;
      const double tg = mo * a.state[0] + om * (s_tot[1] / Md);
      a.state[0] = tg;
      double mx = 0.0;
      for (int c = 0; c < C; ++c) {
        const double pt = mo * a.state[1 + c] + om * (s_tot[2 + c] / Md);
        a.state[1 + c] = pt;
        mx = fmax(mx, pt);
      }
      for (int c = 0; c < C; ++c) a.tau[c] = (float)(a.state[1 + c] / mx * tg);
    }
    *a.ticket = 0u;
  }
}

inline size_t pl_nblk(long M) { return (size_t)((M + kSlab - 1) / kSlab); }

}  // namespace

// [partials: nblk x (2 + C) doubles][ticket, 64 bytes][counts: nblk x 2 C unsigned ints], nblk = ceil(N H W / 1024)
extern "C" size_t spcl_pseudo_label_workspace_bytes(int N, int C, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0 || C < 1 || C > 16) return 0;
  const size_t nblk = pl_nblk((long)N * H * W);
  return nblk * (size_t)(C + 2) * sizeof(double) + 64 + nblk * (size_t)(2 * C) * sizeof(unsigned int);
}

extern "C" int spcl_pseudo_label_ce(const float* teacher, const float* student_logits, int N, int C, int H, int W,
                                    const uint8_t* flags_teacher, float* tau, double* state, double momentum, float weight,
                                    float* loss, float* dstudent, double* stats, unsigned long long* hist, uint8_t* label, void* ws,
                                    size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(teacher && student_logits && tau && loss && dstudent && stats && hist && ws,
                 "spcl_pseudo_label_ce: null pointer");
  SPCL_CHECK_ARG(N > 0 && H > 0 && W > 0 && C >= 1 && C <= 16, "spcl_pseudo_label_ce: bad shape (C <= 16)");
  SPCL_CHECK_ARG((long)N * H * W < (1L << 31), "spcl_pseudo_label_ce: too many pixels");
  SPCL_CHECK_ARG(!state || (momentum >= 0.0 && momentum < 1.0), "spcl_pseudo_label_ce: momentum %g outside [0, 1)", momentum);
  const long M = (long)N * H * W;
  SPCL_CHECK_ARG(ws_bytes >= spcl_pseudo_label_workspace_bytes(N, C, H, W), "spcl_pseudo_label_ce: workspace too small");
  SPCL_CHECK_ARG((uintptr_t)ws % 8 == 0, "spcl_pseudo_label_ce: workspace not 8-byte aligned");
  const size_t nblk = pl_nblk(M);
  hipStream_t st = (hipStream_t)stream;
  pl_args a{};
  a.teacher = teacher;
  a.student = student_logits;
  a.flags = flags_teacher;
  a.tau = tau;
  a.state = state;
  a.momentum = momentum;
  a.scale = (double)weight / (double)M;
  a.gs = (float)a.scale;
  a.loss = loss;
  a.dstudent = dstudent;
  a.stats = stats;
  a.hist = hist;
  a.label = label;
  a.partial = (double*)ws;
  a.ticket = (unsigned int*)((char*)ws + nblk * (size_t)(C + 2) * sizeof(double));
  a.counts = (unsigned int*)((char*)a.ticket + 64);
  a.M = M;
  a.C = C;
  a.H = H;
  a.W = W;
  if (hipMemsetAsync(a.ticket, 0, sizeof(unsigned int), st) != hipSuccess) {
    spcl::set_error("spcl_pseudo_label_ce: memset failed");
    return SPCL_ELAUNCH;
  }
  const bool vec = C == 4 && ((uintptr_t)teacher | (uintptr_t)student_logits | (uintptr_t)dstudent) % 16 == 0;
  spcl::prof_cost(3.0 * M * C * 4 + (label ? (double)M : 0.0), 30.0 * M * C);
  if (vec) SPCL_LAUNCH(pseudo_label_kernel<4>, dim3((unsigned)nblk), dim3(256), 0, st, a);
  else SPCL_LAUNCH(pseudo_label_kernel<0>, dim3((unsigned)nblk), dim3(256), 0, st, a);
  SPCL_LAUNCH_CHECK("spcl_pseudo_label_ce");
  return SPCL_OK;
}
