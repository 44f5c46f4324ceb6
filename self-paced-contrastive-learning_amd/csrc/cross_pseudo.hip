// Cross pseudo supervision (semi_seg/hooks/cps.py; Chen et al., CVPR 2021): two networks saw the same images, each is trained
// with cross-entropy towards the other's hard arg-max prediction.  Both directions in ONE launch.
//
//   spcl_cross_pseudo_ce: per pixel  pA = softmax(a), pB = softmax(b), yA / yB = argmax of the LOGITS (lowest class on a tie),
//                         confA = 1 / zA, confB = 1 / zB (the soft-max's largest numerator is exp(0) = 1: the confidence of
//                         pseudo_label.hip, the same helper, the same bits), keepA = confA >= tau[yA], keepB = confB >= tau[yB],
//                         term = keepB * -log pA[yB] + keepA * -log pB[yA].  loss = weight / M * sum term; da = keepB ? weight / M *
//                         (pA - onehot(yB)) : 0, db = keepA ? weight / M * (pB - onehot(yA)) : 0.  Each map is read once, each
//                         soft-max is formed once, both gradients are written.  Two pseudo_label_ce calls read both maps twice
//                         and form both soft-maxes twice.
//
// Laid out like pseudo_label.hip, on the pieces of pixel_criterion.hpp: a workgroup owns a slab of kSlab = 1024 pixels (thread
// t: pixels t, t + 256, t + 512, t + 768, added in that order; the xor butterfly of the wave; the four waves in order) and
// hands in a row of 2 doubles (the two directions) and 4 C + 1 integers (wave-uniform: popcount(ballot)).  The last workgroup to
// take its ticket cuts the rows into G = 256 / (4 C + 3) groups of consecutive rows, thread (group, column) adds its column over
// its group in row order, one thread per column adds the G group sums in group order.  One fixed association: the bits do not
// depend on scheduling.  No floating-point atomics and no memset: the workspace arrives zero-filled once, the close resets
// the ticket.
#include "common.hpp"
#include "pixel_criterion.hpp"

namespace {

constexpr int kSlab = 1024;  // pixels per workgroup (4 per thread)
constexpr int kND = 2;       // doubles per row: the term of a <- b, the term of b <- a
constexpr int kMaxC = 65;    // 4 C + 1 integers per row

struct cps_args {
  const float* a;
  const float* b;
  const float* tau;  // (NULL: every pixel is kept)
  double scale;      // weight / M
  float gs;          // (float)scale
  float* loss;
  float* parts;
  float* da;
  float* db;
  unsigned long long* hist;
  uint8_t* label_a;
  uint8_t* label_b;
  double* partial;  // [nblk][2]
  unsigned int* ticket;
  unsigned int* counts;  // [nblk][4 C + 1]
  long M;
  int C;
};

// (argmax_logits, cross_term: pixel_criterion.hpp, shared with cutmix.hip)

// CT = 4: C == 4 and the four maps 16-byte aligned (vector accesses); CT = 0: any C <= 16
template <int CT>
__global__ void __launch_bounds__(256) cross_pseudo_kernel(const cps_args a) {
  const int C = CT ? CT : a.C;
  const int NC = 4 * C + 1;
  __shared__ float s_tau[16];
  __shared__ double s_wd[4][kND];
  __shared__ unsigned int s_wc[4][kMaxC];
  __shared__ double s_gd[256];
  __shared__ unsigned long long s_gc[256];
  __shared__ double s_tot[kND];
  __shared__ unsigned int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // no thresholds: conf >= 0 keeps every pixel whose confidence is a number
  if (tid < 16) s_tau[tid] = (a.tau && tid < C) ? a.tau[tid] : 0.f;
  __syncthreads();

  double ta = 0.0, tb = 0.0;
  unsigned int na[16], nb[16], ka[16], kb[16], agree = 0u;  // (wave-uniform)
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
    bool keepA = false, keepB = false;
    if (pix < a.M) {
      float xa[16], xb[16];
      load_pixel<CT>(a.a + pix * C, C, xa);
      load_pixel<CT>(a.b + pix * C, C, xb);
      yA = argmax_logits(xa, C);
      yB = argmax_logits(xb, C);
      // the learner's logit at the other's label and its own largest logit, before the logits become numerators
      float a_yB = xa[0], b_yA = xb[0], mA = xa[0], mB = xb[0];
#pragma unroll
      for (int k = 1; k < 16; ++k)
        if (k < C) {
          mA = fmaxf(mA, xa[k]);
          mB = fmaxf(mB, xb[k]);
          if (k == yB) a_yB = xa[k];
          if (k == yA) b_yA = xb[k];
        }
      const float zA = softmax_numerators(xa, C), zB = softmax_numerators(xb, C);
      const float confA = 1.f / zA, confB = 1.f / zB;
      keepA = confA >= s_tau[yA];  // (a NaN confidence keeps nothing)
      keepB = confB >= s_tau[yB];
      ta += cross_term<CT>(xa, zA, mA, a_yB, yB, keepB, a.gs, C, a.da + pix * C);
      tb += cross_term<CT>(xb, zB, mB, b_yA, yA, keepA, a.gs, C, a.db + pix * C);
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
  // 2 + 4 C + 1 columns, added over the rows in one fixed association (rows_grouped_total); thread `column` holds its total
  double tot;
  unsigned long long n;
  rows_grouped_total(a.partial, a.counts, kND, NC, s_gd, s_gc, tot, n);
  if (tid < kND + NC) {
    if (tid < kND) {
      s_tot[tid] = tot;
      a.parts[tid] = (float)(tot * a.scale);
    } else {
      a.hist[tid - kND] = n;
    }
  }
  __syncthreads();
  if (tid == 0) {
    a.loss[0] = (float)((s_tot[0] + s_tot[1]) * a.scale);
    *a.ticket = 0u;
  }
}

inline size_t cps_nblk(long M) { return (size_t)((M + kSlab - 1) / kSlab); }

}  // namespace

// [partials: nblk x 2 doubles][ticket, 64 bytes][counts: nblk x (4 C + 1) unsigned ints], nblk = ceil(N H W / 1024)
extern "C" size_t spcl_cross_pseudo_workspace_bytes(int N, int C, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0 || C < 1 || C > 16) return 0;
  if ((long)N * H * W >= (1L << 31)) return 0;
  const size_t nblk = cps_nblk((long)N * H * W);
  return nblk * (size_t)kND * sizeof(double) + 64 + nblk * (size_t)(4 * C + 1) * sizeof(unsigned int);
}

extern "C" int spcl_cross_pseudo_ce(const float* a_logits, const float* b_logits, int N, int C, int H, int W, const float* tau,
                                    float weight, float* loss, float* parts, float* da, float* db, unsigned long long* hist,
                                    uint8_t* label_a, uint8_t* label_b, void* ws, size_t ws_bytes, void* stream) {
  SPCL_CHECK_ARG(a_logits && b_logits && loss && parts && da && db && hist && ws, "spcl_cross_pseudo_ce: null pointer");
  SPCL_CHECK_ARG(N > 0 && H > 0 && W > 0 && C >= 1 && C <= 16, "spcl_cross_pseudo_ce: bad shape (C <= 16)");
  SPCL_CHECK_ARG((long)N * H * W < (1L << 31), "spcl_cross_pseudo_ce: too many pixels");
  SPCL_CHECK_ARG(da != db, "spcl_cross_pseudo_ce: da and db are one buffer");
  const long M = (long)N * H * W;
  SPCL_CHECK_ARG(ws_bytes >= spcl_cross_pseudo_workspace_bytes(N, C, H, W), "spcl_cross_pseudo_ce: workspace too small");
  SPCL_CHECK_ARG((uintptr_t)ws % 8 == 0, "spcl_cross_pseudo_ce: workspace not 8-byte aligned");
  const size_t nblk = cps_nblk(M);
  hipStream_t st = (hipStream_t)stream;
  cps_args a{};
  a.a = a_logits;
  a.b = b_logits;
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
  a.C = C;
  // No memset of the ticket here: the caller hands in a workspace that was zero-filled before its first use, and the closing
  // workgroup leaves the ticket at zero.  A captured memset node was seen to write the low bits of its destination address
  // instead of its value from the second replay of a graph on, which a ticket does not survive.
  const bool vec = C == 4 && ((uintptr_t)a_logits | (uintptr_t)b_logits | (uintptr_t)da | (uintptr_t)db) % 16 == 0;
  spcl::prof_cost(4.0 * M * C * 4 + (label_a ? (double)M : 0.0) + (label_b ? (double)M : 0.0), 60.0 * M * C);
  if (vec) SPCL_LAUNCH(cross_pseudo_kernel<4>, dim3((unsigned)nblk), dim3(256), 0, st, a);
  else SPCL_LAUNCH(cross_pseudo_kernel<0>, dim3((unsigned)nblk), dim3(256), 0, st, a);
  SPCL_LAUNCH_CHECK("spcl_cross_pseudo_ce");
  return SPCL_OK;
}
