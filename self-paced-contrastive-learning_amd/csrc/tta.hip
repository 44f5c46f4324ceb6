// Test-time augmentation for inference: the merge of V views' class maps in one launch (spcl_tta_merge).
//
// The V views of a batch are its mirrored / transposed copies (functional.tta_views); the network's logits for view j lie in
// that view's frame.  Per pixel of the ORIGINAL frame the kernel reads each view's logits once, through the view's index
// map (op byte: bit 0 the input was flipped along H, bit 1 along W, bit 2 its H and W axes were swapped after the flips) --
// no un-flipped or transposed copy is written --, forms each view's softmax, adds the V probability rows pairwise in a fixed
// balanced tree over the view index, multiplies by the exact 1 / V and writes the mean probability, its first maximal class
// and the normalised entropy -sum_c p_c log(p_c + eps) / log(C) (the uncertainty of comparable.py:94-98, here of the averaged
// prediction).  The mean of the entropy map rides in the same launch on the skeleton of pixel_criterion.hpp (per-workgroup
// double partials, added in index order by the last workgroup, which resets the ticket): bitwise reproducible.
//
// Why a tree: V equal rows p give 2p, 4p, 8p (exact) and p again after the multiplication by 1 / V, so V exactly flipped /
// transposed copies of one map merge to the bits of that map alone; a running sum would round at 3p.
//
// One thread per pixel; V and the channel access (CT = 4: C == 4 and every pointer 16-byte aligned, one 16-byte access per
// row; CT = 0: any 2 <= C <= 16, 4-byte accesses) are template parameters, so the tree is straight-line code and the view
// pointers are read from the kernel's argument block at constant offsets.  With bit 2 neighbouring lanes read one column of
// the view (stride W C floats); nothing is staged through LDS (measured, tools/diag/tta_time.py).
#include "common.hpp"
#include "pixel_criterion.hpp"

namespace {

// the V view maps and their op bytes, by value in the kernel's argument block (as ucmt_noisy)
struct tta_views {
  const float* p[8];
  uint8_t op[8];
};

template <int CT, int V>
struct tta_merge_px {
  static constexpr bool kCounts = false;
  tta_views vw;
  int C, H, W;
  float eps;
  float* prob;
  int64_t* pred;
  float* entropy;

  // out <- the sum of softmax(view j at its image of (n, u, v)) over j in [LO, LO + CNT): (left half) + (right half)
  template <int LO, int CNT>
  __device__ __forceinline__ void rows(int n, int u, int v, int CC, float (&out)[16]) const {
    if constexpr (CNT == 1) {
      const unsigned op = vw.op[LO];
      const int uu = flip_idx(u, H, op & 1), vv = flip_idx(v, W, op & 2);
      // (bit 2: H == W, checked on the host, so row vv < W = H and column uu < H = W stay inside the map)
      const long src = (op & 4) ? ((long)n * H + vv) * W + uu : ((long)n * H + uu) * W + vv;
      load_pixel<CT>(vw.p[LO] + src * CC, CC, out);
      const float z = softmax_numerators(out, CC);
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < CC) out[k] = out[k] / z;
    } else {
      float right[16];
      rows<LO, CNT / 2>(n, u, v, CC, out);
      rows<LO + CNT / 2, CNT / 2>(n, u, v, CC, right);
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < CC) out[k] += right[k];
    }
  }

  __device__ double operator()(long pix, bool&) const {
    const int CC = CT ? CT : C;
    const int n = (int)(pix / ((long)H * W));
    const int rem = (int)(pix - (long)n * H * W), u = rem / W, v = rem - u * W;
    float p[16];
    rows<0, V>(n, u, v, CC, p);
    constexpr float inv = 1.f / (float)V;  // a power of two: the product is exact
    float e = 0.f, m = -INFINITY;
    int best = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < CC) {
        p[k] *= inv;
        e = fmaf(p[k], logf(p[k] + eps), e);
        if (k == 0 || p[k] > m) {  // the first maximum, as spcl_argmax_classes
          m = p[k];
          best = k;
        }
      }
    store_pixel<CT>(prob + pix * CC, CC, p);
    pred[pix] = best;
    const float ent = -e / logf((float)CC);
    if (entropy) entropy[pix] = ent;
    return (double)ent;
  }
};

template <int CT, int V>
int launch_tta(const tta_views& vw, int C, int H, int W, float eps, float* prob, int64_t* pred, float* entropy,
               const pixel_launch& p, float* mean_entropy) {
  return launch_pixel_criterion("spcl_tta_merge", tta_merge_px<CT, V>{vw, C, H, W, eps, prob, pred, entropy}, p,
                                1.0 / (double)p.M, mean_entropy);
}

template <int CT>
int launch_tta_v(int V, const tta_views& vw, int C, int H, int W, float eps, float* prob, int64_t* pred, float* entropy,
                 const pixel_launch& p, float* mean_entropy) {
  switch (V) {
    case 1: return launch_tta<CT, 1>(vw, C, H, W, eps, prob, pred, entropy, p, mean_entropy);
    case 2: return launch_tta<CT, 2>(vw, C, H, W, eps, prob, pred, entropy, p, mean_entropy);
    case 4: return launch_tta<CT, 4>(vw, C, H, W, eps, prob, pred, entropy, p, mean_entropy);
    default: return launch_tta<CT, 8>(vw, C, H, W, eps, prob, pred, entropy, p, mean_entropy);
  }
}

}  // namespace

extern "C" size_t spcl_tta_merge_workspace_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return pixel_workspace_bytes((long)N * H * W);
}

extern "C" int spcl_tta_merge(const float* const* views, const uint8_t* ops, int V, int N, int C, int H, int W, float eps,
                              float* prob, int64_t* pred, float* entropy, float* mean_entropy, void* ws, size_t ws_bytes,
                              void* stream) {
  SPCL_CHECK_ARG(V == 1 || V == 2 || V == 4 || V == 8, "spcl_tta_merge: V = %d views (1, 2, 4 or 8)", V);
  SPCL_CHECK_ARG(views && ops && prob && pred && mean_entropy && ws, "spcl_tta_merge: null pointer");
  SPCL_CHECK_ARG(N > 0 && H > 0 && W > 0, "spcl_tta_merge: bad shape (N = %d, H = %d, W = %d)", N, H, W);
  SPCL_CHECK_ARG(C >= 2 && C <= 16, "spcl_tta_merge: C = %d classes (2 <= C <= 16)", C);
  SPCL_CHECK_ARG(eps >= 0.f, "spcl_tta_merge: negative eps");
  SPCL_CHECK_ARG((uintptr_t)prob % 4 == 0 && (uintptr_t)pred % 8 == 0 && (uintptr_t)entropy % 4 == 0 &&
                     (uintptr_t)mean_entropy % 4 == 0 && (uintptr_t)ws % 8 == 0,
                 "spcl_tta_merge: misaligned output or workspace");
  const uintptr_t bytes = (uintptr_t)N * H * W * C * sizeof(float), lo = (uintptr_t)prob, hi = lo + bytes;
  tta_views vw{};
  bool vec = C == 4 && (uintptr_t)prob % 16 == 0;
  for (int j = 0; j < V; ++j) {
    SPCL_CHECK_ARG(views[j], "spcl_tta_merge: null pointer (view %d)", j);
    SPCL_CHECK_ARG((uintptr_t)views[j] % 4 == 0, "spcl_tta_merge: view %d is not 4-byte aligned", j);
    SPCL_CHECK_ARG(ops[j] < 8, "spcl_tta_merge: op %d of view %d (bit 0 flip H, bit 1 flip W, bit 2 swap; < 8)", (int)ops[j], j);
    SPCL_CHECK_ARG(!(ops[j] & 4) || H == W, "spcl_tta_merge: view %d swaps its axes (op %d), which needs H == W, given %d x %d",
                   j, (int)ops[j], H, W);
    // a pixel of prob is written while other pixels of the views are still to be read
    SPCL_CHECK_ARG((uintptr_t)views[j] + bytes <= lo || (uintptr_t)views[j] >= hi, "spcl_tta_merge: prob overlaps view %d", j);
    vw.p[j] = views[j];
    vw.op[j] = ops[j];
    vec = vec && (uintptr_t)views[j] % 16 == 0;
  }
  pixel_launch p;
  if (int rc = pixel_prepare("spcl_tta_merge", "2 <= C <= 16", N, C, H, W, ws, ws_bytes, false, stream, &p)) return rc;
  spcl::prof_cost((double)(V + 1) * p.M * C * 4 + (entropy ? 12.0 : 8.0) * p.M, (20.0 * V + 25.0) * p.M * C);
  if (vec) return launch_tta_v<4>(V, vw, C, H, W, eps, prob, pred, entropy, p, mean_entropy);
  return launch_tta_v<0>(V, vw, C, H, W, eps, prob, pred, entropy, p, mean_entropy);
}
