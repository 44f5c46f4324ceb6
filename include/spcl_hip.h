/* spcl_hip.h -- C ABI of libspcl_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * self-paced contrastive pre-train hot path.
 *
 * The reference (jizongFox/Self-paced-Contrastive-Learning) has NO FFI: its seam is four Python classes
 * dispatching stock ATen ops.  Each entry point below replaces the ATen op sequence of one reference
 * call site (cited per function as  path:line  relative to the reference root).  The Python mirror of the
 * reference classes (self-paced-contrastive-learning_amd/{contrastyou,semi_seg}) binds these through ctypes;
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error (spcl_last_error() gives the text); nothing throws
 *  - all data pointers are DEVICE pointers owned by the caller and only borrowed for the call
 *  - work is enqueued on the caller's stream (hipStream_t passed as void*); no host sync, no allocation,
 *    no internal threads -> every call is hipGraph-capturable
 *  - activations are NHWC ("channels last"), channel count padded to a multiple of 16 (pad lanes hold 0)
 *  - dtype: SPCL_F32 = 0 (f32 storage: the parity mode; convolution products are f32-grade split-bf16 by default, exact-f32
 *    MFMA on request -- spcl_conv_set_f32_split below), SPCL_BF16 = 1 (bf16 storage, f32 accumulate)
 *  - the library reads NOTHING from the environment: every switch is an argument or a setter declared here
 */
#ifndef SPCL_HIP_H
#define SPCL_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SPCL_F32 0
#define SPCL_BF16 1

#define SPCL_OK 0
#define SPCL_EINVAL (-1)
#define SPCL_ELAUNCH (-2)
#define SPCL_EUNSUPPORTED (-3)

/* Bumped whenever a struct layout, a limit (SPCL_*_MAX) or an entry point's meaning changes.  The library is git-ignored and
 * travels next to the sources: the Python binding (native.py) refuses a library whose version is not the header's, so that a
 * stale build fails at load time instead of running kernels on structs of another stride. */
#define SPCL_ABI_VERSION 37
int spcl_abi_version(void);
const char* spcl_last_error(void);

/* ---------------------------------------------------------------- contrastive loss -----------------------
 * Replaces contrastyou/losses/contrast_loss3.py:25-31 (exp_sim_temperature), :41-110 (SupConLoss1._forward),
 * :126-214 (SelfPacedSupConLoss._forward/_self_paced_mask) and the autograd backward of those (K11-K17).
 *
 * z1,z2   [n,d] f32 row-major (unit rows);  labels [n] f32 or NULL;  mask [n,n] f32 or NULL
 *         (labels==NULL && mask==NULL -> SimCLR identity positives, contrast_loss3.py:140-143)
 * sp_mode 0 = no self-pacing (SupConLoss1), 1 = hard, 2 = soft;  gamma = age parameter
 * ws      workspace of spcl_supcon_workspace_bytes(n,d) bytes (f32 aligned); holds the padded projections,
 *         the per-row statistics kept for backward and the column-split partials
 * Three schedules, chosen by size alone (same results within the parity tolerance, same workspace contract):
 *   2n <= 64 (the training sizes): one workgroup, one launch -- forward scalars, row statistics and dLoss/dP for a unit
 *     upstream gradient (kept in ws; spcl_supcon_backward then is one scaling launch); exact-f32 MFMA, same k order as the
 *     sweeps;
 *   64 < 2n < 1024, or an explicit `mask`: the [2n,2n] matrix is never materialised; every sweep recomputes its S tiles on the
 *     exact-f32 MFMA (bitwise an fmaf chain) -- the training sizes are launch-latency bound either way;
 *   2n >= 1024 (labels / SimCLR modes, d <= 128, 2n a multiple of 256): the forward is FUSED -- two sweeps over the
 *     similarity tiles (row sums first, then the weights that depend on them), each recomputing S on the bf16 matrix pipe from
 *     the two-term split P = Ph + Pm (S ~ Ph Ph^T + Ph Pm^T + Pm Ph^T, logit error ~1e-5); no logits matrix is written or
 *     read (SURVEY 8(d) prices this size against the materialised schedule's 205.5 MB; the fused forward's own HBM traffic is
 *     a few MB).  The backward forms H = G + G^T tile by tile the same way.  Other large shapes (d > 128, ragged 2n) keep
 *     the round-1 schedule: logits written once to ws as f32 [2n,2n], streamed by the later passes.
 * out     [8] f32: out[0]=loss out[1]=rho(downgrade ratio) out[2]=kappa(effective -dloss/drow scale)
 *                  out[3]=max|‖z‖-1| (is_normalized contract, contrast_loss3.py:20-22,154)
 */
size_t spcl_supcon_workspace_bytes(int n, int d);
int spcl_supcon_forward(const float* z1, const float* z2, const float* labels, const float* mask, int n, int d,
                        float temperature, int sp_mode, float gamma, int correct_grad, float* ws, float* out,
                        void* stream);
/* dz1,dz2 [n,d] f32 = grad_out[0] * dLoss/dz ; uses the row statistics left in ws by the forward call */
int spcl_supcon_backward(const float* labels, const float* mask, int n, int d, float temperature, int sp_mode,
                         float gamma, const float* ws_fwd, float* ws_bwd, const float* out_fwd,
                         const float* grad_out, float* dz1, float* dz2, void* stream);
size_t spcl_supcon_bwd_workspace_bytes(int n, int d);
/* 1 (and the block's offset in the FORWARD workspace, in floats, and its row pitch) when spcl_supcon_forward leaves dLoss/dP
 * for a unit upstream gradient there (the training sizes, 2n <= 64): rows [0, 2n) x [0, d) of it ARE the gradient when the
 * upstream gradient is exactly 1 -- spcl_supcon_backward would only multiply them by it.  0: this shape recomputes. */
int spcl_supcon_unit_gradient_block(int n, int d, size_t* offset_floats, int* row_pitch);
/* K (1..4) losses of ONE shape in the launches of one -- the K meta-label hooks that semi_seg/hooks/creator.py:102-124
 * puts on one feature, each with its own label vector and its own self-paced age parameter (hooks/infonce.py:133-141).
 * Head h reads z1 + h z_stride and z2 + h z_stride ([n,d] f32 each), labels + h n (NULL: SimCLR for every head), uses
 * gammas[h] (host array, read during the call), owns ws + h ws_stride floats (>= spcl_supcon_workspace_bytes(n,d) / 4)
 * and writes out + 8 h.  Same arithmetic, per head, as spcl_supcon_forward / _backward (bit-identical results).  Only the
 * training-size schedules (2n below the large-batch threshold; SPCL_EUNSUPPORTED otherwise) and no explicit mask.
 * backward: grad_out[K] (device), dz1 / dz2 + h z_stride, ws_bwd + h wsb_stride floats. */
int spcl_supcon_forward_heads(int K, const float* z1, const float* z2, size_t z_stride, const float* labels, int n,
                              int d, float temperature, int sp_mode, const float* gammas, int correct_grad, float* ws,
                              size_t ws_stride, float* out, void* stream);
/* The projector's F.normalize (contrastyou/projectors/heads.py:15-17, nn.py:29-36) and its backward inside the loss launch:
 * o1 / o2 are the K heads' rows BEFORE normalisation; the launch normalises them (z = o / max(||o||, 1e-12): the rows it
 * leaves in the workspace for the taps are the normalised ones, bit for bit those of spcl_l2norm_rows_forward), evaluates
 * the loss exactly as spcl_supcon_forward_heads does on them, and the unit-gradient block (spcl_supcon_unit_gradient_block;
 * spcl_supcon_backward(_heads) scales it) holds d loss / d o.  Training sizes only: spcl_supcon_rows_supported(n, d) != 0
 * (2n <= 64, d <= 256: the one-workgroup schedule); labels [K][n] or NULL, no explicit mask.  K = 1: strides unused. */
int spcl_supcon_rows_supported(int n, int d);
int spcl_supcon_forward_rows(int K, const float* o1, const float* o2, size_t o_stride, const float* labels, int n, int d,
                             float temperature, int sp_mode, const float* gammas, int correct_grad, float* ws,
                             size_t ws_stride, float* out, void* stream);
int spcl_supcon_backward_heads(int K, const float* labels, int n, int d, float temperature, int sp_mode,
                               const float* gammas, const float* ws_fwd, size_t ws_stride, float* ws_bwd,
                               size_t wsb_stride, const float* out_fwd, const float* grad_out, float* dz1, float* dz2,
                               size_t z_stride, void* stream);
/* lazily materialise the [2n,2n] hook taps (contrast_loss3.py:175-178,188): any pointer may be NULL */
int spcl_supcon_materialize(const float* labels, const float* mask, int n, int d, float temperature, int sp_mode,
                            float gamma, const float* ws_fwd, float* sim_logits, float* sim_exp, float* pos_mask,
                            float* neg_mask, float* sp_mask, void* stream);

/* SupConLoss1(exclude_other_pos=True) (contrast_loss3.py:97-100: every positive pair is scored against the row's
 * negatives only, their sum divided by the row's negative ratio + 1e-4) and its gradient; not used by the hooks, plain
 * fp32 row kernels.  labels / mask as above (both NULL = SimCLR); ws of spcl_supcon_xpos_workspace_bytes(n, d) (0 when
 * n > 4096) keeps d loss / d logits for the backward; out[0] = loss, out[3] = max | |row| - 1 |. */
size_t spcl_supcon_xpos_workspace_bytes(int n, int d);
int spcl_supcon_xpos_forward(const float* z1, const float* z2, const float* labels, const float* mask, int n, int d,
                             float temperature, float* ws, float* out, void* stream);
int spcl_supcon_xpos_backward(const float* z1, const float* z2, int n, int d, float temperature, const float* ws,
                              const float* grad_out, float* dz1, float* dz2, void* stream);

/* Weighted supervised-contrastive losses (csrc/supcon_weighted.hip): replaces contrastyou/losses/contrast_loss.py:49-104
 * (SupConLoss2, in / out mode), :144-181 (SupConLoss3, real-valued pos_weight) and :220-270 (SupConLoss4, block weights)
 * and the autograd backward of those.  Over the 2n rows of cat(z1, z2), s_ij = z_i . z_j / t, pair weights P_ij >= 0 and
 * a 0/1 denominator switch E_ij (both 0 on the diagonal):  D_i = sum_j E_ij exp(s_ij), W_i = sum_j P_ij,
 *   in_mode == 0:  loss = -mean_i [ sum_j P_ij (s_ij - log D_i) / W_i ]
 *   in_mode != 0:  loss = -mean_i [ log( sum_j P_ij exp(s_ij) / D_i ) / W_i ]
 * P and E are read by index (u = i mod n, v = j mod n), never built as [2n,2n] matrices:
 *   labels [n] f32 (blocks must be 0):  P = [labels_u == labels_v], E = 1  (contrast_loss.py:68-75; SimCLR, :76-80, is the
 *     label vector 0 .. n-1)
 *   labels NULL: bit 0 = w11 is block (1,1), bit 1 = w22 is block (2,2), bit 2 = w12 is BOTH blocks (1,2) and (2,1), not
 *     transposed (:233-237); [n,n] f32 each, not assumed symmetric.  On a present block E = 1 and P = its entry w; on an
 *     absent block P = E = 0.  mask_semantics != 0 reads w as P = [w == 1], E = [w == 0 or w == 1] (:62-66).
 *     SupConLoss3's pos_weight.repeat(2, 2) (:152) is the same matrix in all three slots, blocks == 7.
 * z1, z2 [n,d] f32 unit rows; n <= 4096, d <= 4096 (spcl_supcon_weighted_workspace_bytes returns 0 beyond).
 * ws: workspace of that many bytes.  For 2n <= 64 and d <= 256 (one workgroup, one launch, exact-f32 MFMA) its first 2n*d
 * floats are dLoss/dz (rows of z1, then of z2; pitch d) for a unit upstream gradient after the forward call, and the backward
 * call is one scaling launch; above that S is formed in 64 x 64 tiles on the same MFMA, row kernels take the statistics, and
 * dLoss/dS stays there ([2n,2n]) for the backward call's tiles.
 * out [8] f32: out[0] = loss (NaN when a row has W_i = 0 in out mode, as the reference's arithmetic: it raises, :102-103,
 * 179-180,268-269), out[1] = 1, out[2] = 1/2n, out[3] = max | |row| - 1 | (is_normalized, :20-22).  Sums in a fixed order. */
size_t spcl_supcon_weighted_workspace_bytes(int n, int d);
int spcl_supcon_weighted_forward(const float* z1, const float* z2, const float* labels, const float* w11,
                                 const float* w22, const float* w12, int blocks, int mask_semantics, int in_mode, int n,
                                 int d, float temperature, float* ws, float* out, void* stream);
/* dz1, dz2 [n,d] f32 = grad_out[0] * dLoss/dz, from what the forward call left in ws (same z1, z2, n, d, temperature);
 * above the one-workgroup sizes it writes its partial sums into a part of ws the forward call left free */
int spcl_supcon_weighted_backward(const float* z1, const float* z2, int n, int d, float temperature, float* ws,
                                  const float* grad_out, float* dz1, float* dz2, void* stream);
/* the [2n,2n] hook taps as the reference stores them, BEFORE the diagonal is removed (contrast_loss.py:83-86,159-161,
 * 247-250): sim_logits = S/t - max(S/t), sim_exp = exp(sim_logits), pos_weight = P, enable_mask = E (SupConLoss2's
 * neg_mask is E - P).  Any of the four may be NULL.  Uses the last 2n floats of ws as scratch, nothing else of it. */
int spcl_supcon_weighted_materialize(const float* z1, const float* z2, const float* labels, const float* w11,
                                     const float* w22, const float* w12, int blocks, int mask_semantics, int n, int d,
                                     float temperature, float* ws, float* sim_logits, float* sim_exp, float* pos_weight,
                                     float* enable_mask, void* stream);

/* ---------------------------------------------------------------- projector ------------------------------
 * Replaces contrastyou/projectors/heads.py:9-25,78-92 + nn.py:8-15,29-36,56-58:
 * AdaptiveAvgPool2d((1,1)) -> Flatten -> Linear -> LeakyReLU(0.01) -> Linear -> F.normalize(p=2,dim=1).
 * feat [N,H,W,Cs] NHWC (dtype), first C of Cs channels used; w1 [hid,C] b1 [hid] w2 [out,hid] b2 [out] f32
 * (hid == 0 -> "linear" head: w1 is [out,C], w2/b2 ignored).  Saved for backward: pooled [N,C], pre [N,hid],
 * o [N,out] (un-normalised), all f32.  z [N,out] f32.
 * feat == NULL (spcl_proj_forward, spcl_proj_heads_forward): `pooled` is an INPUT -- the rows the producer of the feature
 * map left beside it (spcl_bnrelu_gap_forward) -- and no pooling launch runs; normalize == 0 with z == o: no copy.
 */
int spcl_proj_forward(const void* feat, int dtype, int N, int HW, int C, int Cs, const float* w1, const float* b1,
                      const float* w2, const float* b2, int hid, int out_dim, int normalize, float* pooled,
                      float* pre, float* o, float* z, void* stream);
/* dz [N,out] -> dw1,db1,dw2,db2 (f32, overwritten) and dfeat [N,H,W,Cs] (dtype, overwritten; NULL to skip) */
int spcl_proj_backward(const float* dz, int dtype, int N, int HW, int C, int Cs, const float* w1, const float* w2,
                       int hid, int out_dim, int normalize, const float* pooled, const float* pre, const float* o,
                       float* dw1, float* db1, float* dw2, float* db2, float* scratch /* [N,hid]+[N,out]+[N,C] f32 */,
                       void* dfeat, void* stream);

/* K <= 4 heads of IDENTICAL shape on the SAME feature -- several meta-label hooks on one encoder tap (hooks/creator.py:
 * 102-124 builds one INFONCEHook per contrast_on, each with its own ProjectionHead; semi_seg/hooks/infonce.py:224-231
 * projects the same tensor in each): the feature is average-pooled once and every layer of all K heads is ONE launch
 * (blockIdx.z = head); the backward sums the K input gradients in head order and broadcasts once.  The pointer
 * arguments marked [] are HOST arrays of K device pointers; the rest as spcl_proj_forward / spcl_proj_backward.
 * scratch: K * N * (out_dim + hid) + N * C floats. */
int spcl_proj_heads_forward(int K, const void* feat, int dtype, int N, int HW, int C, int Cs, const float* const* w1 /*[]*/,
                            const float* const* b1 /*[]*/, const float* const* w2 /*[]*/, const float* const* b2 /*[]*/,
                            int hid, int out_dim, int normalize, float* pooled, float* const* pre /*[]*/,
                            float* const* o /*[]*/, float* const* z /*[]*/, void* stream);
int spcl_proj_heads_backward(int K, const float* const* dz /*[]*/, int dtype, int N, int HW, int C, int Cs,
                             const float* const* w1 /*[]*/, const float* const* w2 /*[]*/, int hid, int out_dim,
                             int normalize, const float* pooled, const float* const* pre /*[]*/,
                             const float* const* o /*[]*/, float* const* dw1 /*[]*/, float* const* db1 /*[]*/,
                             float* const* dw2 /*[]*/, float* const* db2 /*[]*/, float* scratch, void* dfeat, void* stream);
/* the same with the feature gradient as ONE value per (image, channel): dfeat_nc [N][Cs] of dtype (Cs == C), = dpooled / HW,
 * what every pixel of that image and channel receives from the global average pool (heads.py:9-18).  The N x HW x Cs
 * broadcast is never written; spcl_bnrelu_backward_bcast consumes the [N][Cs] form. */
int spcl_proj_heads_backward_pooled(int K, const float* const* dz, int dtype, int N, int HW, int C, int Cs,
                                    const float* const* w1, const float* const* w2, int hid, int out_dim, int normalize,
                                    const float* pooled, const float* const* pre, const float* const* o, float* const* dw1,
                                    float* const* db1, float* const* dw2, float* const* db2, float* scratch, void* dfeat_nc,
                                    void* stream);

/* ---------------------------------------------------------------- encoder --------------------------------
 * Replaces semi_seg/arch/unet.py:67-82 (_ConvBlock: Conv2d 3x3 no bias -> BatchNorm2d -> ReLU, x2),
 * :118-121 (MaxPool2d 2x2), :156-190 (forward until Conv5) and their autograd backward (K1-K4, K17).
 */

/* weights: OIHW f32 master (state_dict layout) -> MFMA fragment-packed kernel layout (zero padded to 16-channel
 * multiples).  kind 0: forward  (K = (tap, ci), N = co);  kind 1: dgrad (K = (tap', co), N = ci, taps flipped
 * 180 degrees) -- the data gradient of a 3x3 same-conv is the same conv on these weights.
 * size in elements of `dtype`: spcl_conv_packed_elems(Cin, Cout, kind, dtype). */
size_t spcl_conv_packed_elems(int Cin, int Cout, int kind, int dtype);
int spcl_conv_pack_weights(const float* w_oihw, int Cin, int Cout, int kind, int dtype, void* packed, void* stream);
/* both layouts of one layer in one launch (forward keeps the dgrad copy for its backward) */
int spcl_conv_pack_weights_both(const float* w_oihw, int Cin, int Cout, int dtype, void* packed_fwd,
                                void* packed_dgrad, void* stream);

/* both convolutions of a Conv-BN-ReLU x2 block (forward + dgrad layouts each, sizes as spcl_conv_packed_elems) in one
 * launch, issued right before the block so that the fragments are still in L2 when its kernels fetch them */
int spcl_conv_pack_weights_block(const float* wa_oihw, int CinA, int CoutA, void* a_fwd, void* a_dgrad,
                                 const float* wb_oihw, int CinB, int CoutB, void* b_fwd, void* b_dgrad, int dtype,
                                 void* stream);
/* the same for weights that will be used at image size H x W: the band-GEMM layout of a dual-layout buffer is written only
 * where spcl_conv3x3_forward picks that kernel at this size (H = W = 0: both layouts, == spcl_conv_pack_weights_block) */
int spcl_conv_pack_weights_block_at(const float* wa_oihw, int CinA, int CoutA, void* a_fwd, void* a_dgrad,
                                    const float* wb_oihw, int CinB, int CoutB, void* b_fwd, void* b_dgrad, int dtype,
                                    int H, int W, void* stream);

/* forward + dgrad layouts of up to SPCL_PACK_MULTI_MAX layers in ONE launch (every conv weight of the UNet encoder at the
 * start of its forward pass: unet.py:123-131 are ten nn.Conv2d; one launch instead of one per block).  Per layer: the
 * OIHW master, both destination buffers (sizes as spcl_conv_packed_elems) and the image size it will be used at (as
 * spcl_conv_pack_weights_block_at: 0, 0 = both layouts of a dual-layout buffer).  items is host memory, read during the
 * call. */
#define SPCL_PACK_MULTI_MAX 24
typedef struct spcl_pack_item {
  const float* w_oihw;
  void* fwd;
  void* dgrad;
  int Cin, Cout, H, W;
} spcl_pack_item;
int spcl_conv_pack_weights_multi(const spcl_pack_item* items, int n, int dtype, void* stream);
/* the same launch also runs spcl_image_autocorr(image, N, H, W, acorr) (see "image3" below) in workgroups of its own: two
 * short, independent jobs at the start of a forward pass overlap and pay one launch.  image == NULL: the plain pack. */
int spcl_conv_pack_weights_multi_acorr(const spcl_pack_item* items, int n, int dtype, const float* image, int N, int H,
                                       int W, float* acorr, void* stream);
/* ... and zeroes zero_bytes bytes at `zero` in the same launch (the step's BatchNorm accumulator blocks, see spcl_bn_acc below:
 * they must be zero before the first convolution of the pass, and this is the pass's first launch).  zero == NULL: none. */
int spcl_conv_pack_weights_multi_zero(const spcl_pack_item* items, int n, int dtype, const float* image, int N, int H, int W,
                                      float* acorr, void* zero, size_t zero_bytes, void* stream);

/* y = conv3x3(act(x)), NHWC, implicit GEMM on MFMA.                    (unet.py:72,75; dgrad: with kind-1 weights)
 * x [N,H,W,CinS] of dtype; CinK = GEMM-K channels (multiple of 16, == CinS for in_mode 0/1).
 * in_mode 0: act = identity;  1: act = relu(in_scale[c]*x+in_shift[c])  (the producer's BatchNorm-apply + ReLU,
 * unet.py:73-74, fused into the load);  2: x is the f32 input image [N,H,W,CinS] with CinS<=16 real channels
 * (== NCHW when CinS==1), zero-padded to CinK=16 on load.
 * y [N,H,W,CoutS] raw conv output (dtype).  stats != NULL: per-tile Chan partials (count, mean, M2) per output
 * channel, one row stats[tile][3][CoutS] f32 per pixel tile (tile < spcl_conv_num_tiles(N,H,W)), for the train-mode
 * BatchNorm that follows; the buffer holds spcl_bn_stats_elems(ntiles, CoutS) floats (tile rows + the finalize
 * kernel's partial rows). */
int spcl_conv_num_tiles(int N, int H, int W);
/* Statistics rows the convolution of this configuration writes (stats [rows][3][CoutS], rows2 [rows][2][CoutS]): the
 * pixel tiles above, except where the workgroup-level GEMM kernel runs (csrc/conv_gemm.hip: bf16, channel counts
 * multiples of 64 with one side >= 128, see spcl_conv_set_gemm), which writes one row per (image band, pixel part). */
int spcl_conv_stat_rows(int dtype, int N, int H, int W, int CinK, int CoutS);
/* Which kernel takes those layers: -1 (default) the GEMM kernel only at image sizes the per-wave kernels have no
 * specialisation for (widths that do not tile by 14 columns: the 32^2 / 16^2 levels of 256^2 inputs), 1 wherever it fits,
 * 0 never.  Packed weights are valid under every setting. */
void spcl_conv_set_gemm(int mode);
/* How the f32-storage convolutions (forward, data gradient, weight gradient: nn.Conv2d of unet.py:72,75 run in torch's default
 * float32, the north_star's "within fp32 tolerance" path) multiply: 1 (default) every f32 operand as the exact sum of three
 * bf16 pieces, six v_mfma_f32_16x16x32_bf16 products per pair accumulated in f32 (the dropped terms are below 2^-24 of a
 * product: f32-grade results at 3/8 of the exact path's matrix time); 0 v_mfma_f32_16x16x4_f32 (exact f32 products, 1/16 of
 * the bf16 matrix rate).  Packed f32 weights carry both layouts: the switch may change between any two launches.  One
 * process-wide setting, read at launch time on the calling thread (not synchronised: set it before the threads that launch
 * start, as the tests and bench.py --f32-exact do).  The one-channel image convolution (in_mode 2, CoutS == 16) is a direct
 * exact-FMA kernel under both settings. */
void spcl_conv_set_f32_split(int on);
int spcl_conv_get_f32_split(void);
size_t spcl_bn_stats_elems(int ntiles, int CS);
int spcl_conv3x3_forward(const void* x, int dtype, int N, int H, int W, int CinS, int CinK, int CoutS,
                         const void* w_packed, int in_mode, const float* in_scale, const float* in_shift, void* y,
                         float* stats, void* stream);
/* The first convolution of the image block (semi_seg/arch/unet.py:123 behind :67-71, nn.Conv2d(1, 16, 3, 1, 1, bias=False)
 * on the f32 slice, in_mode 2 of spcl_conv3x3_forward) that ALSO leaves the image's autocorrelation partial rows -- what
 * spcl_image_autocorr / spcl_conv_pack_weights_multi_acorr compute in a pass of their own for the "image3" backward of that
 * convolution (spcl_bnrelu_backward_rows_image3): acorr_rows [rows][64] f32, one row per 14 x 14 tile, same layout and
 * meaning per row (45 upper-triangle sums R[t'][t] + 9 image sums over the tile's pixels), so spcl_conv16_bwd_fused's
 * fold and the image3 final kernels take them unchanged.  _rows: the number of rows, 0 where the specialised kernel does
 * not take the shape (bf16, CinS == 1, CoutS == 16, H and W multiples of 14 above 112): where the library's own dispatch
 * runs it.  The call itself takes every whole-tile size (H and W multiples of 14): spcl_block1_kernels_take answers for the
 * call.
 * y == NULL: the statistics-only form -- stats and acorr_rows bit for bit as with y, no output stream (32 of the launch's 36
 * bytes per pixel); the raw output is then formed again, per tile and bit for bit, by the two launches that read it:
 * spcl_conv3x3_forward_from_image and spcl_conv16_bwd_fused_image. */
int spcl_conv3x3_forward_image_acorr_rows(int dtype, int N, int H, int W, int CinS, int CoutS);
int spcl_conv3x3_forward_image_acorr(const void* x, int dtype, int N, int H, int W, int CinS, int CoutS,
                                     const void* w_packed, void* y, float* stats, float* acorr_rows, void* stream);
/* The image block WITHOUT the first convolution's raw output (unet.py:123 -> :72-75 of the reference: Conv2d(1, 16) ->
 * BatchNorm2d -> ReLU -> Conv2d(16, 16); the tensor between the two convolutions is 103 MB at 64 x 224^2 and was written once
 * and read twice per step).  spcl_conv3x3_forward_from_image is the second convolution (what spcl_conv3x3_forward(in_mode 1,
 * in_scale, in_shift) computes from the stored tensor, replacing unet.py:72-75's BatchNorm2d / ReLU / Conv2d reads of it): per
 * 14 x 14 tile it forms the first convolution's output on the 16 x 16 halo from the f32 image [N][H][W] and
 * w_packed_image (spcl_conv_pack_weights kind 0 of the [16][1][3][3] filters) with the instruction, operand packing and
 * rounding of spcl_conv3x3_forward_image_acorr -- the same bits -- then applies relu(in_scale y + in_shift), zero outside the
 * image.  y [N][H][W][16] bf16 and stats (one row set per 14 x 14 tile) as spcl_conv3x3_forward.  bf16, H and W multiples of
 * 14.  y_image != NULL: the stored tensor is read instead (image / w_packed_image unused), on the same tiles -- the comparison
 * form.  spcl_block1_recompute_supported: 1 where the library offers the block without the tensor, i.e. where all of its
 * three launches have their kernel (the statistics-only spcl_conv3x3_forward_image_acorr, this call on 14-row tiles,
 * spcl_conv16_bwd_fused_image): bf16, CinS == 1, CoutS == 16, H and W multiples of 14 above 112.  It answers for the kernels:
 * this call writes its statistics as per-tile rows only, so a caller whose second BatchNorm goes through an accumulator
 * block (spcl_conv_bn_acc_supported says yes: at most 4 096 tiles, e.g. N <= 16 at 224^2) keeps the stored tensor.
 * spcl_block1_kernels_take: 1 where the block's 14 x 14-tile kernels accept a CALL whatever tile the library's own dispatch
 * picks for the size -- this call, spcl_conv3x3_forward_image_acorr, spcl_conv16_bwd_fused and spcl_conv16_bwd_fused_image:
 * bf16, CinS == 1, CoutS == 16, H and W multiples of 14 (the _rows / _supported queries of those calls say where the
 * library itself uses them; this one says where they may be called). */
int spcl_block1_recompute_supported(int dtype, int N, int H, int W, int CinS, int CoutS);
int spcl_block1_kernels_take(int dtype, int N, int H, int W, int CinS, int CoutS);
int spcl_conv3x3_forward_from_image(const float* image, const void* y_image, int dtype, int N, int H, int W, int CoutS,
                                    const void* w_packed_image, const float* in_scale, const float* in_shift,
                                    const void* w_packed, void* y, float* stats, void* stream);
/* The decoder's torch.cat((skip, up), dim=1) -> Conv2d(2 Chalf, Cout, 3, 1, 1) (unet.py:194-197, 201-204, ... the first
 * convolution of every Up_conv block) WITHOUT the concatenated tensor: input channels [0, Chalf) are read from xa, [Chalf,
 * 2 Chalf) from xb, both dense [N][H][W][Chalf] bf16; w_packed = spcl_conv_pack_weights(kind 0) of the [Cout][2 Chalf]
 * weight, y / stats as spcl_conv3x3_forward.  Only where a specialised kernel exists (Chalf 16 or 32, 14-column tiles,
 * not a layer whose weight gradient the batched GEMM takes): spcl_conv_cat_supported answers; spcl_conv3x3_wgrad_cat is
 * the matching weight gradient (workspace: spcl_conv_wgrad_workspace_bytes with CinK = 2 Chalf).  The input gradient is the
 * ordinary dgrad: one [N][H][W][2 Chalf] tensor whose channel halves the two producers' backward passes read in place
 * (spcl_bnrelu_pool_backward_strided). */
int spcl_conv_cat_supported(int dtype, int N, int H, int W, int Chalf, int CoutS);
int spcl_conv3x3_forward_cat(const void* xa, const void* xb, int dtype, int N, int H, int W, int Chalf, int CoutS,
                             const void* w_packed, const float* xb_scale, const float* xb_shift, void* y, float* stats,
                             void* stream);
/* xb_scale / xb_shift [Chalf] (both, or both NULL; Chalf 16 / 32): xb is the RAW output of the up-convolution (unet.py:90) and
 * the concatenation holds relu(xb_scale xb + xb_shift) -- that BatchNorm + ReLU (unet.py:91-92) applied while the halo is
 * staged, so the up-convolution's activation is never written either. */
int spcl_conv3x3_wgrad_cat(const void* xa, const void* xb, const void* dy, int dtype, int N, int H, int W, int Chalf,
                           int Cout, int CoutS, const float* xb_scale, const float* xb_shift, float* partial,
                           float* dw_oihw, void* stream);
/* nn.Upsample(scale_factor=2) -> Conv2d of the up-convolution (unet.py:89-90) without the upsampled tensor: x_half is the
 * half-resolution activation [N][H / 2][W / 2][CinK], H x W the convolution's size; the loaders turn a fine halo pixel
 * (gy, gx) into pixel (gy >> 1, gx >> 1) of x_half.  Forward (y / stats as spcl_conv3x3_forward; where
 * spcl_conv_up2_supported says so) and weight gradient (workspace: spcl_conv_wgrad_workspace_bytes; the batched kernel
 * takes it through spcl_wgrad_item::x_up2).  The input gradient is the ordinary dgrad followed by the 2 x 2 sum
 * (spcl_upsample2x_backward / spcl_bnrelu_backward_up2). */
int spcl_conv_up2_supported(int dtype, int N, int H, int W, int CinK, int CoutS);
int spcl_conv3x3_forward_up2(const void* x_half, int dtype, int N, int H, int W, int CinK, int CoutS, const void* w_packed,
                             void* y, float* stats, void* stream);
int spcl_conv3x3_wgrad_up2(const void* x_half, const void* dy, int dtype, int N, int H, int W, int Cin, int Cout, int CoutS,
                           float* partial, float* dw_oihw, void* stream);
/* ... and the input gradient of that convolution as the gradients of the two concatenated tensors: the plain 3x3 convolution
 * (w_packed = the dgrad layout, kind 1) whose output channels [0, CoutS / 2) are written to y_lo and [CoutS / 2, CoutS) to
 * y_hi, both dense [N][H][W][CoutS / 2] bf16 (torch.cat's backward, unet.py:194-224, without the interleaved tensor).
 * Where spcl_conv_split_supported says so (a specialised kernel, CoutS a multiple of 32). */
int spcl_conv_split_supported(int dtype, int N, int H, int W, int CinK, int CoutS);
int spcl_conv3x3_forward_split(const void* x, int dtype, int N, int H, int W, int CinK, int CoutS, const void* w_packed,
                               void* y_lo, void* y_hi, void* stream);
/* ... the same with the BatchNorm-backward partial sums of the layer behind the UPPER half -- the up-convolution (unet.py:90-92):
 * y2_hi [N][H][W][CoutS / 2] its raw output, scale2 / shift2 / mean2 [CoutS / 2] its coefficients; rows2
 * [spcl_conv_stat_rows(dtype, N, H, W, CinK, CoutS)][2][CoutS / 2] (sum dz, sum dz (y2 - mean)) as spcl_conv3x3_dgrad_bnstats
 * leaves them, for spcl_bnrelu_backward_rows: that layer's reduction pass over (y2, g_hi) disappears. */
int spcl_conv_split_bnstats_supported(int dtype, int N, int H, int W, int CinK, int CoutS);
int spcl_conv3x3_dgrad_split_bnstats(const void* dy, int dtype, int N, int H, int W, int CinK, int CoutS,
                                     const void* w_packed, void* g_lo, void* g_hi, const void* y2_hi, const float* scale2,
                                     const float* shift2, const float* mean2, float* rows2, void* stream);

/* dW[co][ci][ky][kx] (OIHW f32, overwritten) = sum_pixels act(x)[p+tap][ci] * dy[p][co]   (weight gradient of
 * unet.py:72,75).  x / in_mode / CinK as in forward; Cin, Cout = real channel counts of dW.
 * partial: workspace of spcl_conv_wgrad_workspace_bytes() (deterministic two-stage reduction, no atomics). */
size_t spcl_conv_wgrad_workspace_bytes(int N, int H, int W, int CinK, int CoutS);
int spcl_conv3x3_wgrad(const void* x, const void* dy, int dtype, int N, int H, int W, int Cin, int CinS, int CinK,
                       int Cout, int CoutS, int in_mode, const float* in_scale, const float* in_shift, float* partial,
                       float* dw_oihw, void* stream);

/* nn.AdaptiveAvgPool2d / nn.AdaptiveMaxPool2d((OH, OW)) on an NHWC tensor x [N,H,W,Cs] of dtype (C real channels) ->
 * out [N,OH,OW,C] f32 (contrastyou/projectors/nn.py:56-64: the pooling of ProjectionHead(pool_name="adaptive_max") and of
 * DenseProjectionHead, heads.py:96-120).  mode 0 average, 1 maximum (argmax [N,OH,OW,C] int32 receives the flat y * W + x of
 * the first maximum).  Backward: dx [N,H,W,Cs] of dtype, deterministic (one thread per input element, no atomics). */
int spcl_adaptive_pool2d_forward(const void* x, int dtype, int N, int H, int W, int C, int Cs, int OH, int OW, int mode,
                                 float* out, int* argmax, void* stream);
int spcl_adaptive_pool2d_backward(const float* dout, const int* argmax, int dtype, int N, int H, int W, int C, int Cs,
                                  int OH, int OW, int mode, void* dx, void* stream);

/* F.normalize(p=2, dim=-1, eps=1e-12) of `rows` rows of O floats (projectors/nn.py:29-36 on a pixel-major map) and its
 * backward. */
int spcl_l2norm_rows_forward(const float* x, size_t rows, int O, float* z, void* stream);
int spcl_l2norm_rows_backward(const float* x, const float* dz, size_t rows, int O, float* dx, void* stream);

/* Normalize() and SoftmaxWithT's division of the cluster heads, on the logits (contrastyou/projectors/heads.py:42-75 with
 * nn.py:29-36, :50-58 of the reference): over `rows` rows of pitch ld, per subhead s < S,
 *   z[m][s*K + k] = l[m][s*K + k] / max(||l[m][s*K ..]||_2, 1e-12) / T        (normalize == 0: l / T)
 * and the exact backward (below 1e-12 the denominator is the constant).  f32, one thread per (row, subhead), no atomics;
 * columns >= S*K are neither read nor written.  z, dz and dl have the pitch of l.  T > 0. */
int spcl_group_l2norm_temp_forward(const float* l, size_t rows, long ld, int S, int K, int normalize, float T, float* z,
                                   void* stream);
int spcl_group_l2norm_temp_backward(const float* l, const float* dz, size_t rows, long ld, int S, int K, int normalize, float T,
                                    float* dl, void* stream);

/* The same weight gradients for SEVERAL layers in ONE launch (bf16, channel counts multiples of 64: _Conv3.b.._Conv5.b
 * and the decoder's wide layers).  The workgroups split the union of the layers' pixel ranges, so the launch writes
 * one split-K partial per CU in total instead of one per CU and layer (csrc/wgrad_gemm.hip).  x / dy / in_mode (0 or
 * 1) / in_scale / in_shift as above with CinK == Cin; dw_oihw [Cout][Cin][3][3] f32 is overwritten, or added to when
 * accumulate != 0 (a gradient bucket that was zeroed before backward and may already hold another use's gradient).
 * partial: spcl_conv_wgrad_batched_workspace_bytes(items, n) bytes.  items is host memory, read during the call. */
#define SPCL_WGRAD_BATCH_MAX 16
typedef struct spcl_wgrad_item {
  const void* x;
  const void* dy;
  const float* in_scale;
  const float* in_shift;
  float* dw_oihw;
  int N, H, W, Cin, CinS, Cout, CoutS, in_mode;
  const void* x2; /* NULL, or: input channels [Cin / 2, Cin) come from this tensor and [0, Cin / 2) from x, both dense
                     [N][H][W][Cin / 2] (the decoder's concatenation read in place; Cin a multiple of 128, in_mode 0) */
  int x_up2;      /* 1: x is [N][H / 2][W / 2][CinS] and the layer's input its nearest x2 upsample (unet.py:89), in_mode 0 */
} spcl_wgrad_item;
int spcl_conv_wgrad_batched_supported(int dtype, int Cin, int CinS, int Cout, int CoutS, int in_mode);
size_t spcl_conv_wgrad_batched_workspace_bytes(const spcl_wgrad_item* items, int n);
int spcl_conv3x3_wgrad_batched(const spcl_wgrad_item* items, int n, int accumulate, float* partial, void* stream);

/* Deferred final sums ("tails") of the weight gradients that do NOT go through the batched GEMM kernel: the narrow
 * layers' split partials of spcl_conv3x3_wgrad and the first layer's per-workgroup rows of the fused BN-backward +
 * weight-gradient pass (spcl_bnrelu_backward_image_wgrad / spcl_bnrelu_backward_rows with an image).  Each of those
 * ends in its own few-microsecond reduction launch; with a capture armed the producer skips it and describes the
 * pending sum instead, and spcl_conv3x3_wgrad_batched_tails finishes up to SPCL_WGRAD_TAILS_MAX of them in extra
 * workgroups of the batched launch's reduction kernel (fixed summation order; dw written, or added to when
 * accumulate != 0).  The producer's `partial` / `ws` buffer must stay alive until that launch has run.
 *   spcl_wgrad_tail_capture(slot): one-shot, per calling thread -- the NEXT call of one of the producers above fills
 *   *slot and leaves dw untouched (slot == NULL disarms).  A producer that takes the batched path itself (bf16, channel
 *   counts multiples of 64) ignores the capture and clears it; slot->kind stays -1 then.
 * unet.py:72,75 weight gradients; replaces nothing new in the reference, only removes launches. */
#define SPCL_WGRAD_TAILS_MAX 16
typedef struct spcl_wgrad_tail {
  const float* partial; /* kind 0: [nsplit][nblk_ci*nblk_co][9*CIB*COB]; kind 1: [nsplit][9][COB] */
  float* dw;            /* OIHW destination */
  int kind;             /* -1 empty, 0 conv split partials, 1 first-layer rows */
  int nsplit, nblk_ci, nblk_co, CIB, COB, Cin, Cout;
} spcl_wgrad_tail;
int spcl_wgrad_tail_capture(spcl_wgrad_tail* slot);
/* n may be 0 (tails only; partial may then be NULL), ntails may be 0 (== spcl_conv3x3_wgrad_batched) */
int spcl_conv3x3_wgrad_batched_tails(const spcl_wgrad_item* items, int n, const spcl_wgrad_tail* tails, int ntails,
                                     int accumulate, float* partial, void* stream);
/* train-mode BatchNorm statistics (unet.py:73,76; torch.nn.BatchNorm2d semantics): combines the conv epilogue
 * partials stats[ntiles][3][CS] (Chan, fixed order, in double; the tail of the buffer is scratch) -> mean, invstd = 1/sqrt(var_biased+eps), scale = gamma*invstd,
 * shift = beta-mean*scale (all [CS] f32, zero in the channel padding) and updates running_mean / running_var
 * (unbiased variance, momentum) and num_batches_tracked (+1) when those pointers are non-NULL. */
int spcl_bn_finalize(float* stats, int ntiles, int C, int CS, const float* gamma, const float* beta,
                     float momentum, float eps, float* running_mean, float* running_var,
                     int64_t* num_batches_tracked, float* mean, float* invstd, float* scale, float* shift,
                     void* stream);
/* eval mode: mean/invstd/scale/shift from the running statistics */
int spcl_bn_eval_affine(int C, int CS, const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, float eps, float* mean, float* invstd, float* scale, float* shift,
                        void* stream);
/* ... of up to SPCL_BN_EVAL_MAX BatchNorms in one launch (the eval-mode forward of the full UNet: 22 layers); st: [4][CS] =
 * mean, invstd, scale, shift of that layer, as spcl_bn_eval_affine writes them. */
#define SPCL_BN_EVAL_MAX 32
typedef struct {
  const float* gamma;
  const float* beta;
  const float* running_mean;
  const float* running_var;
  float* st;
  int C, CS;
  float eps;
} spcl_bn_eval_item;
int spcl_bn_eval_affine_multi(const spcl_bn_eval_item* items, int n, void* stream);

/* a = relu(scale*y+shift) [N,H,W,CS] (act_out, may be NULL) and/or its 2x2/2 max-pool p [N,H/2,W/2,CS]
 * (pool_out, may be NULL)                                                       -- unet.py:74,77 + :118-121 */
int spcl_bnrelu_pool_forward(const void* y, int dtype, int N, int H, int W, int CS, const float* scale,
                             const float* shift, void* act_out, void* pool_out, void* stream);
/* backward of the above through ReLU, (optional) max-pool and BatchNorm:
 *   g  = dact (+ dpool routed to the window arg-max: first maximum in scan order, as torch.max_pool2d)
 *   dz = g * [scale*y+shift > 0];  dbeta = sum dz;  dgamma = sum dz*yhat,  yhat = (y-mean)*invstd
 *   training: dy = scale*(dz - dbeta/M - yhat*dgamma/M);   eval: dy = scale*dz
 * dact / dpool may be NULL (not both).  Deterministic: per-workgroup partials + fixed-order second stage. */
size_t spcl_bnrelu_bwd_workspace_bytes(int N, int H, int W, int CS);
int spcl_bnrelu_pool_backward(const void* y, const void* dact, const void* dpool, int dtype, int N, int H, int W,
                              int C, int CS, const float* mean, const float* invstd, const float* scale,
                              const float* shift, int training, float* ws, float* dgamma, float* dbeta, void* dy,
                              void* stream);
/* The same two calls with the activation written / its gradient read as a CHANNEL SLICE of a wider NHWC tensor
 * (act_stride / dact_stride = elements between two pixels, >= CS, a multiple of 8): the decoder's
 * `torch.cat((skip, up), dim=1)` (semi_seg/arch/unet.py:194-224) then needs no copy in either direction -- both producers
 * write their half of the concatenated tensor, both consumers read their half of its gradient (round 4, row N1). */
/* BN-apply + ReLU written 2x2-REPLICATED: up_out [N][2H][2W][CS] = nearest-upsample(relu(scale y + shift)) -- the activation of
 * a block whose only consumer is the decoder's nn.Upsample(scale_factor=2) (semi_seg/arch/unet.py:89): neither the
 * low-resolution activation nor a separate upsampling pass is written (round 4, row N1). */
int spcl_bnrelu_up2_forward(const void* y, int dtype, int N, int H, int W, int CS, const float* scale, const float* shift,
                            void* up_out, void* stream);
int spcl_bnrelu_pool_forward_strided(const void* y, int dtype, int N, int H, int W, int CS, const float* scale,
                                     const float* shift, void* act_out, int act_stride, void* pool_out, void* stream);
int spcl_bnrelu_pool_backward_strided(const void* y, const void* dact, int dact_stride, const void* dpool, int dtype, int N,
                                      int H, int W, int C, int CS, const float* mean, const float* invstd,
                                      const float* scale, const float* shift, int training, float* ws, float* dgamma,
                                      float* dbeta, void* dy, void* stream);
/* BN + ReLU backward of a block whose activation went through nn.Upsample(scale_factor=2) (unet.py:89) before its consumer:
 * d_up = the gradient w.r.t. the UPSAMPLED activation [N][2H][2W][CS]; the 2 x 2 sums (spcl_upsample2x_backward) are formed
 * inside the BatchNorm-backward reduction pass and left in dact [N][H][W][CS] (scratch, written) for the apply pass.  Results as
 * spcl_upsample2x_backward followed by spcl_bnrelu_pool_backward(y, dact, NULL, ...), bit for bit; one pass over the fine
 * gradient and one launch less. */
int spcl_bnrelu_backward_up2(const void* y, const void* d_up, void* dact, int dtype, int N, int H, int W, int C, int CS,
                             const float* mean, const float* invstd, const float* scale, const float* shift, int training,
                             float* ws, float* dgamma, float* dbeta, void* dy, void* stream);
/* BN + ReLU backward (no pooling) for a gradient that is the same for every pixel of an image: dact_nc [N][CS] of dtype.
 * Same arithmetic as spcl_bnrelu_pool_backward(dact = the expanded tensor, dpool = NULL). */
int spcl_bnrelu_backward_bcast(const void* y, const void* dact_nc, int dtype, int N, int H, int W, int C, int CS,
                               const float* mean, const float* invstd, const float* scale, const float* shift, int training,
                               float* ws, float* dgamma, float* dbeta, void* dy, void* stream);

/* BatchNorm+ReLU backward of the FIRST conv of a one-channel image block, fused with that conv's weight gradient
 * (`_Conv1.conv.0`/`.1`/`.2` backward, semi_seg/arch/unet.py:70-72 with input_dim = 1, + autograd).  The input image
 * needs no gradient, so this layer's dy feeds nothing but dW: it is formed in registers and never written.
 *   y, dact   [N][H][W][CS] of dtype (raw conv output, gradient of the activation);  image [N][H][W] f32
 *   dw        [C][1][3][3] f32;  dgamma, dbeta [C];  ws of spcl_bnrelu_image_wgrad_workspace_bytes
 * CS a power of two in 16..256.  Deterministic (fixed workgroup partition, fixed-order sums). */
size_t spcl_bnrelu_image_wgrad_workspace_bytes(int N, int H, int W, int CS);
int spcl_bnrelu_backward_image_wgrad(const void* y, const void* dact, const float* image, int dtype, int N, int H,
                                     int W, int C, int CS, const float* mean, const float* invstd, const float* scale,
                                     const float* shift, int training, float* ws, float* dgamma, float* dbeta,
                                     float* dw, void* stream);

/* dgrad of a block's SECOND conv fused with the per-tile partial sums of the FIRST conv's BatchNorm backward
 * (`_ConvBlock.conv.3` input gradient -> `.conv.1/.2` backward, semi_seg/arch/unet.py:70-77 + autograd): the dgrad's
 * output g is d loss / d relu(bn(y2)), so its epilogue already holds what the reduction pass over (y2, g) would read.
 *   dy [N][H][W][CinK], g [N][H][W][CoutS], y2 [N][H][W][CoutS] (raw output of the first conv), all bf16;
 *   rows2 [spcl_conv_num_tiles(N,H,W)][2][CoutS] f32: sum dz and sum dz (y2 - mean) per conv tile, dz = g [bn(y2) > 0].
 * Exists only where a specialised conv kernel does: ask spcl_conv_dgrad_bnstats_supported (1 / 0) first, else run
 * spcl_conv3x3_forward + spcl_bnrelu_pool_backward.  spcl_bnrelu_backward_rows finishes from the rows: dgamma, dbeta and
 * either dy (image == dw == NULL) or, for a one-channel image block, that layer's dW (dy == NULL), as the two entry
 * points above do after their own reduction pass.  Same workspace sizes as those. */
int spcl_conv_dgrad_bnstats_supported(int dtype, int N, int H, int W, int CinK, int CoutS);
int spcl_conv3x3_dgrad_bnstats(const void* dy, int dtype, int N, int H, int W, int CinK, int CoutS, const void* w_packed,
                               void* g, const void* y2, const float* scale2, const float* shift2, const float* mean2,
                               float* rows2, void* stream);

/* ---- image3: the first conv of a block whose input is a ONE-CHANNEL f32 image (unet.py:123 with input_dim == 1, the
 * configuration every driver of the reference uses).  Its BatchNorm backward and weight gradient need no pass over the
 * activations: with dy = scale dz + A y + B (the folded BN backward), dW[c][t] = scale[c] sum_p dz[p][c] img[p + t] +
 * A[c] (W R)[c][t] + B[c] sum_p img[p + t], R = the 9 x 9 autocorrelation of the zero-padded image batch (y is linear in
 * the image).  Replaces spcl_bnrelu_backward_rows(image != NULL) + the dgrad before it where supported (bf16, 16 -> 16
 * channels, sizes tiled 14 x 14):
 *   spcl_image_autocorr          image [N][H][W] f32 (W <= 256) -> out [spcl_image_autocorr_rows(N, H, W)][64] partial rows
 *   spcl_conv3x3_dgrad_bnstats_image   spcl_conv3x3_dgrad_bnstats + rows 2 .. 10 of rows11 [tiles][11][CoutS] = the nine
 *                                sums sum_p dz[p][co] image[p + tap] (tiles = spcl_conv_stat_rows); g == NULL: the
 *                                gradient tensor is not written (image3 needs only the rows)
 *   spcl_bnrelu_backward_rows_image3   rows11 + autocorrelation + the f32 master weights [C][1][3][3] -> dgamma, dbeta, dW
 *                                (ws: spcl_bnrelu_image3_workspace_bytes(CS) bytes) */
int spcl_image_autocorr_rows(int N, int H, int W);
int spcl_image_autocorr(const float* image, int N, int H, int W, float* out, void* stream);
int spcl_conv_dgrad_bnstats_image_supported(int dtype, int N, int H, int W, int CinK, int CoutS);
int spcl_conv3x3_dgrad_bnstats_image(const void* dy, int dtype, int N, int H, int W, int CinK, int CoutS,
                                     const void* w_packed, void* g, const void* y2, const float* scale2,
                                     const float* shift2, const float* mean2, const float* image, float* rows11,
                                     void* stream);
/* The image block's SECOND conv (unet.py:75 at 16 -> 16 channels), its whole backward in one pass over dy and y2: the
 * weight gradient (what spcl_conv3x3_wgrad(x = y2, in_mode 1, scale2, shift2) computes; partial = the split slabs,
 * spcl_conv16_bwd_fused_splits(N, H, W) x 9 x 256 floats; the final sum goes to dw_oihw [Cout][Cin][3][3] or to a captured
 * tail, as there) AND the rows11 of spcl_conv3x3_dgrad_bnstats_image(g == NULL).  Nothing is written per pixel.
 * Same gate as spcl_conv_dgrad_bnstats_image_supported (where the library's own dispatch runs it; the call also takes every
 * image whose H and W are multiples of 14: spcl_block1_kernels_take).
 * Exactly one of rows11 ([tiles][11][CoutS], as above) / wg_rows: ONE row set per workgroup (its tiles summed in
 * registers), [11][16][spcl_conv16_bwd_fused_splits] -- the layout spcl_bnrelu_backward_wgrows_image3 finishes from without
 * a folding launch; with wg_rows the same launch folds the autocorrelation's partial rows acorr [nacorr][64] to
 * acorr16 [16][64]. */
int spcl_conv16_bwd_fused_supported(int dtype, int N, int H, int W, int CinK, int CoutS);
int spcl_conv16_bwd_fused_splits(int N, int H, int W);
int spcl_conv16_bwd_fused(const void* dy, int dtype, int N, int H, int W, const void* w_packed_dgrad, const void* y2,
                          const float* scale2, const float* shift2, const float* mean2, const float* image,
                          float* rows11, float* partial, float* dw_oihw, int Cin, int Cout, float* wg_rows,
                          const float* acorr, int nacorr, float* acorr16, void* stream);
/* spcl_conv16_bwd_fused for a first conv whose raw output y2 was never stored (the backward of unet.py:75 and of the
 * BatchNorm2d / ReLU of unet.py:73-74 in front of it): y2 is formed per tile from `image` and w_packed_image (kind 0 of the
 * [16][1][3][3] filters), bit for bit what spcl_conv3x3_forward_image_acorr stores; every output as spcl_conv16_bwd_fused.
 * bf16, H and W multiples of 14 (spcl_conv16_bwd_fused_image_supported). */
int spcl_conv16_bwd_fused_image_supported(int dtype, int N, int H, int W, int CinK, int CoutS);
int spcl_conv16_bwd_fused_image(const void* dy, int dtype, int N, int H, int W, const void* w_packed_dgrad,
                                const void* w_packed_image, const float* scale2, const float* shift2, const float* mean2,
                                const float* image, float* rows11, float* partial, float* dw_oihw, int Cin, int Cout,
                                float* wg_rows, const float* acorr, int nacorr, float* acorr16, void* stream);
/* spcl_conv16_bwd_fused_image whose incoming gradient dy is never stored either: the block's output goes through
 * nn.BatchNorm2d / nn.ReLU (unet.py:75-77) and nn.MaxPool2d(2, 2) (unet.py:118-121) only, so dy is the autograd backward of
 * those three applied to dpool -- what spcl_bnrelu_backward_rows_acc(y, dact = NULL, dpool, rows, ..) writes.  The call takes
 * that call's inputs in dy's place: y [N][H][W][16] (this convolution's raw output), dpool [N][H/2][W/2][16], the per-tile
 * rows [nrows][2][16] of the BatchNorm's backward sums, its forward st4 [4][16] and its ZEROED accumulator block acc.  One
 * small launch adds the rows to the block (as there); the one-pass kernel derives the BatchNorm's folded coefficients from it,
 * forms dy per tile in its loader -- bit for bit the tensor the apply pass would have written, zero outside the image -- and
 * its first workgroup writes dgamma / dbeta [16].  Every other argument and output as spcl_conv16_bwd_fused_image.
 * _supported: training mode, bf16, 16 -> 16 channels, H and W multiples of 14 (hence even), the row-mapped two-wave kernel,
 * one image under 2 GiB. */
int spcl_conv16_bwd_fused_image_pooled_supported(int dtype, int N, int H, int W, int CinK, int CoutS, int training);
int spcl_conv16_bwd_fused_image_pooled(const void* y, const void* dpool, const float* rows, int nrows, int dtype, int N, int H,
                                       int W, const float* st4, int training, long long* acc, float* dgamma, float* dbeta,
                                       const void* w_packed_dgrad, const void* w_packed_image, const float* scale2,
                                       const float* shift2, const float* mean2, const float* image, float* rows11,
                                       float* partial, float* dw_oihw, int Cin, int Cout, float* wg_rows, const float* acorr,
                                       int nacorr, float* acorr16, void* stream);
int spcl_bnrelu_backward_wgrows_image3(const float* wg_rows, int nwg, const float* acorr, int nacorr, const float* w_oihw,
                                       int N, int H, int W, int C, int CS, const float* mean, const float* invstd,
                                       const float* scale, int training, float* ws, float* dgamma, float* dbeta,
                                       float* dw, void* stream);
size_t spcl_bnrelu_image3_workspace_bytes(int CS);
int spcl_bnrelu_backward_rows_image3(const float* rows11, int nrows, const float* acorr, int nacorr, const float* w_oihw,
                                     int N, int H, int W, int C, int CS, const float* mean, const float* invstd,
                                     const float* scale, int training, float* ws, float* dgamma, float* dbeta, float* dw,
                                     void* stream);

/* The same across a POOLED block boundary: dy = gradient of the next block's first conv output (H x W), g = its input
 * gradient = d loss / d maxpool2x2(relu(bn(y2))), y2 [N][H2][W2][CoutS] the raw second-conv output of the block before
 * (H == H2 / 2, W == W2 / 2; semi_seg/arch/unet.py:118-121,159-166).  rows2 [spcl_conv_stat_rows(...)][2][CoutS]: per conv
 * tile, sum dz and sum dz (y2 - mean) with dz = g routed to the window's first positive maximum -- what
 * spcl_bnrelu_pool_backward's reduction pass computes, without that pass.  bf16, per-wave kernels only: ask
 * spcl_conv_dgrad_poolstats_supported first; finish with spcl_bnrelu_pool_backward_rows. */
int spcl_conv_dgrad_poolstats_supported(int dtype, int N, int H, int W, int CinK, int CoutS, int H2, int W2);
int spcl_conv3x3_dgrad_poolstats(const void* dy, int dtype, int N, int H, int W, int CinK, int CoutS, const void* w_packed,
                                 void* g, const void* y2, int H2, int W2, const float* scale2, const float* shift2,
                                 const float* mean2, float* rows2, void* stream);
int spcl_bnrelu_pool_backward_rows(const void* y, const void* dpool, const float* rows, int nrows, int dtype, int N, int H,
                                   int W, int C, int CS, const float* mean, const float* invstd, const float* scale,
                                   const float* shift, int training, float* ws, float* dgamma, float* dbeta, void* dy,
                                   void* stream);
int spcl_bnrelu_backward_rows(const void* y, const void* dact, const float* image, const float* rows, int nrows, int dtype,
                              int N, int H, int W, int C, int CS, const float* mean, const float* invstd,
                              const float* scale, const float* shift, int training, float* ws, float* dgamma,
                              float* dbeta, void* dy, float* dw, void* stream);


/* ---------------------------------------------------------------------------------------------------------------
 * Segmentation head and fine-tune / evaluation arithmetic.  Activations [npix][CS] of dtype (NHWC,
 * npix = N*H*W); class maps [npix][K] f32 with K <= 16; labels [npix] int64.
 *   spcl_conv1x1_forward/backward   nn.Conv2d(C, K, 1) with bias = `_Deconv_1x1`, semi_seg/arch/unet.py:147,229 (+ autograd):
 *                                   out = x W^T + b;  dx (dtype, padding channels zeroed), dW [K][C], db [K]
 *   spcl_softmax_forward/backward   `logits.softmax(1)` of semi_seg/epochers/new_epocher.py:86,271 (+ autograd)
 *   spcl_kl_div_forward/backward    deepclustering2.loss.KL_div(reduction="mean") as called there (un-vendored; restated):
 *                                   loss = mean_p sum_k -t log((p+eps)/(t+eps));  dprob = grad_loss * (-t/(p+eps))/npix
 *   spcl_one_hot                    class2one_hot (new_epocher.py:84,270) into [npix][K] f32
 *   spcl_argmax_classes             `.max(1)[1]` (new_epocher.py:89,282): first maximum
 *   spcl_dice_counts                UniversalDice._intersaction / ._union on class-coded maps
 *                                   (contrastyou/meters/general_dice_meter.py:131-160): inter/union [B][C] int64, which
 *                                   the caller zeroes (integer atomics: exact and order-independent) */
int spcl_conv1x1_forward(const void* x, int dtype, size_t npix, int C, int CS, int K, const float* w, const float* b,
                         float* out, void* stream);
size_t spcl_conv1x1_bwd_workspace_bytes(int C, int K);
int spcl_conv1x1_backward(const void* x, const float* dout, int dtype, size_t npix, int C, int CS, int K, const float* w,
                          void* dx, float* dw, float* db, float* ws, void* stream);
/* The decoder's LAST BatchNorm + ReLU (unet.py:79-81 of Up_conv2) folded into the 1x1 convolution that is its only
 * consumer (unet.py:229), on both sides: y is the raw output of the last 3x3 convolution ([npix][CS] of dtype), the class map
 * is conv1x1(relu(scale y + shift)) with the activation rounded to dtype exactly as the writer would have stored it -- no
 * activation tensor.  Backward: dact = the gradient w.r.t. that activation, dw / db as spcl_conv1x1_backward, and rows
 * [spcl_conv1x1_bwd_rows(npix)][2][CS] = the partial sums of that BatchNorm's backward (sum dz, sum dz (y - mean)) in the
 * form spcl_bnrelu_backward_rows finishes: its reduction pass over (y, dact) disappears too. */
int spcl_conv1x1_forward_bn(const void* y, int dtype, size_t npix, int C, int CS, int K, const float* scale,
                            const float* shift, const float* w, const float* b, float* out, void* stream);
int spcl_conv1x1_bwd_rows(size_t npix);
int spcl_conv1x1_backward_bn(const void* y, const float* dout, int dtype, size_t npix, int C, int CS, int K,
                             const float* scale, const float* shift, const float* mean, const float* w, void* dact,
                             float* dw, float* db, float* ws, float* rows, void* stream);
int spcl_softmax_forward(const float* logits, size_t npix, int K, float* prob, void* stream);
int spcl_softmax_backward(const float* prob, const float* dprob, size_t npix, int K, float* dlogits, void* stream);
size_t spcl_kl_workspace_bytes(void);
int spcl_kl_div_forward(const float* prob, const float* target, size_t npix, int K, float eps, float* ws, float* loss,
                        void* stream);
int spcl_kl_div_backward(const float* prob, const float* target, size_t npix, int K, float eps, const float* grad_loss,
                         float* dprob, void* stream);
/* The supervised criterion of the fine-tune loop in one pass (semi_seg/epochers/new_epocher.py:268-282:
 * KL_div(logits.softmax(1), class2one_hot(target, C)) and the Dice counts of logits.max(1)[1] against target):
 * logits [B * per_sample][K] f32, labels [B * per_sample] int64 -> loss (mean over positions), dlogits_unit (the gradient
 * w.r.t. the logits for grad_loss == 1: the caller scales it), inter / union [B][K] int64 (written, not added to: they
 * need no zero fill -- the workgroups leave count rows in ws and the finishing launch adds them up in fixed order; K == the
 * number of classes).  Per pixel the arithmetic of spcl_softmax_forward / spcl_kl_div_forward / _backward /
 * spcl_softmax_backward in the same order: the same bits.  ws: spcl_kl_workspace_bytes(). */
int spcl_sup_loss_forward(const float* logits, const int64_t* labels, int B, int per_sample, int K, float eps, float* ws,
                          float* loss, float* dlogits_unit, int64_t* inter_zeroed, int64_t* union_zeroed, void* stream);
int spcl_one_hot(const int64_t* labels, size_t npix, int K, float* out, void* stream);
int spcl_argmax_classes(const float* logits, size_t npix, int K, int64_t* out, void* stream);
int spcl_dice_counts(const int64_t* pred, const int64_t* target, int B, int per_sample, int C, int64_t* inter_zeroed,
                     int64_t* union_zeroed, void* stream);

/* Surface distances of two class-coded maps (csrc/surface.hip): replaces SurfaceMeter._evalue
 * (contrastyou/meters/surface_meter.py:109-128: one host call per (slice, class)) and the three functions it dispatches to
 * (contrastyou/meters/surface_distance.py: hausdorff_distance, mod_hausdorff_distance, average_surface_distance -- medpy's
 * erosion + exact Euclidean distance transform + gather, restated from their definition).
 *   pred, target  [B][H][W] int64 class-coded maps;  report: n_report (<= 64) HOST ints, the classes to evaluate, each in [0, C)
 *   per (b, r): A = (pred[b] == report[r]), T = (target[b] == report[r]);  border(m) = the pixels of m with a 4-neighbour outside
 *   m or outside the image;  sds(A, T) = for every border pixel of A the distance sqrt((dy sy)^2 + (dx sx)^2) to the nearest
 *   border pixel of T
 *   hd   [B][n_report] f64  max(max sds(A, T), max sds(T, A))
 *   mhd  [B][n_report] f64  max(P(sds(A, T)), P(sds(T, A))), P = numpy's linear percentile at `percentile` (0 .. 100)
 *   asd  [B][n_report] f64  (mean sds(A, T) + mean sds(T, A)) / 2
 *   empty[B][n_report] u8   1 where A or T has no pixel (medpy raises there); hd, mhd and asd are NaN at those entries
 * The transform is exact (separable two-pass; integer squared distances under unit spacing, one f64 sqrt at the end), its cost
 * H W (H + W) per pair whatever the masks look like; the means are summed in a fixed order (same input, same bits).  H, W <= 1024.
 * ws: spcl_surface_workspace_bytes(B, H, W, n_report) bytes, 16-byte aligned (0 = unsupported shape).  Four launches on
 * `stream`, nothing is read back. */
size_t spcl_surface_workspace_bytes(int B, int H, int W, int n_report);
int spcl_surface_distances(const int64_t* pred, const int64_t* target, int B, int H, int W, int C, const int* report,
                           int n_report, double sy, double sx, double percentile, double* hd, double* mhd, double* asd,
                           uint8_t* empty, void* ws, size_t ws_bytes, void* stream);

/* The same metrics per SCAN (csrc/surface.hip): what SurfaceMeter._evalue (contrastyou/meters/surface_meter.py:109-128) computes
 * when `*hw` is a volume -- medpy's n-D erosion and exact n-D distance transform under `voxelspacing`
 * (contrastyou/meters/surface_distance.py:9-29), restated from their definition.
 *   pred, target  [V][D][H][W] int64 class-coded maps: V volumes of D slices, axis 1 is z
 *   per (v, r): A = (pred[v] == report[r]), T = (target[v] == report[r]);  border(m) = the voxels of m with one of their SIX
 *   neighbours (+-x, +-y, +-z) outside m or outside the volume -- in a one-slice volume every voxel of m, which is NOT the 2-D
 *   call's border of that slice;  squared distance of two voxels = ((dz sz)^2 + (dy sy)^2) + (dx sx)^2, rounded in that order
 *   (exact int32 under unit spacing);  directed sets, hd, mhd (numpy's linear percentile), asd and empty as in the 2-D call
 *   hd, mhd, asd, empty   [V][n_report]
 * D, H, W <= 1024, D H W < 2^31, spacing finite and positive, percentile in [0, 100].  The cost is D H W (D + H + W) per pair
 * whatever the masks look like.  ws: spcl_surface_3d_workspace_bytes(V, D, H, W, n_report) bytes, 16-byte aligned
 * (0 = unsupported shape).  Five launches on `stream`, nothing is read back; the same input gives the same bits. */
size_t spcl_surface_3d_workspace_bytes(int V, int D, int H, int W, int n_report);
int spcl_surface_distances_3d(const int64_t* pred, const int64_t* target, int V, int D, int H, int W, int C, const int* report,
                              int n_report, double sz, double sy, double sx, double percentile, double* hd, double* mhd,
                              double* asd, uint8_t* empty, void* ws, size_t ws_bytes, void* stream);

/* Largest connected component per foreground class and volume (csrc/components.hip): the post-processing step segmentation
 * results are usually reported after.  NOT in the reference; inference opts into it (InferenceEpocher(postprocess=...)).
 *   labels  [V][D][H][W] int64 class-coded maps, read only;  out  the same shape, may NOT alias labels (SPCL_EINVAL)
 *   classes n_classes (1 .. 15) HOST ints, distinct, each in [1, C): the classes to process; 0 is the fill value.  C >= 2.
 *   A component is a maximal set of voxels of ONE label value joined through 6-neighbour steps (+-z, +-y, +-x) inside its
 *   volume -- the neighbourhood of spcl_surface_distances_3d's borders; D = 1: 4-neighbour components per slice ([B][H][W]
 *   slice-wise is V = B, D = 1).  Diagonal contact does not connect.
 *   For every listed class the largest component by voxel count keeps its label in `out`, every other voxel of the class
 *   becomes 0.  Equal sizes: the component whose smallest linear index (z*H + y)*W + x is smallest wins -- what
 *   numpy.argmax(numpy.bincount(...)) picks on scipy.ndimage.label output (components numbered in raster order of their first
 *   voxel, first maximum).  Voxels whose label is not listed (background, unlisted classes, values outside [0, C)) are copied
 *   unchanged, form no components and join nothing.
 *   kept_size    [V][n_classes] int64  voxel count of the kept component of classes[i] (0: the class is absent)
 *   n_components [V][n_classes] int32  number of components the class had
 * D H W < 2^31.  ws: spcl_largest_component_workspace_bytes(V, D, H, W, n_classes) bytes (0 = unsupported shape), 16-byte
 * aligned: three uint32 words per voxel (union-find parents, flat roots, sizes) and one 64-bit word per (volume, class).
 * Five launches on `stream`, integer atomics only (the same input gives the same bits), nothing is read back or allocated:
 * the call can be captured.  Every argument is checked before the first launch. */
size_t spcl_largest_component_workspace_bytes(int V, int D, int H, int W, int n_classes);
int spcl_largest_component(const int64_t* labels, int V, int D, int H, int W, int C, const int* classes, int n_classes,
                           int64_t* out, int64_t* kept_size, int32_t* n_components, void* ws, size_t ws_bytes, void* stream);

/* Test-time augmentation: the merge of V views' class maps (csrc/tta.hip).  NOT in the reference; inference opts into it
 * (InferenceEpocher(tta=...)).  The entropy is the normalised one the uncertainty-aware mean teacher thresholds
 * (semi_seg/epochers/comparable.py:94-98: Entropy(softmax(.)) / log(C), eps 1e-16), here of the averaged prediction.
 *   views  a HOST array of V (1, 2, 4 or 8) device pointers to f32 class logits [N][H][W][C], 2 <= C <= 16, handed to the
 *          kernel by value -- nothing is uploaded;  ops  V HOST bytes, each < 8: bit 0 the view's input was flipped along H,
 *          bit 1 along W, bit 2 its H and W axes were swapped AFTER the flips (needs H == W, else SPCL_EINVAL).
 *   Per output pixel (n, u, v), u' = bit 0 ? H-1-u : u, v' = bit 1 ? W-1-v : v: view j is read at (n, u', v'), with bit 2 at
 *   row v', column u'; no un-flipped or transposed copy is written.  q_j = softmax of that row (exp(x - max), a true division
 *   by the sum); the V rows are added pairwise in a fixed balanced tree over the view index ((0+1), (2+3), ..., then those
 *   sums) and multiplied by the exact 1 / V: V equal rows give back their common value bit for bit.
 *   prob          [N][H][W][C] f32  the mean probability p; may not overlap a view
 *   pred          [N][H][W] int64   the first maximal class of p (the tie rule of spcl_argmax_classes)
 *   entropy       [N][H][W] f32, may be NULL   -sum_c p_c log(p_c + eps) / log(C)
 *   mean_entropy  f32 scalar        the mean of that entropy over the N H W pixels: per-workgroup double partials added in
 *                                   index order by the last workgroup (bitwise reproducible, no second launch)
 * N H W < 2^31.  ws: spcl_tta_merge_workspace_bytes(N, H, W) bytes, 8-byte aligned.  One launch and the ticket's memset on
 * `stream`, one thread per pixel, 16-byte accesses where C == 4 and every pointer is 16-byte aligned; nothing is read back or
 * allocated: the call can be captured.  Every argument is checked before the memset. */
size_t spcl_tta_merge_workspace_bytes(int N, int H, int W);
int spcl_tta_merge(const float* const* views, const uint8_t* ops, int V, int N, int C, int H, int W, float eps, float* prob,
                   int64_t* pred, float* entropy, float* mean_entropy, void* ws, size_t ws_bytes, void* stream);

/* Pre-training monitor: k-nearest neighbours, label votes, instance retrieval, alignment and uniformity (Wang & Isola 2020)
 * of N embeddings in one sweep over their N x N similarity matrix, which is never stored (csrc/embed_monitor.hip).  NOT in
 * the reference; the pre-train trainers opt into it (EmbeddingMonitor, `monitor=`).
 *   z      [N] rows of d f32, row pitch ldz >= d floats; rows need not be unit length: zh_i = z_i / max(|z_i|, 1e-12) as
 *          F.normalize (|z_i| from a double sum of squares), s_ij = zh_i . zh_j on the f32 MFMA v_mfma_f32_16x16x4_f32, the
 *          contraction in one order whatever the position of (i, j): s_ij == s_ji bitwise, equal rows give equal bits.
 *   labels [L][N] int32 (0 <= L <= 4 kinds; NULL with L == 0);  pair [N] int32: the index of the row's other view, or -1 (a
 *          value outside [0, N) counts as -1; NULL: no row has one);  1 <= k <= 32.  Labels are only compared with each
 *          other, never used as an index: the range [0, 65535] the Python binding documents is its contract, not a need
 *          of the kernel.
 *   The candidates of row i are all j != i, with exclude_pair also j != pair[i].  Candidate a beats b when s_ia > s_ib, or
 *   they are equal and a < b.
 *   knn_idx [N][k] int32, knn_sim [N][k] f32   the k best candidates in rank order; the tail of a row with fewer candidates
 *                                              is -1 / -inf
 *   pred    [L][N] int32     the majority label among the row's valid neighbours; equal counts go to the label whose
 *                            best-ranked neighbour comes first; -1 for a row without a neighbour
 *   correct [L] int32        the number of rows with pred == label (zeroed by the call's memset)
 *   pair_rank [N] int32      rows with a pair: the number of j not in {i, pair[i]} that beat pair[i]; else -1
 *   scalars [4] f64          the mean over paired rows of 2 - 2 s_i,pair (NaN without a paired row) | log of the mean over
 *                            ordered i != j of exp(-4 (1 - s_ij)) | the number of paired rows | the smallest |z_i|
 * Limits: 2 <= N <= 8192, 1 <= d <= 512; anything else is SPCL_EINVAL before any launch.  ws: 16-byte aligned,
 * spcl_embed_monitor_workspace_bytes(N, d, k) bytes (0 outside the limits).  Four launches and, with L > 0, one memset on
 * `stream`; every floating-point sum in a fixed order (bitwise reproducible), counts by integer atomics; nothing is read
 * back or allocated: the call can be captured. */
size_t spcl_embed_monitor_workspace_bytes(int N, int d, int k);
int spcl_embed_monitor(const float* z, int64_t ldz, const int32_t* labels, int L, const int32_t* pair, int N, int d, int k,
                       int exclude_pair, int32_t* knn_idx, float* knn_sim, int32_t* pred, int32_t* correct,
                       int32_t* pair_rank, double* scalars, void* ws, size_t ws_bytes, void* stream);

/* The same call with groups (ABI 30): group [N] int32, or NULL.  With group[i] >= 0 the candidates of row i also leave out
 * every j with group[j] == group[i] -- the cells of one scan are near-duplicates of each other, and a vote among them
 * measures nothing (DenseEmbeddingMonitor, `dense_monitor=`).  A negative id means ungrouped: nothing more is left out for
 * that row.  The tie rule, uniformity, alignment, pair_rank and the smallest norm are those of spcl_embed_monitor: groups
 * enter the neighbour lists (knn_idx, knn_sim, pred, correct) and nothing else.  One code path: spcl_embed_monitor IS this call
 * with group == NULL, bit for bit.  Limits, workspace (spcl_embed_monitor_workspace_bytes), launches, reproducibility and
 * capture as above; the group ids are read by the sweep where they lie, one per candidate and tile. */
int spcl_embed_monitor_grouped(const float* z, int64_t ldz, const int32_t* labels, int L, const int32_t* pair,
                               const int32_t* group, int N, int d, int k, int exclude_pair, int32_t* knn_idx, float* knn_sim,
                               int32_t* pred, int32_t* correct, int32_t* pair_rank, double* scalars, void* ws, size_t ws_bytes,
                               void* stream);

/* The majority class of every cell of an adaptive pool (ABI 30): the label of a row of DenseProjectionHead's output.
 *   labels     [N][H][W] uint8 class codes below C (2 <= C <= 16); a value >= C is counted for no class
 *   (sh, sw)   the output grid, 1 <= sh <= H, 1 <= sw <= W.  Cell (u, v) covers rows floor(u H / sh) .. ceil((u + 1) H / sh) - 1
 *              and the same rule for columns: the windows of nn.AdaptiveAvgPool2d, which overlap when the size does not divide
 *   cell_label [N][sh][sw] int32   the class with the largest integer count in the window, equal counts to the lower class;
 *                                  -1 for a window that holds only values >= C
 *   purity     [N][sh][sw] f32, may be NULL   float(count) / float(window size), correctly rounded; 0 with label -1
 * H, W <= 32768, N sh sw < 2^31 - 4; anything else is SPCL_EINVAL before the launch.  One launch on `stream`, one wave per
 * cell, integer counts from ballots (no atomics, no floating-point sum): the same bits every run; nothing is read back or
 * allocated: the call can be captured. */
int spcl_cell_majority(const uint8_t* labels, int N, int H, int W, int C, int sh, int sw, int32_t* cell_label, float* purity,
                       void* stream);

/* Decoder data movement (NHWC, CS a multiple of 16): nn.Upsample(scale_factor=2) of `_UpConv` (unet.py:89) and its
 * backward (H, W = the low-resolution size in both calls), torch.cat((skip, up), dim=1) (unet.py:194-224) and its
 * backward (split).  Channel runs must be multiples of 16 bytes. */
int spcl_upsample2x_forward(const void* x, void* y, int dtype, int N, int H, int W, int CS, void* stream);
int spcl_upsample2x_backward(const void* dy, void* dx, int dtype, int N, int H, int W, int CS, void* stream);
int spcl_concat2_channels(const void* a, const void* b, void* out, int elem_size, size_t npix, int CA, int CB,
                          void* stream);
int spcl_split2_channels(const void* in, void* a, void* b, int elem_size, size_t npix, int CA, int CB, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Optimizer step of the pre-train iteration (contrastyou/trainer/base.py:62 builds RAdam from the un-vendored
 * deepclustering2; the build follows torch.optim.RAdam(decoupled_weight_decay=False)) on ONE
 * flat fp32 parameter:  g' = g + wd p;  m = lerp(m, g', 1-b1);  v = b2 v + (1-b2) g'^2;  t = ++step;
 *   rho_t = rho_inf - 2 t b2^t/(1-b2^t);  p -= lr m/(1-b1^t) * (rho_t > 5 ? rect(rho_t) sqrt(1-b2^t)/(sqrt(v)+eps) : 1).
 * step (int64) and lr (float) live in device memory so that a captured hipGraph replays with an advancing step
 * count and a host-updated learning rate; coef: 4 floats of device scratch.  All buffers 16-byte aligned. */
int spcl_radam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, int64_t* step,
                    const float* lr, double beta1, double beta2, double eps, double weight_decay, float* coef,
                    void* stream);
/* the same, and the step's meter updates (spcl_accumulate_scalars' k <= 8 pairs) ride in its coefficient launch: one
 * launch less per training step.  k == 0: exactly spcl_radam_step. */
int spcl_radam_step_scalars(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, int64_t* step,
                            const float* lr, double beta1, double beta2, double eps, double weight_decay, float* coef,
                            int k, const void* const* src, void* const* dst, const float* count, void* stream);
/* the same on grad_scale * grad (0 < grad_scale <= 1): the data-parallel MEAN of the flat gradient bucket is its RCCL sum
 * times 1 / world, and that factor is applied while the bucket streams through the optimizer instead of by a separate
 * pass over it (the reference is single-process; its seam for N ranks is semi_seg/main_infonce.py:35,39).
 * grad_scale == 1: bit-identical to spcl_radam_step_scalars. */
int spcl_radam_step_scaled(float* param, const float* grad, double grad_scale, float* exp_avg, float* exp_avg_sq, size_t n,
                           int64_t* step, const float* lr, double beta1, double beta2, double eps, double weight_decay,
                           float* coef, int k, const void* const* src, void* const* dst, const float* count, void* stream);
/* the same WITHOUT the coefficient launch: coef[0..2] = { lr / (1 - b1^t), rho_t > 5 ? rect(rho_t) sqrt(1 - b2^t) : 0,
 * rho_t > 5 } and coef[3] = t were computed by the caller on the host (the formulas above, in double) and are already in
 * device memory -- a step replayed from a hipGraph uploads a few host-written bytes per replay anyway (labels, flip flags:
 * spcl_stage_bytes / spcl_flip_pair_stage), the four floats travel with them.  The launch records t in *step (so that the
 * counter, which spcl_radam_step reads, stays the state_dict's truth) and performs the k meter updates. */
int spcl_radam_apply_staged(float* param, const float* grad, double grad_scale, float* exp_avg, float* exp_avg_sq, size_t n,
                            int64_t* step, const float* coef, double beta1, double beta2, double eps, double weight_decay,
                            int k, const void* const* src, void* const* dst, const float* count, void* stream);

/* The other optimizers a configuration may name (contrastyou/trainer/base.py:60-69 builds optim.__dict__[config["Optim"]["name"]]:
 * Adam, AdamW and SGD are as legal as RAdam), built like the RAdam step above: ONE flat fp32 parameter, step (int64) and lr
 * (float) in device memory, coef = 4 floats of device scratch, grad_scale in (0, 1] applied as the gradient streams
 * (grad_scale == 1: bit-identical to not scaling), the k <= 8 meter updates of spcl_accumulate_scalars in the same launches.
 *
 * Adam / AdamW (torch.optim.Adam / AdamW, single-tensor path, amsgrad = maximize = false):
 *   decoupled == 0:  g' = grad_scale g + wd p;      decoupled == 1:  p *= (1 - lr wd),  g' = grad_scale g;
 *   m = lerp(m, g', 1-b1);  v = b2 v + (1-b2) g'^2;  t = ++step;  p -= (lr / (1-b1^t)) m / (sqrt(v) / sqrt(1-b2^t) + eps).
 * 28 bytes per element.  spcl_adam_step_scaled: a one-wave coefficient launch (advances *step, reads *lr, writes coef, performs
 * the meter updates), then the streaming launch.  spcl_adam_apply_staged: NO coefficient launch -- coef[0..3] =
 * { lr / (1-b1^t), sqrt(1-b2^t), (float)(1 - lr wd), t } were computed by the caller on the host (in double, powers by
 * repeated squaring, lr as the float the device holds: the bits of the coefficient launch) and are already in device memory;
 * the launch records t in *step and performs the meter updates. */
int spcl_adam_step_scaled(float* param, const float* grad, double grad_scale, float* exp_avg, float* exp_avg_sq, size_t n,
                          int64_t* step, const float* lr, double beta1, double beta2, double eps, double weight_decay,
                          int decoupled, float* coef, int k, const void* const* src, void* const* dst, const float* count,
                          void* stream);
int spcl_adam_apply_staged(float* param, const float* grad, double grad_scale, float* exp_avg, float* exp_avg_sq, size_t n,
                           int64_t* step, const float* coef, double beta1, double beta2, double eps, double weight_decay,
                           int decoupled, int k, const void* const* src, void* const* dst, const float* count, void* stream);
/* SGD (torch.optim.SGD; contrastyou/trainer/base.py:60-69 as above):  g' = grad_scale g + wd p;  with momentum != 0:
 *   buf = g' at t == 1, buf = momentum buf + (1 - dampening) g' afterwards;  g' = nesterov ? g' + momentum buf : buf;
 *   p -= lr g'.   Whether a step is the first is read from DEVICE memory (the counter the coefficient launch advanced, or the
 * staged coef[3]), never decided by the host: a replayed hipGraph must not repeat step 1.  momentum_buffer is NULL if and
 * only if momentum == 0; that path moves 12 bytes per element and touches no buffer, with momentum it moves 20.
 * coef = { lr, 0, 0, t }.  Nesterov needs momentum > 0 and dampening == 0. */
int spcl_sgd_step_scaled(float* param, const float* grad, double grad_scale, float* momentum_buffer, size_t n, int64_t* step,
                         const float* lr, double momentum, double dampening, double weight_decay, int nesterov, float* coef,
                         int k, const void* const* src, void* const* dst, const float* count, void* stream);
int spcl_sgd_apply_staged(float* param, const float* grad, double grad_scale, float* momentum_buffer, size_t n, int64_t* step,
                          const float* coef, double momentum, double dampening, double weight_decay, int nesterov, int k,
                          const void* const* src, void* const* dst, const float* count, void* stream);

/* Running means of the host-side meters (contrastyou/meters/averagemeter.py via MeterInterface) kept on the device:
 * for i < k (k <= 8):  dst[i][0] += count[i] * src[i][0];  dst[i][1] += count[i].  src / dst / count are HOST arrays
 * (of device pointers / floats) read at call time: ONE launch for all of a step's meter updates. */
int spcl_accumulate_scalars(int k, const void* const* src, void* const* dst, const float* count, void* stream);

/* Per-step HOST inputs of a hipGraph-captured step (the label vector `torch.Tensor(target)` of
 * contrastyou/losses/contrast_loss3.py:133-139, the per-sample flip decisions of semi_seg/epochers/new_pretrain.py:57-58):
 * nbytes (multiple of 4) bytes of host memory are copied to the persistent device block dst, in stream order.  The bytes
 * travel as kernel arguments (read at call time: host_src may be reused as soon as the call returns), 3 584 per launch. */
int spcl_stage_bytes(void* dst, const void* host_src, size_t nbytes, void* stream);
/* two device-to-device copies in one launch (the labelled batch into the captured fine-tune step's persistent input buffers,
 * semi_seg/epochers/new_epocher.py:260-266 hands the step a fresh image / target pair every iteration): sizes and addresses
 * multiples of 16 bytes */
int spcl_copy_pair(void* dst_a, const void* src_a, size_t bytes_a, void* dst_b, const void* src_b, size_t bytes_b,
                   void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Pre-train augmentation on device (replaces the PIL recipe of semi_seg/augment.py:6-22
 * `ACDCStrongTransforms.pretrain`: RandomRotation -> RandomVerticalFlip -> RandomHorizontalFlip -> RandomCrop ->
 * ColorJitter(brightness, contrast) -> ToTensor): one OH x OW view per parameter row, gathered from the device-resident
 * slice store src [S][HS][WS] f32 in [0,1].  params: device int32 [nviews][8] = {slice, cos * 65536, sin * 65536 (rounded;
 * rotation counter-clockwise about the image centre, nearest sampling, 0 outside), flags (1 horizontal flip, 2 vertical
 * flip, 4 contrast before brightness), crop top, crop left, brightness factor (f32 bits), contrast factor (f32 bits)}.
 * out [nviews][OH][OW] f32.  Geometry is integer arithmetic: bit-exact against oracle.augment_view. */
int spcl_augment_views(const float* src, int S, int HS, int WS, const int* params, int nviews, float* out, int OH,
                       int OW, void* stream);
/* The same recipe in PIL's own arithmetic -- what semi_seg/augment.py:6-22 computes through torchvision on 8-bit slices:
 * Image.rotate(angle, NEAREST) (Geometry.c affine_fixed: 16.16 coefficients a0..a5 rounded on the host as PIL rounds them),
 * transposes, crop, ImageEnhance.Brightness / .Contrast (Image.blend on 8-bit values, truncating; Contrast against
 * int(mean + 0.5)), ToTensor (/ 255).  src holds 8-bit grey levels as k / 255.  params: device int32 [nviews][12] =
 * {slice, a0, a1, a2, a3, a4, a5, flags (1 hflip, 2 vflip, 4 contrast before brightness), crop top, crop left, brightness
 * (f32 bits), contrast (f32 bits)}.  Bit-exact against PIL itself: tests/golden/g9_augment.npz (tools/gen_golden.py augment),
 * oracle.augment_view_pil. */
int spcl_augment_views_pil(const float* src, int S, int HS, int WS, const int* params, int nviews, float* out, int OH,
                           int OW, void* stream);
/* The pixel-wise (1x1-convolution) MLP of the dense projector -- contrastyou/projectors/heads.py:28-39,96-120:
 * Conv2d(C, hid, 1) -> LeakyReLU(0.01) -> Conv2d(hid, out, 1) on every pixel of a decoder feature map -- as tiled
 * matrix products over the M = N*H*W pixel rows on the exact-f32 matrix instruction (round 6; until then the rows went through the
 * global projector's 64-row kernels: 158 ms per training step at Up_conv3, 630 ms at Up_conv2).  Row-major operands, f32
 * accumulation; tensors with a dtype argument are f32 or bf16 rows (a channels-last map is read in place through its pitch):
 *   forward          y[M][N]  = act(x)[M][K] W[N][K]^T + bias[N]      act = LeakyReLU(0.01) when leaky_in (x is then a saved f32
 *                                                                      pre-activation); y f32
 *   forward_act      h[M][N]  = LeakyReLU(x[M][K] W[N][K]^T + bias[N])   h of h_dtype.  h carries the pre-activation's sign: it
 *                                                                      stands in for `pre` below
 *   backward_input   dx[M][K] = (g[M][N] W[N][K]) * (pre ? LeakyReLU'(pre[M][K]) : 1)     (with pre: g is f32)
 *   backward_weight  dW[N][K] = sum_m g[m][N] act(x)[m][K],  db[N] = sum_m g[m][N]  (db may be NULL): slabs of rows folded in
 *                    index order (bit-deterministic); ws of spcl_rows_linear_backward_weight_workspace_bytes(M, N, K).
 *   spcl_adaptive_avgpool2d_backward_act: dx = unpool(dout [N][OH][OW][C] f32) * LeakyReLU'(.) with act = LeakyReLU(pre)
 *                    [N][H][W][C] given instead of pre; act and dx of `dtype`; C % 4 == 0.
 * The dense projector's pooled-hidden form (functional._PixelMlpPooledFn): adaptive average pooling commutes with the linear
 * second layer, which then runs on the pooled rows only; the hidden activation and its gradient are stored in the feature
 * map's dtype.  K, N and the row pitches are multiples of 4. */
int spcl_rows_linear_forward(const void* x, int x_dtype, long ldx, int leaky_in, const float* W, const float* bias, int M,
                             int K, int N, float* y, void* stream);
int spcl_rows_linear_forward_act(const void* x, int x_dtype, long ldx, const float* W, const float* bias, int M, int K, int N,
                                 void* h, int h_dtype, void* stream);
int spcl_adaptive_avgpool2d_backward_act(const float* dout, const void* act, int dtype, int N, int H, int W, int C, int OH,
                                         int OW, void* dx, void* stream);
int spcl_rows_linear_backward_input(const void* g, int g_dtype, const float* W, const float* pre, int M, int N, int K, void* dx,
                                    int dx_dtype, long lddx, void* stream);
size_t spcl_rows_linear_backward_weight_workspace_bytes(int M, int N, int K);
int spcl_rows_linear_backward_weight(const void* g, int g_dtype, const void* x, int x_dtype, long ldx, int leaky_in, int M, int N,
                                     int K, float* ws, size_t ws_bytes, float* dW, float* db, void* stream);
/* The reference's other PIL recipes, and the interpolation its wrapper really selects (semi_seg/augment.py:23-37,54-75;
 * contrastyou/augment/synchronize.py:95-103: BILINEAR on images, NEAREST on targets): params[v][28] =
 *   [0] slice [1] flags (1 hflip, 2 vflip, 4 contrast first, 8 bilinear image rotation, 16 crop first = the rotation turns the
 *   crop about its centre) [2] top [3] left [4] pad [5] brightness [6] contrast (f32 bits) [8..13] PIL's 16.16 nearest
 *   coefficients [14..25] the six doubles of PIL's rotation matrix -- of the image the rotation acts on (slice or crop).
 * labels / label_out (optional, together): the slice's u8 label map through the same geometry with NEAREST -> int64. */
int spcl_augment_views_recipe(const float* src, const unsigned char* labels, int S, int HS, int WS, const int* params,
                              int nviews, float* out, long long* label_out, int OH, int OW, int max_pad, void* stream);
/* The same views (bit for bit) from a grid that fills the chip: spcl_augment_views_recipe runs ONE workgroup per view, which
 * samples its pixels twice (ImageEnhance.Contrast needs the view's mean first) -- 180 us for the 60 views of a pre-train batch
 * on a quarter of the CUs.  Here up to 64 workgroups per view sample a chunk each once, park the 8-bit levels and their integer
 * partial sum in `workspace` (spcl_augment_views_recipe_workspace_bytes, 8-byte aligned, contents irrelevant on entry), and
 * a second launch finishes the pixels.  What semi_seg/data/augment.py RecipeViews calls (ABI 7). */
size_t spcl_augment_views_recipe_workspace_bytes(int nviews, int OH, int OW);
int spcl_augment_views_recipe_ws(const float* src, const unsigned char* labels, int S, int HS, int WS, const int* params,
                                 int nviews, float* out, long long* label_out, int OH, int OW, int max_pad, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* Image.resize((OW, OH), BILINEAR) of every slice of a store of 8-bit levels (k / 255) -- torchvision Resize,
 * semi_seg/augment.py:56,71,79 -- with the coefficient rows of Resample.c precomputed by the caller per axis
 * (bounds[out][2] = first tap, tap count; kk[out][ksize]: 22 fractional bits); tmp: [S][HS][OW] floats. */
int spcl_resize_bilinear_pil(const float* src, int S, int HS, int WS, const int* bounds_x, const int* kk_x, int ksize_x,
                             const int* bounds_y, const int* kk_y, int ksize_y, float* tmp, float* out, int OH, int OW,
                             void* stream);
/* Image.resize((OW, OH), NEAREST) of every slice of a u8 label store [S][HS][WS] -> out [S][OH][OW]: what Resize(224)
 * (semi_seg/augment.py:57,74,86) does to a TARGET, for which the reference's wrapper swaps the common transform's
 * interpolation to NEAREST (contrastyou/augment/synchronize.py:105-107).  out[s][y][x] = src[s][ytab[y]][xtab[x]]; the
 * caller precomputes one int32 source-index table per axis on the host by PIL's own rule -- the ACCUMULATED form
 * xo = scale / 2; tab[x] = (int)xo; xo += scale with scale = n_in / n_out in double, NOT (x + 0.5) * scale, which differs
 * from PIL in places (semi_seg/data/augment.py nearest_resize_table).  The caller keeps every entry inside [0, n_in); as a
 * defence the kernel clamps an entry into that range (a wrong table then gives a wrong pixel of the same slice, never a
 * read outside the store).  One thread writes 16 neighbouring output bytes of a row with one 128-bit store where
 * OW % 16 == 0 and `out` is 16-byte aligned, 4 bytes with one 32-bit store where OW % 4 == 0 and `out` is 4-byte aligned,
 * single bytes otherwise; src needs no alignment.  SPCL_EINVAL: a null pointer, a non-positive shape,
 * S * OH * OW >= 2^31.  (ABI 24) */
int spcl_resize_nearest_pil(const unsigned char* src, int S, int HS, int WS, const int* xtab /*[OW]*/,
                            const int* ytab /*[OH]*/, unsigned char* out, int OH, int OW, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Per-sample random flips of an NCHW batch (TensorRandomFlip(axis=[1,2], threshold=0.8), new_epocher.py:112, applied
 * per sample in new_pretrain.py:57-58): out[n] = x[n] flipped along H when flags[n] & 1 and along W when flags[n] & 2.
 * flags: device uint8[N] (the host draws the decisions from python `random`, as the reference does).  x != out. */
int spcl_flip_batch(const void* x, void* out, int elem_size, int N, int C, int H, int W, const uint8_t* flags,
                    void* stream);
/* The pre-train step's input pair in one launch: out [2N][C][H][W] = [ first | flip(second, flags) ] -- the per-sample
 * flip of view 2 and the torch.cat of semi_seg/epochers/new_pretrain.py:57-58,93. */
int spcl_flip_pair(const void* first, const void* second, void* out, int elem_size, int N, int C, int H, int W,
                   const uint8_t* flags, void* stream);
/* the same launch also performs spcl_stage_bytes(stage_dst, host_src, nbytes) and takes the N flag bytes from
 * host_src + flag_off (kernel arguments: nbytes <= 3 584): the two eager launches in front of a replayed step are one. */
int spcl_flip_pair_stage(const void* first, const void* second, void* out, int elem_size, int N, int C, int H, int W,
                         void* stage_dst, const void* host_src, size_t nbytes, size_t flag_off, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Built-in kernel timer (bench.py's live roofline measurement): spcl_profile_enable(1) clears the log and makes every
 * kernel launch of the library record HIP events on its launch stream; spcl_profile_get returns launch i's kernel
 * symbol (as rocprofv3 prints it), its duration and the algorithmic bytes / FLOPs its entry point declared (0 when
 * none).  Not usable inside a hipGraph capture.  spcl_profile_enable(0) clears the log and switches it off. */
int spcl_profile_enable(int on);
int spcl_profile_count(void);
int spcl_profile_get(int i, char* name, int name_cap, float* usec, double* bytes, double* flops);

/* ---------------------------------------------------------------- BatchNorm sums as fixed-point accumulator blocks --------
 * Replaces the finalize launches between a train-mode nn.BatchNorm2d's producer and consumer (semi_seg/arch/unet.py:73,76 and
 * its autograd backward): the producing kernel's epilogue ADDS its tile's sums to a block of 64-bit fixed-point words
 * (integer atomics: exact, order-free, bit-for-bit deterministic), the next launch derives the coefficients in its prologue.
 * A block is spcl_bn_acc_elems(CS) int64 words, ZEROED by the caller before the producer launch (one memset per step for all
 * blocks of a step).  Forward blocks hold sum x / sum x^2, backward blocks sum dz / sum dz (y - mean).  csrc/bn_acc.hpp has
 * the format.  Offered for bf16 layers the specialised 14-column convolution kernels take, with at most 4096 tiles, CS <= 256. */
typedef struct spcl_bn_acc {
  long long* acc;                 /* the forward block of this BatchNorm */
  const float* gamma;             /* [C] */
  const float* beta;              /* [C] */
  float* running_mean;            /* [C] or NULL (no update) */
  float* running_var;             /* [C] or NULL */
  long long* num_batches_tracked; /* or NULL */
  float* st;                      /* [4][CS] mean, invstd, scale, shift: WRITTEN by the consuming launch's first workgroup */
  float momentum, eps;
  float count;                    /* values per channel: N * H * W */
  int C, CS;
} spcl_bn_acc;
size_t spcl_bn_acc_elems(int CS);
/* can spcl_conv3x3_forward_acc run this layer with its input read as it is (in_kind 0), through a BatchNorm + ReLU whose
 * coefficients are derived from a block (1) or come as arrays (2), and (with_stats_acc) its output statistics added to a block? */
int spcl_conv_bn_acc_supported(int dtype, int N, int H, int W, int CinK, int CoutS, int in_kind, int with_stats_acc);
/* spcl_conv3x3_forward with blocks on either side: in_bn != NULL -> the input is the previous convolution's RAW output and
 * relu(scale x + shift) of its BatchNorm is applied by the loader, scale / shift derived from in_bn->acc (no spcl_bn_finalize);
 * in_bn == NULL: scale / shift from in_scale / in_shift when given, else the input is read as it is;
 * stats_acc != NULL -> the output's statistics are added to that block; else stats_rows (per-tile rows, or NULL). */
int spcl_conv3x3_forward_acc(const void* x, int dtype, int N, int H, int W, int CinK, int CoutS, const void* w_packed,
                             const spcl_bn_acc* in_bn, const float* in_scale, const float* in_shift, void* y,
                             long long* stats_acc, float* stats_rows, void* stream);
/* spcl_bn_finalize + spcl_bnrelu_pool_forward in one launch (coefficients derived in the prologue) */
int spcl_bnrelu_pool_forward_acc(const void* y, int dtype, int N, int H, int W, int CS, const spcl_bn_acc* bn, void* act_out,
                                 void* pool_out, void* stream);
/* BN-apply + ReLU of a block's last convolution (unet.py:76-77) with the activation's global average per (image, channel) as
 * a side output: gap_out[n][c] = mean over the pixels of act_out as stored -- the AdaptiveAvgPool2d((1, 1)) at the head of
 * the projector (contrastyou/projectors/heads.py:78-92, nn.py:56-58) then has nothing to read back (spcl_proj_forward with
 * feat == NULL takes the rows).  bn == NULL: coefficients from scale / shift; else derived from the accumulator block as in
 * spcl_bnrelu_pool_forward_acc (scale / shift unused).  spcl_bnrelu_gap_supported: small maps (H W <= 4096), CS <= 256. */
int spcl_bnrelu_gap_supported(int dtype, int H, int W, int C, int CS);
int spcl_bnrelu_gap_forward(const void* y, int dtype, int N, int H, int W, int C, int CS, const float* scale,
                            const float* shift, const spcl_bn_acc* bn, void* act_out, float* gap_out, void* stream);
/* spcl_conv3x3_dgrad_bnstats / _poolstats with the BatchNorm-backward sums added to a block instead of written as rows */
int spcl_conv_dgrad_bnstats_acc_supported(int dtype, int N, int H, int W, int CinK, int CoutS);
int spcl_conv3x3_dgrad_bnstats_acc(const void* dy, int dtype, int N, int H, int W, int CinK, int CoutS, const void* w_packed,
                                   void* g, const void* y2, const float* scale2, const float* shift2, const float* mean2,
                                   long long* acc, void* stream);
int spcl_conv_dgrad_poolstats_acc_supported(int dtype, int N, int H, int W, int CinK, int CoutS, int H2, int W2);
int spcl_conv3x3_dgrad_poolstats_acc(const void* dy, int dtype, int N, int H, int W, int CinK, int CoutS, const void* w_packed,
                                     void* g, const void* y2, int H2, int W2, const float* scale2, const float* shift2,
                                     const float* mean2, long long* acc, void* stream);
/* The pooled boundary through the WINDOW-MAXIMUM tensor.  Forward: spcl_bnrelu_pool_forward (bn == NULL: scale / shift) or
 * spcl_bnrelu_pool_forward_acc (bn != NULL) with one more output, ymax_out [N][H/2][W/2][CS]: per complete 2x2 window and
 * channel the RAW y of the window's first maximum of fma(scale, y, shift) in scan order (the position max_pool2d's gradient
 * goes to); act_out may be NULL, pool_out and ymax_out may not.  Backward: spcl_conv3x3_dgrad_poolstats(_acc) with that
 * tensor, ymax [N][H][W][CoutS] at the dgrad's own resolution, in place of (y2, H2, W2): a quarter of the bytes, one load
 * and one fma per window where the other form has four and a selection -- g, the rows and the block's words are the same
 * bits.  Ask the _supported queries first (they imply the _poolstats ones for H2 = 2 H, W2 = 2 W). */
int spcl_bnrelu_pool_forward_ymax(const void* y, int dtype, int N, int H, int W, int CS, const float* scale,
                                  const float* shift, const spcl_bn_acc* bn, void* act_out, void* pool_out, void* ymax_out,
                                  void* stream);
int spcl_conv_dgrad_poolmax_supported(int dtype, int N, int H, int W, int CinK, int CoutS);
int spcl_conv3x3_dgrad_poolmax(const void* dy, int dtype, int N, int H, int W, int CinK, int CoutS, const void* w_packed,
                               void* g, const void* ymax, const float* scale2, const float* shift2, const float* mean2,
                               float* rows2, void* stream);
int spcl_conv_dgrad_poolmax_acc_supported(int dtype, int N, int H, int W, int CinK, int CoutS);
int spcl_conv3x3_dgrad_poolmax_acc(const void* dy, int dtype, int N, int H, int W, int CinK, int CoutS, const void* w_packed,
                                   void* g, const void* ymax, const float* scale2, const float* shift2, const float* mean2,
                                   long long* acc, void* stream);
/* the BatchNorm + ReLU (+ max-pool) backward's apply pass with A, B derived from a backward block in its prologue (no reduction
 * pass where a dgrad filled the block, no finalize launch): exactly one of dact [N][H][W][CS], dpool [N][H/2][W/2][CS]
 * (block already filled) or dact_nc [N][CS] (one value per image and channel: this call's reduction pass fills the block).
 * st4 = the forward's [4][CS].  dgamma / dbeta [C] are written by the apply launch. */
int spcl_bnrelu_backward_acc(const void* y, const void* dact, const void* dpool, const void* dact_nc, int dtype, int N, int H,
                             int W, int C, int CS, const float* st4, int training, long long* acc, float* dgamma, float* dbeta,
                             void* dy, void* stream);
/* ... and for a gradient that did NOT come with its sums -- an activation with several consumers (the decoder's skip
 * connections, unet.py:193-230), the up-convolutions (:85-97), a gradient that arrives as a channel slice of a wider tensor
 * (dact_stride > 0 elements per pixel) or at twice the resolution (d_up [N][2H][2W][CS] non-NULL: dact is then scratch the call
 * fills with the 2 x 2 sums) --: the reduction pass ADDS its sums to the zeroed block `acc`, the apply pass derives the
 * coefficients from it; two launches, no finalize launch between them.  Exactly spcl_bnrelu_pool_backward(_strided) /
 * spcl_bnrelu_backward_up2's results (the sums in another, fixed-point order).  CS <= 256. */
int spcl_bnrelu_backward_fill_acc(const void* y, void* dact, int dact_stride, const void* dpool, const void* d_up, int dtype,
                                  int N, int H, int W, int C, int CS, const float* st4, int training, long long* acc,
                                  float* dgamma, float* dbeta, void* dy, void* stream);
/* ... and for a gradient whose sums came as per-tile rows [nrows][2][CS] (sum dz, sum dz (y - mean): what the dgrad epilogues
 * leave where a layer has more tiles than the blocks take adds from): one small launch adds the rows to the zeroed block, the
 * apply pass (exactly one of dact / dpool) derives its coefficients: spcl_bnrelu_backward_rows / spcl_bnrelu_pool_backward_rows
 * without their finalize launch. */
int spcl_bnrelu_backward_rows_acc(const void* y, const void* dact, const void* dpool, const float* rows, int nrows, int dtype,
                                  int N, int H, int W, int C, int CS, const float* st4, int training, long long* acc,
                                  float* dgamma, float* dbeta, void* dy, void* stream);

/* IIC criteria of the UDA-IIC baseline (csrc/iic.hip; semi_seg/hooks/discretemi.py, contrastyou/losses/iic_loss.py).
 * lx / ly: cluster-head logits as pixel rows [N][H][W][ld] f32, subhead s in columns s*K .. s*K+K-1 (2 <= K <= 32); the grouped
 * softmax is applied as the rows are read.  flags_x: uint8 [N] (bit 0 flips H, bit 1 flips W) applied to X by indexing, or NULL.
 *   spcl_iic_joint_forward: J[s][dy][dx][i][j] = sum_{n,u,v} PX[n,s,i,u+dy-p,v+dx-p] PY[n,s,j,u,v] (PX = 0 outside the image),
 *                    0 <= p <= 7, as 32.32 fixed-point words in jacc (spcl_iic_joint_workspace_bytes; zeroed by the call):
 *                    bitwise deterministic.
 *   spcl_iic_loss:   one launch for all subheads; reads the joint from jacc or from an f32 jf32 [S][T][T][K][K] (exactly one).
 *                    dense = 1: IIDSegmentationLoss (global min-shift of each subhead, per-displacement normalisation,
 *                    symmetrisation, marginals, eps 1e-16, / T^2); dense = 0: IIDLoss (T = 1, eps 1e-10).  loss = scale *
 *                    sum over subheads; dj = d loss / d J; j_out (optional, with jacc) = J in f32; nan_flag (optional) =
 *                    1 when the dense loss is NaN, else 0.  ws: spcl_iic_loss_workspace_bytes(S, T).
 *   spcl_iic_joint_backward: d(logits) of X (at its flipped rows) and Y from dj (times *gscale when non-NULL); the
 *                    columns s*K + k of dlx / dly are written, the others are left alone.
 *   spcl_consistency_softmax_mse: weight * mean((softmax(flip(a)) - softmax(b))^2) over [N][H][W][C] f32 class maps (C <= 16),
 *                    db = its gradient w.r.t. b for a unit upstream gradient (a gets none); ws:
 *                    spcl_consistency_workspace_bytes(N, H, W).  The loss is a fixed-order sum: deterministic.  It is
 *                    spcl_mt_softmax_mse with teacher_mode = 1 (the same launch), and like it refuses N*H*W >= 2^31 (such
 *                    sizes used to be accepted and overflowed the workgroup count). */
size_t spcl_iic_joint_workspace_bytes(int S, int K, int pad);
int spcl_iic_joint_forward(const float* lx, const float* ly, long ld, int N, int H, int W, int S, int K, int pad,
                           const uint8_t* flags_x, long long* jacc, void* stream);
size_t spcl_iic_loss_workspace_bytes(int S, int T);
int spcl_iic_loss(const long long* jacc, const float* jf32, int S, int K, int T, int dense, float scale, float* j_out,
                  float* loss, float* dj, int* nan_flag, void* ws, size_t ws_bytes, void* stream);
int spcl_iic_joint_backward(const float* lx, const float* ly, long ld, int N, int H, int W, int S, int K, int pad,
                            const uint8_t* flags_x, const float* dj, const float* gscale, float* dlx, float* dly, void* stream);
size_t spcl_consistency_workspace_bytes(int N, int H, int W);
int spcl_consistency_softmax_mse(const float* a, const float* b, int N, int C, int H, int W, const uint8_t* flags_a,
                                 float weight, float* loss, float* db, void* ws, size_t ws_bytes, void* stream);

/* Patch-wise IIC segmentation criterion of the MIDL baseline (csrc/iic_patch.hip).  Replaces IIDSegmentationSmallPathLoss and
 * patch_generator (contrastyou/losses/iic_loss.py:103-128, :154-162) as semi_seg/epochers/comparable.py:222 calls them on the
 * segmentation output: there one F.conv2d and about twenty tensor ops per patch.
 * lx / ly: class logits [N][H][W][C] f32 (2 <= C <= 16); PX = softmax(lx), PY = softmax(flip(ly)), flags_y: uint8 [N] (bit 0
 * flips H, bit 1 flips W) applied to Y by indexing, or NULL.  0 <= pad <= 7, patch >= 2.  The patch starts along an axis of
 * length h are 0, s, 2s, ... < h - patch and then max(h - patch, 0), s = patch / 2; the nP patches are all (row start, column
 * start) pairs in row-major order, each clipped to the map.  Per patch P
 *   J_P[dy][dx][i][j] = sum_{n, (u,v) in P} PX[n,i,u+dy-pad,v+dx-pad] PY[n,j,u,v]   (PX = 0 outside the PATCH)
 * and loss_P = IIDSegmentationLoss of that joint (iic_loss.py:77-97: min-shift over the whole joint, per-displacement
 * normalisation, symmetrisation, marginals, eps 1e-16, / T^2; lamda = 1), in float64 from 32.32 fixed-point joints.
 *   spcl_iic_patch_plan:     argument check without a launch; gives the patch count, the workspace size in bytes and the
 *                    number of f32 elements of dj (each output pointer may be NULL).
 *   spcl_iic_patch_forward:  loss[0] = scale * mean_P loss_P; patch_loss (nullable, [nP]) = the loss_P themselves (not scaled);
 *                    nan_flag[0] = 1 when any loss_P is NaN (iic_loss.py:123), else 0; dj = d loss / d J_P of every patch, in
 *                    the layout spcl_iic_patch_backward reads.  ws is zeroed by the call.  Bitwise deterministic.
 *   spcl_iic_patch_backward: dlx = d loss / d lx (times *gscale when non-NULL); dly, when non-NULL, the same for ly, written
 *                    at Y's unflipped position.  A pixel gathers from every patch that covers it: each element is written
 *                    exactly once, no atomics. */
int spcl_iic_patch_plan(int N, int C, int H, int W, int pad, int patch, int* num_patches, size_t* ws_bytes, size_t* dj_elems);
int spcl_iic_patch_forward(const float* lx, const float* ly, int N, int C, int H, int W, int pad, int patch,
                           const uint8_t* flags_y, float scale, float* loss, float* patch_loss, int* nan_flag, float* dj,
                           void* ws, size_t ws_bytes, void* stream);
int spcl_iic_patch_backward(const float* lx, const float* ly, int N, int C, int H, int W, int pad, int patch,
                            const uint8_t* flags_y, const float* dj, const float* gscale, float* dlx, float* dly, void* stream);

/* The same criterion over S subheads: the decoder criterion of the IIC estimators (csrc/iic_patch.hip).  Replaces
 * IICEstimator.forward's decoder branch (semi_seg/mi_estimator/discrete_mi_estimator.py:33-40, :53-60: per subhead
 * IIDSegmentationSmallPathLoss(padding, patch_size) on the probability maps of a DenseClusterHead, contrastyou/projectors/
 * heads.py:149-169) as semi_seg/epochers/_mixins.py:86 calls it with Y flipped.
 * lx / ly: logits [N][H][W][ld] f32, subhead s in columns s*K .. s*K+K-1, ld >= S*K; 2 <= K <= 32, 0 <= pad <= 7, patch >= 2.
 * flags_y, the patch starts, the clipping and PX = 0 outside the PATCH are those of spcl_iic_patch_*; per (s, P) the joint
 * and IIDSegmentationLoss (iic_loss.py:77-97, lamda = 1) in float64 from 32.32 fixed-point joints.
 *   spcl_iic_patch_heads_plan:     argument check without a launch; patch count nP of ONE subhead, workspace bytes, f32
 *                          elements of dj (each output pointer may be NULL).
 *   spcl_iic_patch_heads_forward:  loss[0] = scale * sum_s mean_P loss_{s,P}; head_patch_loss (nullable, [S][nP]) = the
 *                          loss_{s,P}, not scaled; nan_flag[0] = 1 when any of them is NaN; dj = d loss / d J_{s,P} as
 *                          spcl_iic_patch_heads_backward reads it.  ws is zeroed by the call.  Bitwise deterministic.
 *   spcl_iic_patch_heads_backward: dlx = d loss / d lx (times *gscale when non-NULL) in columns s*K + k only; dly, when
 *                          non-NULL, the same for ly at Y's unflipped position.  Each element is written exactly once, no
 *                          atomics; columns >= S*K are left alone. */
int spcl_iic_patch_heads_plan(int N, int S, int K, long ld, int H, int W, int pad, int patch, int* num_patches,
                              size_t* ws_bytes, size_t* dj_elems);
int spcl_iic_patch_heads_forward(const float* lx, const float* ly, long ld, int N, int H, int W, int S, int K, int pad,
                                 int patch, const uint8_t* flags_y, float scale, float* loss, float* head_patch_loss,
                                 int* nan_flag, float* dj, void* ws, size_t ws_bytes, void* stream);
int spcl_iic_patch_heads_backward(const float* lx, const float* ly, long ld, int N, int H, int W, int S, int K, int pad,
                                  int patch, const uint8_t* flags_y, const float* dj, const float* gscale, float* dlx,
                                  float* dly, void* stream);

/* ---------------------------------------------------------------- mean teacher / entropy minimisation (csrc/semi_reg.hip) ----
 * Replaces the arithmetic of semi_seg/hooks/mt.py:48-54 and semi_seg/hooks/entmin.py:30-34 of the reference.
 *
 *   spcl_ema_update: teacher[i] = (alpha * teacher[i] + (1 - alpha) * student[i]) * (1 - decay) over two flat f32 buffers of n
 *                    elements in ONE launch (mt.py:54 -> deepclustering2 ema_updater: mul_(alpha), add_((1 - alpha) * s),
 *                    mul_(1 - decay) per parameter tensor).  Three f32 roundings per element in that order; decay == 0 leaves
 *                    the last multiplication out.  The buffers need 4-byte alignment only and must not overlap; alpha and decay
 *                    are host values.
 *   spcl_mt_softmax_mse: weight * mean((flip(T) - softmax(student_logits))^2) over [N][H][W][C] f32 class maps (C <= 16), the
 *                    teacher map read through the per-sample flip flags (bit 0 flips H, bit 1 flips W); teacher_mode 0: T is the
 *                    teacher's raw output (what mt.py:49-52 computes: its `prob` is never soft-maxed), 1: T = softmax(teacher)
 *                    (_mixins.py:147).  dstudent = the gradient w.r.t. student_logits for a unit upstream gradient (the teacher
 *                    gets none); ws: spcl_mt_softmax_mse_workspace_bytes(N, H, W).
 *   spcl_entropy_softmax: weight * mean over the N*H*W pixels of -sum_c p_c log(p_c + eps), p = softmax(logits)
 *                    (entmin.py:30-31 -> deepclustering2 Entropy); dlogits = its gradient for a unit upstream gradient; ws:
 *                    spcl_entropy_softmax_workspace_bytes(N, H, W).
 *   spcl_ucmt_softmax_mse: the criterion of the uncertainty-aware mean teacher (semi_seg/epochers/comparable.py:84-105) in one
 *                    launch.  teacher, the K noisy teacher maps (noisy: a HOST array of K device pointers, 1 <= K <= 16, handed
 *                    to the kernel by value -- nothing is uploaded) and student_logits are [N][H][W][C] f32 (C <= 16); every
 *                    teacher map is read through the per-sample flip flags (bit 0 flips H, bit 1 flips W).  Per pixel of the
 *                    student's frame: p = softmax(student), t = softmax(flip(teacher)), avg = (noisy[0] + ... + noisy[K-1]) /
 *                    (float)K (an f32 sum in list order, then one f32 division), q = softmax(flip(avg)), u = -sum_c q_c
 *                    log(q_c + eps) / log(C), m = (u <= threshold) (a NaN u gives 0).  loss = weight / (N H W C) * sum_pixels
 *                    m * sum_c (p_c - t_c)^2; dstudent = its gradient w.r.t. student_logits for a unit upstream gradient
 *                    (exact zeros where m = 0; the teacher maps get none); kept[0] = the number of pixels with m = 1 (an exact
 *                    integer); mask (nullable, [N][H][W] bytes) receives m.  ws: spcl_ucmt_workspace_bytes(N, H, W).
 *   The losses are fixed-order sums (per-workgroup double partials added in index order): bitwise reproducible. */
int spcl_ema_update(float* teacher, const float* student, size_t n, double alpha, double decay, void* stream);
size_t spcl_mt_softmax_mse_workspace_bytes(int N, int H, int W);
int spcl_mt_softmax_mse(const float* teacher, const float* student_logits, int N, int C, int H, int W,
                        const uint8_t* flags_teacher, int teacher_mode, float weight, float* loss, float* dstudent, void* ws,
                        size_t ws_bytes, void* stream);
size_t spcl_entropy_softmax_workspace_bytes(int N, int H, int W);
int spcl_entropy_softmax(const float* logits, int N, int C, int H, int W, float eps, float weight, float* loss, float* dlogits,
                         void* ws, size_t ws_bytes, void* stream);
size_t spcl_ucmt_workspace_bytes(int N, int H, int W);
int spcl_ucmt_softmax_mse(const float* teacher, const float* const* noisy, int K, const float* student_logits, int N, int C,
                          int H, int W, const uint8_t* flags_teacher, float threshold, float eps, float weight, float* loss,
                          float* dstudent, unsigned long long* kept, uint8_t* mask, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- mix-up baseline (csrc/semi_reg.hip) -------------------------
 * Replaces the arithmetic of semi_seg/hooks/mixup.py:19-32 (mixup_data) and :66-75 (one-hot targets, concatenations, softmax,
 * KL_div) of the reference.  Both entry points read the VIRTUAL concatenation of two batches of B = N2 / 2 samples (sample n
 * is the first batch's n for n < B, the second's n - B otherwise; nothing is concatenated) and a device permutation
 * index[N2] (int32) of its samples.  lam / oml: the f32 roundings of the host's float64 lam and 1 - lam.  The caller checks
 * on the host that every index entry lies in [0, N2) (functional.MixupPlan does); for an entry outside it the kernels pair the
 * sample with itself, so that no content of the buffer makes them read outside their inputs.
 *
 *   spcl_mixup_images: out[n] = fl(fl(lam * x[n]) + fl(oml * x[index[n]])) over f32 samples of per_sample elements
 *                    (mixup.py:30): three roundings in the order torch evaluates the expression on an f32 tensor, never
 *                    contracted to a fused multiply-add -- the result is torch's bit for bit.  One launch, 12 bytes per
 *                    element; 16-byte accesses when per_sample % 4 == 0 and the three base pointers are 16-byte aligned,
 *                    4-byte ones otherwise.  out [N2 * per_sample] must not overlap either input.
 *   spcl_mixup_kl_onehot: weight * KL_div(eps)(softmax(logits), lam * onehot(y) + oml * onehot(y[index])), the mean over the
 *                    N2*H*W pixels of sum_c -t_c log((p_c + eps) / (t_c + eps)) (mixup.py:31,66-75), y the two int64 label maps
 *                    [B, H, W], logits [N2, H, W, C] f32 (C <= 16); t_c is built in f32 as torch builds mixed_y (fl(lam + oml)
 *                    where the two labels agree).  Labels are compared with the class index only: one outside [0, C) selects
 *                    no class.  dlogits = the gradient for a unit upstream gradient; ws: spcl_mixup_kl_workspace_bytes(N2,
 *                    H, W).  A fixed-order sum as above: bitwise reproducible. */
int spcl_mixup_images(const float* image, const float* image_tf, const int* index, int N2, size_t per_sample, float lam,
                      float oml, float* out, void* stream);
size_t spcl_mixup_kl_workspace_bytes(int N2, int H, int W);
int spcl_mixup_kl_onehot(const float* logits, const int64_t* target, const int64_t* target_tf, const int* index, int N2, int C,
                         int H, int W, float lam, float oml, float eps, float weight, float* loss, float* dlogits, void* ws,
                         size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- adversarial baseline: DCGAN discriminator (csrc/discr.hip) ---
 * Replaces the ATen sequence of semi_seg/arch/discr.py:17-36 (Conv2d(., ., 4, 2, 1, bias=False) / BatchNorm2d / LeakyReLU(0.2)
 * x 4, Conv2d(., 1, 4, 1, 0) / Sigmoid) and the nn.BCELoss of semi_seg/epochers/new_comparable.py:124,162-163,183-191 (ABI 15).
 * All f32; every sum has a fixed order (no floating-point atomics): bitwise reproducible.
 *
 * Lowering: a 4x4 stride-2 padding-1 convolution is a rows product (spcl_rows_linear_*) over PATCH ROWS
 *   rows[m][k],  m = (n Ho + oh) Wo + ow,  k = 16 c + 4 kh + kw,  Ho = (H + 2 - 4) / 2 + 1 (floor), Wo likewise,
 *   rows[m][k] = T(x[n][c][2 oh - 1 + kh][2 ow - 1 + kw]) inside the image and exactly 0 at a padded tap (NOT T(0)).
 * In this k order the contiguous [Cout][C][4][4] parameter IS the weight matrix Wr[Cout][16 C] of the product, and its gradient
 * dWr the parameter's gradient: nothing is repacked or permuted, in either direction, ever.  The layer's output y[M][Cout] =
 * rows Wr^T is the NHWC map the next layer reads.
 * T (mode): 0 identity | 1 LeakyReLU(0.2)(x), x a stored pre-activation | 2 LeakyReLU(0.2)(scale[c] x + shift[c]), x a stored
 * pre-BatchNorm map.  (The slope is 0.2: the leaky_in flags of the rows product are 0.01 and are not used here.)
 *
 *   spcl_patch4s2_rows_forward: the input is the channel concatenation of two strided f32 maps, a (Ca channels, element
 *                    strides a_sn/a_sc/a_sh/a_sw) in front of b (Cb channels; b NULL with Cb = 0): a class map, or image + class
 *                    map, read where it lies, NCHW or channels-last.  C = Ca + Cb; rows [N Ho Wo][16 C].  A dense NHWC input with
 *                    C % 4 == 0 (an inner layer) is read in 16-byte pieces along c and written in 16-byte pieces along kw.
 *   spcl_patch4s2_rows_backward: gather form -- every input pixel sums the <= 2 x 2 output positions / taps that cover it from
 *                    drows [N Ho Wo][16 C] in a fixed order and multiplies by T'; in mode 2 the result is the gradient w.r.t.
 *                    the BatchNorm OUTPUT scale x + shift (spcl_rows_bn_backward finishes it).  x [N][H][W][C] is the stored map
 *                    of modes 1, 2 (NULL in mode 0).  dx [N][H][W][C - c_lo] dense NHWC holds channels c_lo .. C-1 (c_lo > 0, mode
 *                    0 only: the image channels in front of a class map get no gradient).
 *   spcl_rows_bn_forward: training-mode BatchNorm statistics of x [M][C] (C % 4 == 0, C <= 1024, M >= 2) in ONE launch: sums of
 *                    (x - x[0][c]) and its square per slab of rows, folded in slab order in double by the workgroup that finishes
 *                    last.  stats [4][C] = mean, 1 / sqrt(var + eps) (biased var), scale = gamma invstd, shift = beta - mean
 *                    scale (what mode 2 reads).  running_mean / running_var (both or neither) are updated with `momentum` and the
 *                    unbiased variance; num_batches_tracked is the caller's.  ws: spcl_rows_bn_workspace_bytes(M, C).
 *   spcl_rows_bn_eval_affine: stats [4][C] from the running statistics (eval mode).
 *   spcl_rows_bn_backward: from du = dLoss/d(scale x + shift): dbeta = sum du, dgamma = sum du xhat (one launch, folded as
 *                    above), dx = gamma invstd (du - dbeta / M - xhat dgamma / M) (second launch); with training = 0 the batch
 *                    terms are left out (dx = scale du).  dx may alias du.
 *   spcl_discr_head_forward: Conv2d(C, 1, 4, 1, 0) over LeakyReLU(0.2)(scale x + shift) of x [N][H][W][C] (C % 4 == 0, H, W >= 4),
 *                    w [16 C] in the k order above (the [1][C][4][4] parameter): t [M] logits (M = N (H-3) (W-3)), d [M] = sigmoid(t); with y = 0 or 1 also
 *                    loss[0] = mean BCE(d, y) and dt [M] = (d - y) / M (d - 1 formed as -sigmoid(-t), no cancellation), with y < 0 neither (loss, dt may be NULL).  One launch, the
 *                    mean folded in index order in double by the last workgroup.  The loss is evaluated as softplus(-t) (y = 1) /
 *                    softplus(t) (y = 0), softplus(z) = max(z, 0) + log1p(exp(-|z|)): equal to nn.BCELoss's -max(log(.), -100) of
 *                    the f32 sigmoid while |t| <= 12 or so; beyond, the f32 sigmoid saturates (1 - d = 0 from t ~ 17: the reference
 *                    then reports 100 and a zero gradient where this reports t and a gradient of 1 / M).
 *                    ws: spcl_discr_head_workspace_bytes(N, H, W, C).
 *   spcl_discr_head_backward: dt' = dt * (grad ? grad[0] : 1) (grad a device scalar).  du [N][H][W][C] (nullable) = the gradient
 *                    w.r.t. scale x + shift (gather over the <= 16 positions that cover a pixel); dw [16 C] (nullable) = sum_m dt'
 *                    act(.) over slabs of positions, folded in slab order.  Only what is asked for is computed. */
int spcl_patch4s2_rows_forward(const float* a, int Ca, long a_sn, long a_sc, long a_sh, long a_sw, const float* b, int Cb,
                               long b_sn, long b_sc, long b_sh, long b_sw, int N, int H, int W, int mode, const float* scale,
                               const float* shift, float* rows, void* stream);
int spcl_patch4s2_rows_backward(const float* drows, const float* x, int N, int H, int W, int C, int c_lo, int mode,
                                const float* scale, const float* shift, float* dx, void* stream);
size_t spcl_rows_bn_workspace_bytes(int M, int C);
int spcl_rows_bn_forward(const float* x, int M, int C, const float* gamma, const float* beta, float eps, float momentum,
                         float* running_mean, float* running_var, float* stats, void* ws, size_t ws_bytes, void* stream);
int spcl_rows_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                             float eps, int C, float* stats, void* stream);
int spcl_rows_bn_backward(const float* du, const float* x, int M, int C, const float* gamma, const float* stats, int training,
                          float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);
size_t spcl_discr_head_workspace_bytes(int N, int H, int W, int C);
int spcl_discr_head_forward(const float* x, int N, int H, int W, int C, const float* scale, const float* shift, const float* w,
                            int y, float* t, float* d, float* loss, float* dt, void* ws, size_t ws_bytes, void* stream);
int spcl_discr_head_backward(const float* x, int N, int H, int W, int C, const float* scale, const float* shift, const float* w,
                             const float* dt, const float* grad, float* du, float* dw, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- MINE baseline: the statistics network's two ends (csrc/mine.hip) ---
 * The statistics network of semi_seg/mi_estimator/mineestimator.py:19-30 is two conv3x3 + BatchNorm + ReLU layers (the kernels
 * above) between an input that is a concatenation and a tail that is a pooled linear logit; these four entry points are those
 * two ends (ABI 21).  dtype: SPCL_F32 / SPCL_BF16, the storage type of every map; CS(c) = c rounded up to 16.  Every sum has a
 * fixed order (no floating-point atomics): bitwise reproducible.
 *
 *   spcl_mine_pairs_forward: replaces torch.cat([feat2[1:], feat2[0:1]]), the two torch.cat([feat1, .], dim=1) of
 *                    mineestimator.py:33-35 and the per-sample flips of semi_seg/epochers/_mixins.py:79-82.  feat [2n][H][W][CS(C)]
 *                    is the extracted feature (rows 0..n-1: the unlabelled images, rows n..2n-1: their transformed copies), flags
 *                    uint8 [n] the batch's flips (bit 0 flips H, bit 1 flips W; NULL: none).  joint, marg [n][H][W][CS(2C)]:
 *                    channels 0..C-1 of both are feat[n + i]; channels C..2C-1 are flip_i(feat[i]) in joint and
 *                    flip_j(feat[j]), j = (i + 1) mod n, in marg; pad channels are 0.  One launch; 16-byte accesses when
 *                    C % 16 == 0 and the three pointers are 16-byte aligned, element-wise ones otherwise.
 *   spcl_mine_pairs_backward: its gradient as one gather: dfeat[n + i] = dJ[i][:C] + dM[i][:C], dfeat[i] = flip_i(dJ[i][C:] +
 *                    dM[(i - 1) mod n][C:]), added in f32 and rounded once; pad channels of dfeat [2n][H][W][CS(C)] are 0.
 *   spcl_mine_head_forward: replaces nn.AdaptiveMaxPool2d((1, 1)) / Flatten / nn.Linear(C / 2, 1) of mineestimator.py:27-29 and
 *                    the two F.softplus(.).mean() of :34-35, for both passes in one launch.  act_joint, act_marg
 *                    [n][H][W][CS(C / 2)] are the second layer's stored activations (C the network's input_dim: even,
 *                    C / 2 <= 256).  maxima [2][n][C / 2] (f32) and argmax [2][n][C / 2] (int32, h W + w; the first index in
 *                    row-major order among equal values, a NaN wins) -- pass 0 is the joint one; t [2][n] = b[0] + sum_c w[c]
 *                    maxima[c], an f32 FMA chain in channel order; loss[0] = mean_i sp(t[1][i]) + mean_i sp(t[0][i]) = Em - Ej of
 *                    :34-36, sp(t) = max(t, 0) + log1p(exp(-|t|)), each mean added in index order in double.  A workgroup takes
 *                    256 pixels of one (pass, sample), lanes along the channel axis; the workgroup that finishes last folds the
 *                    slabs in index order and forms logits and loss.  ws: spcl_mine_head_workspace_bytes(n, H, W, C) (0: a
 *                    shape the entry refuses).
 *   spcl_mine_head_backward: one launch.  dt = sigmoid(t) * (grad ? grad[0] : 1) / n (grad a device scalar); dw [C / 2] = sum dt
 *                    maxima and db [1] = sum dt over (pass, sample) in index order (either may be NULL); dact_joint, dact_marg
 *                    [n][H][W][CS(C / 2)] are written densely: w[c] dt at the argmax, 0 everywhere else.  argmax is only ever
 *                    compared with a pixel index, never used as an address. */
int spcl_mine_pairs_forward(const void* feat, const uint8_t* flags, int dtype, int n, int H, int W, int C, void* joint, void* marg,
                            void* stream);
int spcl_mine_pairs_backward(const void* djoint, const void* dmarg, const uint8_t* flags, int dtype, int n, int H, int W, int C,
                             void* dfeat, void* stream);
size_t spcl_mine_head_workspace_bytes(int n, int H, int W, int C);
int spcl_mine_head_forward(const void* act_joint, const void* act_marg, int dtype, int n, int H, int W, int C, const float* w,
                           const float* b, float* t, float* maxima, int* argmax, float* loss, void* ws, size_t ws_bytes,
                           void* stream);
int spcl_mine_head_backward(const float* t, const float* maxima, const int* argmax, const float* w, const float* grad, int dtype,
                            int n, int H, int W, int C, void* dact_joint, void* dact_marg, float* dw, float* db, void* stream);

/* ---------------------------------------------------------------- PICA baseline: partition-uncertainty-index criteria (csrc/pica.hip) ---
 * contrastyou/losses/pica_loss.py of the reference on the cluster heads of the IIC criteria (ABI 22).  Float64 from the
 * probabilities / the joint on, every sum in a fixed order: bitwise reproducible.  ws: spcl_pica_workspace_bytes(S).
 *
 *   spcl_pica_seg_loss: replaces pica_loss.py:63-73,81-84 (PUISegLoss from the F.conv2d joint on: min-shift, per-displacement
 *                    normalisation, symmetrisation, mean over the T^2 displacements, -mean(I log(P + 1e-16))) and its autograd.
 *                    The joint comes as spcl_iic_joint_forward's 32.32 fixed-point jacc or as an f32 jf32 [S][T][T][K][K]
 *                    (exactly one); 2 <= K <= 32, T odd <= 15.  One workgroup per subhead.  With ce_s the criterion of subhead s:
 *                    loss[0] = scale * sum_s (ce_s + lamda_ne), ce_out[0] (nullable) = scale * sum_s ce_s, dj = d loss / d J in
 *                    the layout spcl_iic_joint_backward reads (the min is detached), j_out (nullable, with jacc) = J in f32.
 *                    lamda_ne: lamda times the balance term of pica_loss.py:76-77, which is a constant of the shape there (the
 *                    mean runs over the class axis of the permuted map): lamda * (log M - (M / K) log K), M = N H W.
 *   spcl_pica_global_loss: replaces PUILoss.forward (pica_loss.py:31-38) and its autograd.  lx / ly: logits rows [N][ld] f32,
 *                    subhead s in columns s*K .. s*K+K-1, the grouped softmax applied as the rows are read; any N >= 1.  One
 *                    launch, one workgroup per subhead, two passes over the rows.  loss[0] = scale * sum_s (ce_s + lamda ne_s)
 *                    (ce_s the cross-entropy of the cosine matrix of the columns against its diagonal, ne_s = log K + sum_k
 *                    p_k log p_k of the column means of x, no epsilon), ce_out[0] (nullable) = scale * sum_s ce_s, dlx / dly =
 *                    d loss / d lx, d loss / d ly (times *gscale when non-NULL); the columns s*K + k are written, the others
 *                    are left alone. */
size_t spcl_pica_workspace_bytes(int S);
int spcl_pica_seg_loss(const long long* jacc, const float* jf32, int S, int K, int T, double lamda_ne, float scale, float* j_out,
                       float* loss, float* ce_out, float* dj, void* ws, size_t ws_bytes, void* stream);
int spcl_pica_global_loss(const float* lx, const float* ly, long ld, int N, int S, int K, float lamda, float scale,
                          const float* gscale, float* loss, float* ce_out, float* dlx, float* dly, void* ws, size_t ws_bytes,
                          void* stream);

/* ---------------------------------------------------------------- soft-Dice + class-weighted KL (csrc/sup_dice.hip) ---
 * The supervised criterion of contrastyou/losses/dice.py (not in the reference; ABI 31).  p = softmax(logits), t = one-hot of the
 * label, M = N H W, S = all classes or 1 .. C-1 (include_background == 0), groups g = the batch (G = 1) or one per sample
 * (per_sample != 0, G = N); I_gc = sum p t, P_gc = sum p, T_gc = sum t over the pixels of group g:
 *   L_dice = 1 - 1 / (G |S|) sum_g sum_{c in S} (2 I_gc + smooth) / (P_gc + T_gc + smooth)
 *   L_kl   = 1 / M sum_i class_weight[l_i] * -log((p_{i,l_i} + eps) / (1 + eps))
 *   loss   = dice_weight L_dice + kl_weight L_kl
 * A label outside [0, C) is an all-zero one-hot row: no KL term, nothing in I or T, its probabilities count in P.
 * logits [N][H][W][C] f32 (C <= 16, N <= 1024), labels [N][H][W] int64, class_weight [C] f32, used as given.
 *
 *   spcl_sup_dice_forward: two launches (the sums of every workgroup; their fixed-order total).  loss[0], parts[0] = L_kl, parts[1] = L_dice; inter / uni [N][C] int64 = the Dice counts of
 *                    the arg-max map against the labels, as spcl_sup_loss_forward writes them (written, not added to);
 *                    coef [G][C][2] f32 = per (group, class) a = -2 / (G |S| D) and b = (2 I + smooth) / (G |S| D^2) with
 *                    D = P + T + smooth (both 0 outside S): what spcl_sup_dice_backward reads.  Sums in float64 / integers in
 *                    a fixed order, no floating-point atomics: bitwise reproducible.  ws: spcl_sup_dice_workspace_bytes(N, C,
 *                    H, W) bytes, 16-byte aligned.  Its first 64 bytes hold the workgroups' ticket: zero them ONCE, when the
 *                    workspace is allocated -- a call that completes leaves them zero (no memset per call, nothing but the
 *                    two kernels in a captured graph).  Calls that share a workspace must be ordered on one stream.
 *   spcl_sup_dice_backward: one launch, no reduction: dlogits [N][H][W][C] = d loss / d logits (times gscale[0] when gscale is
 *                    non-NULL), with d loss / d p_c = dice_weight (a t_c + b) - [c == l] kl_weight class_weight[l] /
 *                    (M (p_l + eps)) taken through the softmax. */
size_t spcl_sup_dice_workspace_bytes(int N, int C, int H, int W);
int spcl_sup_dice_forward(const float* logits, const int64_t* labels, const float* class_weight, int N, int C, int H, int W,
                          float dice_weight, float kl_weight, int include_background, int per_sample, float smooth, float eps,
                          float* loss, float* parts, int64_t* inter, int64_t* uni, float* coef, void* ws, size_t ws_bytes,
                          void* stream);
int spcl_sup_dice_backward(const float* logits, const int64_t* labels, const float* class_weight, const float* coef, int N,
                           int C, int H, int W, float dice_weight, float kl_weight, int per_sample, float eps,
                           const float* gscale, float* dlogits, void* stream);

/* ---------------------------------------------------------------- boundary loss (csrc/boundary.hip) -----------------
 * Signed Euclidean distance maps of a label batch and the boundary criterion of contrastyou/losses/boundary.py (Kervadec et
 * al., MIDL 2019; not in the reference; ABI 32).  For sample n and listed class c, m = (labels[n] == c); a label outside the
 * class list's values belongs to no listed class.  d2(x) = the smallest integer (dy)^2 + (dx)^2 from pixel x to a pixel of
 * the same slice whose membership in m differs from x's (unit spacing);
 *   phi[n, c, x] = +sqrt(d2) outside m,  -(sqrt(d2) - 1) inside m  (float64 square root, rounded once to f32),
 *   phi == 0 on the whole slice where no pixel of the opposite membership exists (class absent, or class fills the slice).
 *   L_B = 1 / (N S H W) sum_{n, s, x} softmax(logits)[n, classes[s], x] * phi[n, s, x]
 *
 *   spcl_signed_distance_maps: labels [N][H][W] int64, classes = HOST array of n_classes <= 16 distinct values >= 0,
 *                    phi [N][H][W][n_classes] f32 (channels-last, beside the logits).  H, W <= 1024, N <= 1024.  Two launches
 *                    (column scans into two uint16 planes per (n, class): vertical distance to the nearest pixel inside /
 *                    outside m, 0xFFFF = none; row minima over integer squares in LDS, one wave per row), no atomics, nothing
 *                    read back: the same input gives the same bits.  ws: spcl_signed_distance_workspace_bytes(N, H, W,
 *                    n_classes) bytes (0 = unsupported shape), 16-byte aligned.
 *   spcl_boundary_forward: logits [N][H][W][C] f32 (C <= 16, N <= 1024), classes = HOST array of n_classes distinct values in
 *                    [0, C), alpha = a DEVICE f32 scalar.  lb[0] = L_B, loss[0] = alpha * L_B.  Two launches: float64 partials
 *                    per workgroup, then their sum in index order (no ticket, no fence, no floating-point atomics, no memset):
 *                    bitwise reproducible.  ws: spcl_boundary_workspace_bytes(N, H, W) bytes, 8-byte aligned.
 *   spcl_boundary_backward: one launch: dlogits [N][H][W][C] = g p_k (a_k - sum_c a_c p_c), a_c = alpha phi_c / (N S H W) for a
 *                    listed class and 0 otherwise, g = gscale[0] (a device scalar) or 1 when gscale is NULL.  alpha is read
 *                    on the device: a captured call replays with whatever the scalar holds then. */
size_t spcl_signed_distance_workspace_bytes(int N, int H, int W, int n_classes);
int spcl_signed_distance_maps(const int64_t* labels, int N, int H, int W, const int* classes, int n_classes, float* phi,
                              void* ws, size_t ws_bytes, void* stream);
size_t spcl_boundary_workspace_bytes(int N, int H, int W);
int spcl_boundary_forward(const float* logits, const float* phi, const int* classes, int n_classes, int N, int C, int H, int W,
                          const float* alpha, float* loss, float* lb, void* ws, size_t ws_bytes, void* stream);
int spcl_boundary_backward(const float* logits, const float* phi, const int* classes, int n_classes, int N, int C, int H, int W,
                           const float* alpha, const float* gscale, float* dlogits, void* stream);

/* ---------------------------------------------------------------- pseudo-labelling baseline (csrc/pseudo_label.hip) -----------
 * Self-training with confidence-thresholded pseudo-labels (FixMatch) and the self-adaptive per-class thresholds of FreeMatch
 * (Wang et al., ICLR 2023); not in the reference.  One launch.
 *
 *   spcl_pseudo_label_ce: teacher and student_logits are [N][H][W][C] f32 class maps, 1 <= C <= 16; the teacher map is read
 *                    through the per-sample flip flags (bit 0 flips H, bit 1 flips W, NULL: no flips).  Per pixel of the
 *                    student's frame: q = softmax(flip(teacher)); y = argmax_c of the teacher's LOGITS (exact; a tie goes to
 *                    the lowest class); conf = max_c q_c, formed in f32 as 1 / z with z the sum of exp(logit - max logit);
 *                    keep = conf >= tau[y] (a NaN confidence keeps nothing); p = softmax(student_logits); term = keep ?
 *                    -log p_y : 0.  loss = weight / M * sum term with M = N H W (FixMatch's mean over ALL pixels, not over
 *                    the kept ones); dstudent_k = keep ? weight / M * (p_k - [k == y]) : 0 for a unit upstream gradient
 *                    (exact zeros at dropped pixels; the teacher gets no gradient).
 *                    stats[0] = sum conf, stats[1 + c] = sum q_c over ALL pixels, in double.  hist[c] = the number of pixels
 *                    with y == c, hist[C + c] = the number of KEPT pixels with y == c (exact integers).  label (nullable,
 *                    [N][H][W] bytes) receives keep ? y : 255.
 *                    tau: C device floats.  state == NULL (fixed thresholds): tau is read only.  state != NULL (self-adaptive):
 *                    state = (tau_g, ptilde[0 .. C)) in double on the device; the pixels of THIS launch compare against tau as
 *                    it stands on entry, and once the sums are complete the closing workgroup stores in place, in double,
 *                      tau_g' = m tau_g + (1 - m) stats[0] / M,   ptilde'[c] = m ptilde[c] + (1 - m) stats[1 + c] / M,
 *                      tau'[c] = (float)(ptilde'[c] / max_c ptilde' * tau_g')
 *                    with m = momentum in [0, 1): a one-step lag against FreeMatch's Algorithm 1, which counts the current
 *                    batch into the threshold it is compared with.  Nothing is read back by the host.
 *                    Every sum is a fixed association (per thread in pixel order, wave butterfly, waves in order, workgroup
 *                    rows in index order by the last workgroup to take a ticket): all outputs are bitwise reproducible.  No
 *                    floating-point atomics; one 4-byte memset (the ticket).  Shapes refused: N, H or W <= 0, C outside
 *                    [1, 16], N H W >= 2^31.  ws: spcl_pseudo_label_workspace_bytes(N, C, H, W) bytes (0 for a refused
 *                    shape), 8-byte aligned. */
size_t spcl_pseudo_label_workspace_bytes(int N, int C, int H, int W);
int spcl_pseudo_label_ce(const float* teacher, const float* student_logits, int N, int C, int H, int W,
                         const uint8_t* flags_teacher, float* tau, double* state, double momentum, float weight, float* loss,
                         float* dstudent, double* stats, unsigned long long* hist, uint8_t* label, void* ws, size_t ws_bytes,
                         void* stream);

/* ---------------------------------------------------------------- label-guided pixel contrast (csrc/pixel_contrast.hip) -------
 * A class-balanced sample of decoder cells chosen on the device, the gather of their feature rows and a supervised-contrastive
 * criterion over the gathered, projected rows; not in the reference.  Nothing is read back, the launch count of every entry is
 * fixed, every entry is capturable, all outputs are bitwise reproducible (integer atomics only).
 *
 *   spcl_pixel_sample: cell_label is int32 [ncells] (flat index i = b h w + y w + x); a cell is eligible for class c iff
 *                    cell_label[i] == c with 0 <= c < C (any other value: ineligible).  key(i) = fmix32((((i + 1) *
 *                    0x9E3779B1) mod 2^32) ^ *seed), fmix32 the MurmurHash3 finaliser (h ^= h >> 16; h *= 0x85EBCA6B;
 *                    h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16, mod 2^32), seed ONE 32-bit word in device memory (read by
 *                    the kernels: a captured call replays with what the word holds then).  Keys of distinct cells are
 *                    distinct.  Per class the min(K, n_c) eligible cells with the smallest keys are chosen: idx int32 [C][K]
 *                    receives their flat indices in ascending index order, then -1; count int32 [C] = min(K, n_c).
 *                    A radix select of the K-th key per class (four byte histograms), a count and a write pass in index order:
 *                    one memset and six launches.  Refused: C outside [2, 16], K outside [1, 1024], C K > 4096, ncells < 1.
 *                    ws: spcl_pixel_sample_workspace_bytes(ncells) bytes (0 for ncells < 1), 4-byte aligned.
 *   spcl_rows_gather_forward: rows[m][0 .. Cf) = feat[idx[m]][0 .. Cf) as f32, m < M; feat is the channels-last storage of the
 *                    feature map, f32 or bf16 (SPCL_F32 / SPCL_BF16), cell i at feat + i * cs elements (cs >= Cf).  A row whose
 *                    index is negative (or >= ncells) is exactly zero.
 *   spcl_rows_gather_backward: dfeat (the storage dtype and pitch of feat, ncells * cs elements) is zero everywhere except
 *                    dfeat[idx[m]][0 .. Cf) = drows[m] (rounded to nearest even for bf16).  The indices >= 0 must be distinct
 *                    (the sampler's are): one memset and plain stores, no atomics.
 *   spcl_pixel_supcon_forward: z is [M = C K][d] f32 rows (contiguous, 16-byte aligned).  Slot m = c K + j has class c and is
 *                    VALID iff j < count[c] (count int32 [C] on the device, clamped to [0, K]); no label vector or mask is
 *                    read.  For a valid row i: A(i) = the valid rows other than i, P(i) = those of i's class, I = the valid
 *                    rows with |P(i)| >= 1;
 *                      l_i = -(1 / |P(i)|) sum_{p in P(i)} [ z_i.z_p / t - log sum_{a in A(i)} exp(z_i.z_a / t) ],
 *                      loss = (1 / |I|) sum_{i in I} l_i,   0 when I is empty.
 *                    Invalid rows are never loaded (they may hold NaN).  Products on the exact-f32 MFMA in one contraction
 *                    order; a row block's column tiles are dealt to up to 8 workgroups (a function of M alone), each keeps row
 *                    sums with a running maximum in tile order, a closing workgroup joins them in split order and adds the
 *                    rows' terms in double in index order.  The workspace keeps the rows' log-sums for the backward call.
 *                    Two launches.
 *   spcl_pixel_supcon_backward: dz [M][d] = (*gscale, or 1 for NULL) * dloss/dz; exact zeros in invalid rows and everywhere
 *                    when I is empty.  ws: the workspace the forward call of the SAME z and count left.  Two launches: the
 *                    similarity tiles are formed again with the same bits (the matrix is never stored) and every column
 *                    split leaves its share of the gradient in the workspace; the second launch adds them in split order.
 *                    Refused by both: C outside [2, 16], K outside [1, 1024], C K > 4096, d outside [4, 256] or not a
 *                    multiple of 4, t <= 0.  ws: spcl_pixel_supcon_workspace_bytes(M, d) bytes (0 for a refused M or d),
 *                    16-byte aligned. */
size_t spcl_pixel_sample_workspace_bytes(int ncells);
int spcl_pixel_sample(const int32_t* cell_label, int ncells, int C, int K, const uint32_t* seed, int32_t* idx, int32_t* count,
                      void* ws, size_t ws_bytes, void* stream);
int spcl_rows_gather_forward(const void* feat, int dtype, int ncells, int Cf, int64_t cs, const int32_t* idx, int M, float* rows,
                             void* stream);
int spcl_rows_gather_backward(const float* drows, const int32_t* idx, int M, int Cf, void* dfeat, int dtype, int ncells,
                              int64_t cs, void* stream);
size_t spcl_pixel_supcon_workspace_bytes(int M, int d);
int spcl_pixel_supcon_forward(const float* z, const int32_t* count, int C, int K, int d, float t, float* loss, void* ws,
                              size_t ws_bytes, void* stream);
int spcl_pixel_supcon_backward(const float* z, const int32_t* count, int C, int K, int d, float t, const float* gscale,
                               void* ws, size_t ws_bytes, float* dz, void* stream);

/* ---------------------------------------------------------------- cross pseudo supervision (csrc/cross_pseudo.hip) -----------
 * Two networks on the same images, each trained with cross-entropy towards the other's hard arg-max prediction (CPS; Chen et
 * al., CVPR 2021); not in the reference.  Both directions in one launch.
 *
 *   spcl_cross_pseudo_ce: a_logits and b_logits are [N][H][W][C] f32 class maps in the same frame (no flip flags), 1 <= C <=
 *                    16; they may be one buffer.  Per pixel: pA = softmax(a), pB = softmax(b); yA = argmax_c a_c, yB =
 *                    argmax_c b_c on the LOGITS (exact; a tie goes to the lowest class); confA = max pA, confB = max pB, formed
 *                    in f32 as 1 / z with z the sum of exp(logit - max logit), exactly as spcl_pseudo_label_ce forms its
 *                    confidence; keepA = confA >= tau[yA], keepB = confB >= tau[yB] (tau: C device floats; NULL: every pixel
 *                    with a numeric confidence is kept; a NaN confidence keeps nothing); term = keepB * -log pA[yB] + keepA *
 *                    -log pB[yA].  With M = N H W, for a unit upstream gradient:
 *                      loss[0] = weight / M * sum term (the mean over ALL pixels); parts[0], parts[1] = the two directions
 *                      separately, a <- b then b <- a;
 *                      da_k = keepB ? weight / M * (pA_k - [k == yB]) : 0,  db_k = keepA ? weight / M * (pB_k - [k == yA]) : 0
 *                      (exact zeros at dropped pixels; the labels carry no gradient; da and db must be two buffers);
 *                      hist [4 C + 1], exact integers: pixels per yA, pixels per yB, pixels with keepA per yA, pixels with
 *                      keepB per yB, pixels with yA == yB;
 *                      label_a, label_b (each may be NULL) uint8 [N][H][W]: keep ? y : 255.
 *                    Every sum is a fixed association (per thread in pixel order, wave butterfly, waves in order, workgroup
 *                    rows in index order by the last workgroup to take a ticket): all outputs are bitwise reproducible.  No
 *                    floating-point atomics; ONE launch and no memset; nothing is read back.  Shapes refused: N, H or W <= 0,
 *                    C outside [1, 16], N H W >= 2^31.  ws: spcl_cross_pseudo_workspace_bytes(N, C, H, W) bytes (0 for a
 *                    refused shape), 8-byte aligned, ZERO-FILLED BY THE CALLER BEFORE ITS FIRST USE: it holds the ticket,
 *                    which a completed call leaves at zero, so calls that follow one another on a stream may share it (the
 *                    entry zeroes nothing itself: a captured memset node did not keep its value over replays).
 *                    Captured with such a workspace that outlives the graph, every replay writes all outputs. */
size_t spcl_cross_pseudo_workspace_bytes(int N, int C, int H, int W);
int spcl_cross_pseudo_ce(const float* a_logits, const float* b_logits, int N, int C, int H, int W, const float* tau, float weight,
                         float* loss, float* parts, float* da, float* db, unsigned long long* hist, uint8_t* label_a,
                         uint8_t* label_b, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- CutMix for cross pseudo supervision (csrc/cutmix.hip) -------
 * The strong perturbation of CPS + CutMix (French et al., BMVC 2020; Chen et al., CVPR 2021), ABI 36; not in the reference.  One
 * box per sample, drawn on the device; inside box n the mixed sample n shows sample src = (n + roll) mod N, elsewhere itself.
 * Nothing is read back, every entry is one capturable launch, all outputs are bitwise reproducible, no floating-point atomics.
 *
 *   spcl_cutmix_boxes: boxes int32 [N][4] = (y0, x0, bh, bw): rows [y0, y0 + bh), columns [x0, x0 + bw) of an H x W image.
 *                    seed: ONE 32-bit word in device memory (read by the kernel: a captured call replays with what the word
 *                    holds then).  lo16 <= hi16: the range of the box's share of the image area in units of 1 / 65536.  With
 *                    key(i) = fmix32((((i + 1) * 0x9E3779B1) mod 2^32) ^ *seed) (spcl_pixel_sample's key), integers only and
 *                    every product in 64 bits:
 *                      r_j = key(4 n + j), j = 0 .. 3;  u_j = r_j >> 8
 *                      P = lo16 + (((hi16 - lo16) * u_0) >> 24)                        the area share
 *                      S = P + (((65536 - P) * u_1) >> 24);  T = (P * 65536) / S       the two side shares, S T ~ P 65536
 *                      (sh, sw) = (r_1 & 1) ? (S, T) : (T, S)
 *                      bh = min(H, max(1, (H * sh + 32768) >> 16));  bw = min(W, max(1, (W * sw + 32768) >> 16))
 *                      y0 = ((H - bh + 1) * u_2) >> 24;  x0 = ((W - bw + 1) * u_3) >> 24
 *                    (French et al.'s generator with a linear-uniform side share in place of the log-uniform one: no exp or
 *                    log, so a host restatement is exact; the fair bit r_1 & 1 keeps height and width symmetric.)  Every box
 *                    lies inside its image.  Refused: a null pointer, N outside [1, 2^20], H or W <= 0, not 1 <= lo16 <= hi16
 *                    <= 65536.
 *   spcl_cutmix_images: out[n][..][h][w] = x[src(n, h, w)][..][h][w], src = (n + roll) mod N inside box n and n elsewhere: a
 *                    pure copy (bit-identical to a select between x and its roll).  dtype SPCL_F32 / SPCL_BF16; channels_last
 *                    == 0: x and out are contiguous [N][C][H][W], else [N][H][W][C].  16-byte accesses where the contiguous
 *                    run of an image row (W, or W C, elements) is a multiple of 16 bytes and both pointers are aligned.
 *                    Refused: a null pointer, a bad dtype, a non-positive extent, N C H W >= 2^31, out == x (an in-place
 *                    gather races), roll outside [1, N - 1].  No index is formed from a box value.
 *   spcl_cross_pseudo_ce_mixed: spcl_cross_pseudo_ce with the labels read through the boxes.  s_a, s_b: the two networks'
 *                    logits on the MIXED images (they get the gradients da, db); t_a, t_b: their logits on the UNMIXED images
 *                    (constants); all four [N][H][W][C] f32, 1 <= C <= 16.  Per pixel (n, h, w) with m = src(n, h, w)
 *                    (boxes NULL: m = n, roll ignored):
 *                      yA = argmax_c t_a[m][h][w][c] (lowest class on a tie), confA = max softmax(t_a[m][h][w]) formed as
 *                      spcl_cross_pseudo_ce forms it (the same helper, the same bits), keepA = confA >= tau[yA] (tau NULL:
 *                      every numeric confidence keeps); yB, confB, keepB likewise from t_b;
 *                      term = keepB * -log softmax(s_a[n][h][w])[yB] + keepA * -log softmax(s_b[n][h][w])[yA];
 *                      loss[0] = weight / M * sum term, M = N H W; parts[0], parts[1] the two directions (s_a <- t_b, s_b <-
 *                      t_a); da = keepB ? weight / M * (softmax(s_a) - onehot(yB)) : 0, db likewise with keepA, yA (exact
 *                      zeros at dropped pixels; da and db must be two buffers);
 *                      hist [4 C + 2], exact integers: pixels per yA, pixels per yB, pixels with keepA per yA, pixels with
 *                      keepB per yB, pixels with yA == yB, pixels inside a box;
 *                      label_a, label_b (each may be NULL) uint8 [N][H][W] in the MIXED frame: keep ? y : 255.
 *                    (Mixing the teachers' logits with the binary mask and then taking the arg-max, as the official
 *                    implementation does, is this selection.)  Each map is read once, each soft-max formed once, no mixed
 *                    teacher map is written.  Sums in spcl_cross_pseudo_ce's association: with boxes NULL, t_a == s_a and
 *                    t_b == s_b every output is that entry's, bit for bit.  The sample read is n or (n + roll) mod N whatever
 *                    the boxes hold (unsigned range compares).  Refused: a null pointer, C outside [1, 16], N, H or W <= 0,
 *                    N H W >= 2^31, da == db, a short or not 8-byte aligned workspace and, with boxes given, roll outside
 *                    [1, N - 1] (so N >= 2).  ws: spcl_cross_pseudo_mixed_workspace_bytes(N, C, H, W) bytes (0 for a refused
 *                    shape), ZERO-FILLED BY THE CALLER BEFORE ITS FIRST USE and left with its ticket at zero by every
 *                    completed call, as spcl_cross_pseudo_ce's; ONE launch and no memset. */
int spcl_cutmix_boxes(const uint32_t* seed, int N, int H, int W, int lo16, int hi16, int32_t* boxes, void* stream);
int spcl_cutmix_images(const void* x, void* out, int dtype, int N, int C, int H, int W, int channels_last, const int32_t* boxes,
                       int roll, void* stream);
size_t spcl_cross_pseudo_mixed_workspace_bytes(int N, int C, int H, int W);
int spcl_cross_pseudo_ce_mixed(const float* s_a, const float* s_b, const float* t_a, const float* t_b, int N, int C, int H, int W,
                               const int32_t* boxes, int roll, const float* tau, float weight, float* loss, float* parts,
                               float* da, float* db, unsigned long long* hist, uint8_t* label_a, uint8_t* label_b, void* ws,
                               size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- strong intensity view (csrc/strong_view.hip) ----------------
 * The strong view of the unlabelled pair (FixMatch / UniMatch; the op family is nnU-Net's intensity augmentation), ABI 37; not
 * in the reference.  spcl_strong_view_params draws one row of 16 floats per sample; spcl_strong_view_apply is spcl_flip_batch
 * with the row's ops applied on the way.  Nothing is read back, each entry is one capturable launch, all outputs are bitwise
 * reproducible, no floating-point atomics.
 *
 *   table f32 [N][SPCL_SV_COLS = 16]:
 *     0 gamma   1 contrast c   2 brightness b   3 blur t   4 noise sigma      (the neutral value where the op is not applied)
 *     5 applied: sum of 2^k over the applied ops k, as a float   6 the sample's noise seed word, bit-cast
 *     7 m: the mean of sample n   8 the number of applied ops, as a float   9 .. 15 zero
 *
 *   spcl_strong_view_params: x [N][C][H][W] f32 / bf16 (read for the mean only); seed: ONE 32-bit word in device memory (read
 *                    by the kernel: a captured call replays with what the word holds then); cfg: 15 HOST words, for op k = 0
 *                    gamma, 1 contrast, 2 brightness, 3 blur, 4 noise: cfg[3 k] = p16_k, the gate probability in units of
 *                    1 / 65536 (0 .. 65536), cfg[3 k + 1], cfg[3 k + 2] = the bits of the f32 range ends lo_k, hi_k.  With
 *                    key(i) = pxs_key(i, *seed) (spcl_pixel_sample's key):
 *                      r_j = key(16 n + j), j = 0 .. 10;  u_j = r_j >> 8
 *                      op k is applied iff (r_{2k} & 0xFFFF) < p16_k
 *                      v_k = min(hi_k, lo_k + (hi_k - lo_k) * (float(u_{2k+1}) * 2^-24))
 *                    in f32: the difference, the product and the sum are each rounded to nearest once (no fused
 *                    multiply-add; the scaling by 2^-24 and the min are exact), so a float32 host restatement is bit-equal.
 *                    (The min only bites where the rounded difference carries the sum one spacing past hi_k.)  An op that is
 *                    not applied stores 1, 1, 1, 0, 0, bit-exact.  Column 6 = r_10.  Column 7: the C H W source elements of
 *                    sample n summed in float64 in a fixed association (thread t of 256 adds elements t, t + 256, ... in
 *                    order; the xor butterfly of the wave, offsets 32 .. 1; the four waves in order), divided by C H W,
 *                    rounded to f32 once.  One workgroup per sample.
 *                    Refused: a null pointer, a bad dtype, N outside [1, 2^20], a non-positive extent, C H W >= 2^31, p16
 *                    outside [0, 65536], lo > hi (or a NaN), gamma or brightness lo <= 0, contrast lo < 0, blur range outside
 *                    [0, 1], noise lo < 0.
 *   spcl_strong_view_apply: x, out contiguous [N][C][H][W] f32 / bf16, out != x; flags uint8 [N] as spcl_flip_batch (bit 0
 *                    flips H, bit 1 flips W).  For the output pixel p = (n, c, h, w) with the source pixel s = flip(p), in f32:
 *                      1  a = clamp(x[s], 0, 1);  a = powf(a, gamma_n), not taken (bit-exact) where gamma_n == 1
 *                      2  a = ((a - m_n) * c_n + m_n) * b_n
 *                      3  a = a + t_n * (B(a) - a), B the separable binomial filter [1 4 6 4 1] / 16 (dyadic weights) along W,
 *                         then along H, of the image after 1 - 2 with replicated edges: the coordinate is clamped before the
 *                         load, no index is formed from a table value.  The filter is symmetric and the edges replicate, so it
 *                         commutes with the flip: it is taken in the output frame.  Not taken where t_n == 0.
 *                      4  q = (c H + h) W + w (the OUTPUT frame);  k_i = pxs_key(2 q + i, seed word of n), i = 0, 1;
 *                         z = (k_0 & 0xFFFF) + (k_0 >> 16) + (k_1 & 0xFFFF) + (k_1 >> 16) - 131070  (an Irwin-Hall sum of four
 *                         16-bit uniforms, exact in an int; variance 4 (2^32 - 1) / 12);
 *                         a += (sigma_n * sqrt(3)_f32) * (float(z) * 2^-16): variance sigma_n^2 up to 2^-32 (the scaling of z
 *                         is exact; the last product and the sum may be one fused multiply-add).  Not taken where
 *                         sigma_n == 0.
 *                      5  out[p] = clamp(a, 0, 1), stored in dtype (bf16: round to nearest even).
 *                    A sample whose five values are all neutral is a pure copy (no clamp, no arithmetic): with every row
 *                    neutral the call is spcl_flip_batch, bit for bit.  A workgroup owns a SPCL_SV_TILE_H x SPCL_SV_TILE_W
 *                    tile of one (n, c) plane; with blur the tile and a halo of 2 are staged in LDS with steps 1 - 2 applied
 *                    at the load.  Where W elements are a multiple of 16 bytes and both pointers are 16-byte aligned a thread
 *                    loads and stores 16 bytes at a time (the halo staging of the blur reads element-wise), else element by
 *                    element.
 *                    Refused: a null pointer, a bad dtype, a non-positive extent, C H W >= 2^31 (and N C H W / 1024 tiles
 *                    past 2^31), out == x. */
#define SPCL_SV_COLS 16
#define SPCL_SV_TILE_H 16
#define SPCL_SV_TILE_W 64
int spcl_strong_view_params(const void* x, int dtype, int N, int C, int H, int W, const uint32_t* seed, const int32_t* cfg,
                            float* table, void* stream);
int spcl_strong_view_apply(const void* x, void* out, int dtype, int N, int C, int H, int W, const uint8_t* flags,
                           const float* table, void* stream);
int spcl_strong_view_tile(int* tile_h, int* tile_w);

#ifdef __cplusplus
}
#endif
#endif
