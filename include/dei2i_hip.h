/*
 * dei2i_hip.h -- C ABI of libdei2i_hip.so, the MI355X (gfx950) kernel library under the de-i2i-gan_amd
 * Python host code.
 *
 * The reference (jason2714/de-i2i-gan) has no FFI of its own: its hot path is Python calling ATen ops
 * implicitly.  Each entry point below therefore replaces the ATen op(s) issued at the cited reference
 * call sites (paths relative to /root/reference/defectGAN).  All functions:
 *   - take raw device pointers + plain ints, launch on the caller's hipStream_t, allocate nothing,
 *   - return 0 on success or a hipError_t / negative dei2i error code (the Python side raises RuntimeError),
 *   - activations are NHWC with the channel stride padded to a 16-byte vector (8 bf16 / 4 f32); `dtype`
 *     0 = bf16 storage + bf16 MFMA (fp32 accumulate), 1 = f32 storage + exact f32 MFMA (parity mode).
 */
#ifndef DEI2I_HIP_H
#define DEI2I_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dei2i_stream;   /* hipStream_t */

#define DEI2I_BF16 0
#define DEI2I_F32 1
#define DEI2I_ACT_NONE 0
#define DEI2I_ACT_RELU 1
#define DEI2I_ACT_LRELU 2      /* LeakyReLU(0.2), architecture.py:15 */
#define DEI2I_PAD_ZERO 0       /* also 'valid' when pad == 0 */
#define DEI2I_PAD_REFLECT 1

#define DEI2I_ERR_BAD_ARG (-2)
#define DEI2I_ERR_WORKSPACE (-3)

/* argument limits that the host code on both sides of this ABI checks */
#define DEI2I_EMBED_MAX_LABEL_NC 16   /* dei2i_embed_draw: the combination table has 1 << label_nc rows */
#define DEI2I_DIGEST_MAX_ROWS 65535   /* dei2i_state_digest: rows per launch (the grid's y extent) */

/* nn.Conv2d geometry (architecture.py:51-56,95-100,228-233,320-337; normalization.py:17-22;
 * discriminator.py:60-90).  `up` = 1 fuses the preceding nn.Upsample(scale_factor=2) (architecture.py:203). */
typedef struct dei2i_conv {
  int dtype;
  int N, H, W;          /* physical input extent (before the fused upsample) */
  int Cin, Cout;        /* logical channels */
  int CinS, CoutS;      /* channel strides of the x / y tensors (padded to the vector width) */
  int kh, kw, stride, pad, pad_mode, up;
} dei2i_conv;

/* ---- library / device ---- */
int dei2i_version(void);
int dei2i_init(int device);                         /* queries the CU count; optional */
const char* dei2i_error_string(int code);
/* A-B switches between shipped kernel families (1 = on, the default; 0 = off); any other name -> DEI2I_ERR_BAD_ARG:
 *   "gather_gemm_v2", "wgrad_v2", "halo_conv", "thin_conv", "wgrad_thin", "dgrad_s2_ring" = 0|1
 *   "wgrad_halo" = 0|1|2 (2: also on shapes too small to fill the chip)
 *   "halo16" = 0 (the 8 x 32 halo kernel only) | nonzero (the 16 x 32 halo kernels where they qualify)
 *   "halo16_fold" = 0|1 (reflect dgrads: ring folded inside the 16 x 32 kernel, or as separate launches)
 *   "halo16_s2" = 0|1|2 (4x4 stride-2 forward convs on the 16 x 32 kernel; 2: every channel count, not only 64) */
int dei2i_set_option(const char* name, int value);

/* ---- packed weight layouts (replaces nothing in the reference: layout prep for the kernels) ---- */
size_t dei2i_packed_fwd_elems(const dei2i_conv* c);      /* Cout * kh*kw * CinS */
size_t dei2i_packed_dgrad_elems(const dei2i_conv* c);    /* sum over stride^2 parity classes of Cin * taps * CoutS */
int dei2i_pack_weight_fwd(const dei2i_conv* c, const float* w_oihw, void* packed, dei2i_stream s);
int dei2i_pack_weight_dgrad(const dei2i_conv* c, const float* w_oihw, void* packed, dei2i_stream s);
/* both layouts in one launch (the training path: a weight is re-packed once per optimizer step) */
int dei2i_pack_weight_both(const dei2i_conv* c, const float* w_oihw, void* packed_fwd, void* packed_dgrad, dei2i_stream s);

/* ---- convolution (ATen convolution / convolution_backward) ---- */
void dei2i_conv2d_out_shape(const dei2i_conv* c, int* Ho, int* Wo);
/* dgrad output extent: reflect -> padded logical input (H<<up)+2*pad; zero -> logical input */
void dei2i_conv2d_dgrad_shape(const dei2i_conv* c, int* OH, int* OW);
size_t dei2i_conv2d_workspace_bytes(const dei2i_conv* c);   /* fp32 split-K workspace upper bound (fwd and dgrad) */
int dei2i_conv2d_fwd(const dei2i_conv* c, const void* x, const void* w_packed, const float* bias, int act, void* y,
                     float* ws, size_t ws_bytes, dei2i_stream s);
int dei2i_conv2d_dgrad(const dei2i_conv* c, const void* dy, const void* wd_packed, void* dx_ext, float* ws,
                       size_t ws_bytes, dei2i_stream s);
/* convolution_backward's grad_input in one call: dx (N,H,W,CinS) = the dgrad frame folded back onto the physical
 * input (reflection_pad2d_backward + upsample_nearest2d_backward).  ext_scratch: N*OH*OW*CinS elements of the compute
 * dtype (dei2i_conv2d_dgrad_shape), may be NULL for zero-padded convs without upsample.  Stride-1 reflect convs run
 * as interior GEMM (straight into dx) + reflect-ring GEMM + border fold; everything else as dgrad + dei2i_fold_pad. */
int dei2i_conv2d_dgrad_input(const dei2i_conv* c, const void* dy, const void* wd_packed, void* ext_scratch, void* dx,
                             float* ws, size_t ws_bytes, dei2i_stream s);
/* one wgrad slab: the packed [Cout][kh*kw][CinS] fp32 gradient with Cout rounded up to 8 rows (the kernels store
 * 8-row groups unguarded; the extra rows are never read) */
size_t dei2i_wgrad_slab_elems(const dei2i_conv* c);
/* wgrad straight to the OIHW fp32 gradient (what autograd hands to the optimizer).  scratch: fp32 device buffer of at
 * least dei2i_wgrad_slab_elems(c) floats; extra capacity lets the kernels split the pixel range over more
 * workgroups (one partial slab per split, summed and un-packed by a second kernel: no float atomics). */
/* accumulate != 0: dw_oihw += (a further use of the same weight in one backward pass adds into its gradient in place) */
int dei2i_conv2d_wgrad_oihw(const dei2i_conv* c, const void* x, const void* dy, float* scratch, size_t scratch_elems,
                            float* dw_oihw, int accumulate, dei2i_stream s);
/* ---- fp8 (OCP e4m3) forward of the stride-1 3x3 convolutions (BASELINE.json configs[4]) ----
 * c describes the convolution as usual (dtype = DEI2I_BF16: y, bias and the backward path are bf16 / fp32); x and the
 * packed weights are e4m3 bytes with the same NHWC / [Cout][9][CinS] layouts (CinS % 128 == 0).  fp32 accumulation;
 * y = act(dequant[0] * sum(xq * wq) + bias).  No fallback: unsupported shapes return an error, ask _supported first. */
int dei2i_conv2d_fp8_supported(const dei2i_conv* c);                       /* 1 / 0 */
/* out[i] = e4m3(clamp(x[i] * scale, +-448)); n % 8 == 0 */
int dei2i_quantize_fp8(size_t n, const void* x_bf16, float scale, void* out_e4m3, dei2i_stream s);
/* packed forward weights in e4m3: w_oihw * (448 / amax[0]) (amax: device scalar max|w|); also writes the conv's
 * dequant[0] = 1 / (act_scale * 448 / amax[0]), act_scale being the scale the activations are quantised with */
int dei2i_pack_weight_fwd_fp8(const dei2i_conv* c, const float* w_oihw, const float* amax, float act_scale, void* packed_e4m3,
                              float* dequant, dei2i_stream s);
int dei2i_conv2d_fwd_fp8(const dei2i_conv* c, const void* x_e4m3, const void* w_e4m3, const float* bias, const float* dequant,
                         int act, void* y_bf16, dei2i_stream s);
/* reflection_pad2d_backward + upsample_nearest2d_backward: fold the dgrad output (N,OH,OW,C) back onto the
 * physical input (N,H,W,C); optional addend (residual-branch gradient) is summed in the same pass. */
int dei2i_fold_pad(int dtype, int N, int H, int W, int C, int pad, int pad_mode, int up, const void* dx_ext,
                   const void* addend, void* dx, dei2i_stream s);

/* ---- layout at the module boundary (NCHW fp32 <-> NHWC compute dtype) ----
 * Cs: the NHWC channel stride, >= C and a multiple of the 16-byte vector (8 in bf16, 4 in f32) in all three. */
int dei2i_nchw_to_nhwc(int dtype, int N, int C, int H, int W, int Cs, const float* src, void* dst, dei2i_stream s);
int dei2i_nhwc_to_nchw(int dtype, int N, int C, int H, int W, int Cs, const void* src, float* dst, dei2i_stream s);
/* same as nchw_to_nhwc with F.interpolate(mode='nearest') from (hs,ws) to (H,W) fused (SPADE label map,
 * normalization.py:29) */
int dei2i_nchw_to_nhwc_resize(int dtype, int N, int C, int hs, int ws, int H, int W, int Cs, const float* src, void* dst,
                              dei2i_stream s);

/* ---- per-channel moments (native_batch_norm statistics; generator.py:71,113,124; normalization.py:14) ----
 * partial: (N, chunks, 2, C) fp32 sums / sums of squares.  chunks = dei2i_moments_chunks(HW). */
int dei2i_moments_chunks(int HW);
int dei2i_moments_partial(int dtype, int N, int HW, int C, const void* x, float* partial, dei2i_stream s);
/* ---- BatchNorm groups: a batch that carries several passes takes statistics, apply and backward per GROUP of the batch, one launch
 * for all groups (the paired generator passes of the G loss: defectgan_model.py:185-190 as two passes over 2 x batch); groups = 1 is
 * plain BatchNorm over the whole batch.  N / pixels are PER GROUP, the groups are consecutive in the activation tensors, mean / rstd /
 * a / b hold one row of C per group, the statistics records one block per group. ---- */
/* BatchNorm2d train: batch stats over (N,HW) from `chunks` records per image -> scale/shift a[c], b[c]; mean/rstd saved for backward;
 * running stats (both or neither, may be NULL; group g's at + g * running_stride floats) updated (momentum 0.1, unbiased var).
 * num_batches_tracked (int64 device scalar, may be NULL) is incremented once by the same launch. */
int dei2i_bn_finalize_train(int groups, int N, int HW, int C, int chunks, const float* partial, const float* weight, const float* bias,
                            float* running_mean, float* running_var, int running_stride, float momentum, float eps, float* mean,
                            float* rstd, float* a, float* b, long long* num_batches_tracked, dei2i_stream s);
int dei2i_bn_finalize_eval(int C, const float* weight, const float* bias, const float* running_mean,
                           const float* running_var, float eps, float* a, float* b, dei2i_stream s);
/* InstanceNorm2d(affine=False): per (n,c) mean / rstd, fp32 [N][C], from `chunks` records per image */
int dei2i_in_finalize(int N, int HW, int C, int chunks, const float* partial, float eps, float* mean, float* rstd, dei2i_stream s);

/* ---- fused normalisation + activation, forward ---- */
/* out = act(a[c]*x + b[c]) (+ res)   -- BatchNorm apply + LeakyReLU (+ ResBlock identity), architecture.py:116-118,174-176 */
/* out_e4m3 (bf16 only, may be NULL): also write e4m3(out * e4m3_scale) -- the operand copy of the fp8 forward mode */
int dei2i_affine_act_fwd(int dtype, int groups, size_t pixels, int C, const void* x, const float* a, const float* b, const void* res,
                         int act, void* out, void* out_e4m3, float e4m3_scale, dei2i_stream s);
/* the same, also writing the statistics records of its output: partial (N, dei2i_moments_chunks(HW), 2, C); N: the whole batch */
int dei2i_affine_act_stats_fwd(int dtype, int groups, int N, int HW, int C, const void* x, const float* a, const float* b,
                               const void* res, int act, void* out, float* partial, dei2i_stream s);
/* SPADE + ReLU (normalization.py:24-37, architecture.py:241-245,343-350):
 *   out[n,h,w,c] = relu( (x[n,h>>up,w>>up,c] - mean[n,c]) * rstd[n,c] * (1 + gamma) + beta ) (+ nothing)
 * gb is (N, Hg, Wg, 2*C): gamma = [..., :C], beta = [..., C:].  gb_mode 0: Hg x Wg == output extent;
 * gb_mode 1: Hg = Wg = 5 "border class" table (labels constant over space; class = min(i,2) / 4-(H-1-i)). */
int dei2i_spade_act_fwd(int dtype, int N, int H, int W, int C, int up, const void* x, const float* mean,
                        const float* rstd, const void* gb, int gb_mode, void* out, void* out_e4m3, float e4m3_scale, dei2i_stream s);

/* ---- backward of the above ---- */
/* g = dz * act'(z) (LeakyReLU / ReLU expressed through the saved output z) */
int dei2i_act_bwd(int dtype, size_t n, const void* dz, const void* z, int act, void* g, dei2i_stream s);
/* column sums: out[c] = sum over rows of g[row][c]   (conv bias gradient).  Two deterministic stages (no atomics):
 * partial is fp32 scratch of dei2i_colsum_blocks(rows) * C floats. */
int dei2i_colsum_blocks(size_t rows);
int dei2i_colsum(int dtype, size_t rows, int C, const void* g, float* partial, float* out, dei2i_stream s);
/* BatchNorm backward (train): z = act(a*y+b); g = dz*act'(z); needs sum(g), sum(g*xhat) per channel and group.
 * bn_bwd_partial writes (groups, chunks, 2, C) partial sums over each group's `pixels` rows; bn_bwd_apply finishes:
 *   dy = a * (g - sum_g/M - xhat * sum_gx/M) with the group's own sums (group_sums: (groups, 2, C) floats of scratch),
 *   dweight = sum_gx, dbias = sum_g totalled over the groups -- written, or added to when `accumulate` (a further use of the same
 *   parameters in this backward pass).   train = 0 -> dy = a*g. */
int dei2i_bn_bwd_chunks(size_t pixels);
int dei2i_bn_bwd_partial(int dtype, int groups, size_t pixels, int C, const void* dz, const void* y, const float* a, const float* b,
                         const float* mean, const float* rstd, int act, float* partial, dei2i_stream s);
int dei2i_bn_bwd_apply(int dtype, int groups, size_t pixels, int C, const void* dz, const void* y, const float* a, const float* b,
                       const float* mean, const float* rstd, int act, int train, const float* partial, int chunks,
                       float* group_sums, float* dweight, float* dbias, int accumulate, void* dy, dei2i_stream s);
/* ---- BatchNorm over a batch that is sharded across processes (synchronised BatchNorm; ops.bn_sync) ----
 * The two finalize steps above, each cut in two at the point where the ranks exchange: stage 1 turns this process's records into one
 * small fp64 message, the caller SUMS the messages of all ranks (all-reduce), stage 2 finishes from the summed message.  Records,
 * groups, coefficient rows, running buffers (running_stride) and num_batches_tracked are those of dei2i_bn_finalize_train /
 * dei2i_bn_bwd_apply; N, HW, pixels are THIS process's.  No atomics: the fp64 combine runs in record order.
 *   fwd_sums:     msg (groups, 2*C + 1) doubles = sum x | sum x^2 | the group's element count (N * HW)
 *   fwd_finalize: mean / rstd / a / b, running update (unbiased variance with the summed count) and the counter from the summed msg
 *   bwd_sums:     sums (groups, 2, C) doubles = sum g*xhat | sum g per group; dweight / dbias = THIS process's total over its groups
 *                 (written, or added when `accumulate`) -- local on purpose: parameter gradients are summed over ranks afterwards
 *   bwd_apply:    dy from the summed sums and `count` = the group's pixels over all ranks (`pixels`: this process's, sizes the launch);
 *                 group_sums: (groups, 2, C) floats of scratch */
int dei2i_bn_sync_fwd_sums(int groups, int N, int HW, int C, int chunks, const float* partial, double* msg, dei2i_stream s);
int dei2i_bn_sync_fwd_finalize(int groups, int C, const double* msg, const float* weight, const float* bias, float* running_mean,
                               float* running_var, int running_stride, float momentum, float eps, float* mean, float* rstd, float* a,
                               float* b, long long* num_batches_tracked, dei2i_stream s);
int dei2i_bn_sync_bwd_sums(int groups, int C, const float* partial, int chunks, double* sums, float* dweight, float* dbias,
                           int accumulate, dei2i_stream s);
int dei2i_bn_sync_bwd_apply(int dtype, int groups, size_t pixels, size_t count, int C, const void* dz, const void* y, const float* a,
                            const float* b, const float* mean, const float* rstd, int act, const double* sums, float* group_sums,
                            void* dy, dei2i_stream s);
/* SPADE-family backward.  z = act(v), v = xhat*(1+gamma)+beta, act of the ReLU family with negative slope `slope` (0: SPADE's
 * ReLU, 0.2: LeakyReLU, 1: none), is RECOMPUTED from x and the gamma/beta table in both passes (the op keeps neither its output
 * nor a dxhat tensor): g = dz*(v>0 ? 1 : slope); dgamma = g*xhat, dbeta = g -> dgb (T: dense tensor, or the (N,5,5,2C)
 * border-class table -- its 24 border classes are written by pass 1, the interior class by pass 2); partial (N, chunks, 4, C)
 * fp32 sums of dxhat = g*(1+gamma), dxhat*xhat and the interior-class dgamma / dbeta.  chunks = dei2i_moments_chunks(H*W of the
 * OUTPUT).  In class mode dgb may be NULL: no table gradient is wanted, its border classes are not reduced (pass 2 is then
 * given dgb_cls = NULL).  The same two passes are the backward of
 *   z = act(InstanceNorm2d(x)), affine=False (extractor.py:50-80 with architecture.py:79-176): class mode on an all-zero
 *     (N,5,5,2C) table, dgb = NULL, up = 0;
 *   z = act(IN(x) * (1 + gamma) + beta) with per-(n, c) gamma / beta -- AdaIN (stargan-v2/core/model.py:69-80) and
 *     InstanceNorm2d(affine=True) (model.py:39-40,56-61,333-334: gamma = weight - 1, beta = bias): class mode on a table that holds
 *     the same (gamma | beta) in all 25 classes; the caller sums the 25 classes of dgb.  Forward of both: dei2i_in_finalize +
 *     dei2i_affine_act_img_fwd with A = rstd (1 + gamma), B = beta - mean A. */
int dei2i_spade_bwd_partial(int dtype, int N, int H, int W, int C, int up, const void* dz, const void* x, const float* mean,
                            const float* rstd, const void* gb, int gb_mode, float slope, void* dgb, float* partial, dei2i_stream s);
/* pass 2 (finalize + apply): dx = rstd*(sum_cell dxhat - cnt*mean(dxhat) - cnt*xhat*mean(dxhat*xhat)) (+ addend).
 * coef: fp32 scratch (N,2,C).  dgb_cls: the class-mode (N,5,5,2C) table of pass 1 (its interior class is written here), or NULL. */
int dei2i_spade_bwd_apply(int dtype, int N, int H, int W, int C, int up, const void* dz, const void* x, const float* mean,
                          const float* rstd, const void* gb, int gb_mode, float slope, const float* partial, int chunks,
                          void* dgb_cls, float* coef, const void* addend, void* dx, dei2i_stream s);

/* ---- generator heads + compose (generator.py:266-275) ----
 * raw: (N,H,W,Cs>=4) = [fg_pre(3), prob_pre(1)]; x_in, out: NCHW fp32 (N,3,H,W); prob: NCHW fp32 (N,1,H,W)
 *   out = x*(1-p) + tanh(fg_pre)*p,  p = sigmoid(prob_pre) */
int dei2i_compose_fwd(int dtype, int N, int H, int W, int Cs, const void* raw, const float* x_in, float* out, float* prob,
                      dei2i_stream s);
int dei2i_compose_bwd(int dtype, int N, int H, int W, int Cs, const void* raw, const float* x_in, const float* d_out,
                      const float* d_prob, void* d_raw, float* d_x, dei2i_stream s);
/* NaN guard (generator.py:266-267): flag = any(isnan(x)); then, only if flag: nan->0, +-inf->+-max. No host sync. */
int dei2i_nan_guard(int dtype, size_t n, void* x, int* flag, dei2i_stream s);

/* ---- losses (models/base_model.py:68-80), fp32 tensors ---- */
/* mean( max(x,0) - x*t + log1p(exp(-|x|)) ); target == NULL -> constant `tconst`.  out[0] = loss, summed through ordered
 * block partials (no atomics: bit-reproducible; `out` needs no zero fill). */
int dei2i_bce_logits_fwd(size_t n, const float* x, const float* target, float tconst, float* out, dei2i_stream s);
int dei2i_bce_logits_bwd(size_t n, const float* x, const float* target, float tconst, const float* gout, float* dx,
                         dei2i_stream s);
/* mean |a - b| ; b == NULL -> 0; out[0] = loss.  backward: da = sign(a-b)*gout/n, db = -da (either may be NULL) */
int dei2i_l1_fwd(size_t n, const float* a, const float* b, float* out, dei2i_stream s);
int dei2i_l1_bwd(size_t n, const float* a, const float* b, const float* gout, float* da, float* db, dei2i_stream s);
/* mean (a - b)^2 ; b == NULL -> the constant `bconst`; out[0] = loss (ordered block partials, like the two above).
 * backward: da = 2*(a-b)*gout/n, db = -da (either may be NULL) */
int dei2i_mse_fwd(size_t n, const float* a, const float* b, float bconst, float* out, dei2i_stream s);
int dei2i_mse_bwd(size_t n, const float* a, const float* b, float bconst, const float* gout, float* da, float* db,
                  dei2i_stream s);
/* The `cce` kind of the same helper (the reference tree is not part of this repository, so the
 * function is stated here): torch.nn.functional.cross_entropy(x, target), mean reduction, x (rows, classes) with the class
 * dimension last and contiguous, target a float tensor of the same shape (class weights):
 *   out[0] = 1/rows * sum_r sum_c t[r][c] * (lse_r - x[r][c]),  lse_r = m_r + log sum_c exp(x[r][c] - m_r),  m_r = max_c x[r][c]
 * For one-hot rows this is the class-index form; multi-hot and all-zero rows are legal (a row weighs S_r = sum_c t[r][c]).
 * The row maximum is subtracted before exp (logits of magnitude 1e4 give finite results); ordered partials + finalize, no
 * atomics: out[0] is written, needs no zero fill, and two runs give the same bits.  `classes` has no cap (one wavefront per
 * row, its lanes loop over the classes).
 * backward: dx[r][c] = gout/rows * (S_r * softmax_r[c] - t[r][c]); the target gets no gradient. */
int dei2i_cce_logits_fwd(size_t rows, int classes, const float* x, const float* target, float* out, dei2i_stream s);
int dei2i_cce_logits_bwd(size_t rows, int classes, const float* x, const float* target, const float* gout, float* dx,
                         dei2i_stream s);

/* ---- NoiseInjection (models/networks/architecture.py:374-389, the 'constant' weight the blocks use) ----
 * x, out, dy: NHWC activations viewed as [rows = N*H*W][C] in the compute dtype (C a multiple of 8 for bf16, 4 for fp32);
 * noise: one fp32 N(0,1) value per row; weight: the module's single fp32 scalar (device pointer).
 * fwd: out[r][c] = x[r][c] + weight * noise[r].  bwd: dweight[0] = sum_r noise[r] * sum_c dy[r][c] (ordered block partials:
 * `partials` holds >= 1024 floats of scratch; accumulate != 0 adds into dweight); the activation gradient is dy itself. */
int dei2i_noise_fwd(int dtype, size_t rows, int C, const void* x, const float* noise, const float* weight, void* out,
                    dei2i_stream s);
int dei2i_noise_bwd(int dtype, size_t rows, int C, const void* dy, const float* noise, float* partials, float* dweight,
                    int accumulate, dei2i_stream s);

/* ---- fused multi-tensor Adam (torch.optim.Adam semantics; trainers/base_trainer.py:75-89) ----
 * table: device array of `count` records {p, g, m, v (fp32*), n (int64)}; one launch updates all. */
typedef struct dei2i_adam_rec {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
} dei2i_adam_rec;
int dei2i_adam_step(const dei2i_adam_rec* table_dev, int count, int64_t max_n, float lr, float beta1, float beta2,
                    float eps, float bias_c1, float bias_c2_sqrt, float grad_scale, float decoupled_decay, dei2i_stream s);
/* decoupled_decay: AdamW's weight decay (p *= 1 - lr*decay before the Adam update); 0 = torch.optim.Adam */
/* torch.optim.SGD (kind 0: p -= lr*g) / torch.optim.RMSprop (kind 1: sq = alpha*sq + (1-alpha)*g^2 in rec.m; p -= lr*g/(sqrt(sq)+eps))
 * as trainers/base_trainer.py:71-74 constructs them (lr only: torch's defaults otherwise); same pointer table, rec.v unused */
int dei2i_sgd_rmsprop_step(const dei2i_adam_rec* table_dev, int count, int64_t max_n, int kind, float lr, float alpha, float eps,
                           float grad_scale, dei2i_stream s);

/* torch.optim.Adam's coupled weight decay inside the Adam update: the gradient is g * grad_scale + weight_decay * p (p.grad is not
 * written); otherwise dei2i_adam_step with decoupled_decay 0 */
int dei2i_adam_step_l2(const dei2i_adam_rec* table_dev, int count, int64_t max_n, float lr, float beta1, float beta2, float eps,
                       float bias_c1, float bias_c2_sqrt, float grad_scale, float weight_decay, dei2i_stream s);
/* The same two updates with (lr, bias_c1, bias_c2_sqrt, keep) read from row *index_dev of hyper_dev (`rows` rows of 4 floats; keep =
 * 1 - lr*decoupled_decay, unused by the _l2 form) -- the form a captured graph replays, the host rewriting the rows between replays.
 * Bit-identical to the argument forms given the same floats; an index outside [0, rows) leaves every tensor untouched. */
int dei2i_adam_step_dev(const dei2i_adam_rec* table_dev, int count, int64_t max_n, const float* hyper_dev, const int* index_dev,
                        int rows, float beta1, float beta2, float eps, float grad_scale, dei2i_stream s);
int dei2i_adam_step_l2_dev(const dei2i_adam_rec* table_dev, int count, int64_t max_n, const float* hyper_dev, const int* index_dev,
                           int rows, float beta1, float beta2, float eps, float grad_scale, float weight_decay, dei2i_stream s);
/* ---- global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, L2, error_if_nonfinite=False) on g * grad_scale, without
 * writing a gradient: the clip coefficient is folded into the scale the Adam update multiplies every gradient by anyway.
 * dei2i_grad_sumsq: one launch over a table (only rec.g and rec.n are read), grid = dei2i_grad_sumsq_blocks(max_n) x count;
 * every workgroup stores the fp32 sum of g^2 over its share to partial_dev[row * blocks + block] (0 where it had none), in a fixed
 * order: no clearing, no atomics, bit-reproducible.  Several tables append their partials in one buffer. */
int dei2i_grad_sumsq_blocks(int64_t max_n);
int dei2i_grad_sumsq(const dei2i_adam_rec* table_dev, int count, int64_t max_n, float* partial_dev, dei2i_stream s);
/* One workgroup: S = the sum of the n_partials partials in double; out_dev[0] = (float)(sqrt(S) * grad_scale), the norm of the
 * gradients the optimizer applies; out_dev[1] = grad_scale * min(1, max_norm / (out_dev[0] + 1e-6f)) in float (a NaN stays NaN).
 * max_norm must be > 0. */
int dei2i_grad_clip_finalize(const float* partial_dev, int n_partials, float grad_scale, float max_norm, float* out_dev,
                             dei2i_stream s);
/* dei2i_adam_step / dei2i_adam_step_l2 (coupled != 0; weight_decay is then the L2 one, else the decoupled one) and their _dev
 * forms with grad_scale = *scale_dev (out_dev + 1 of dei2i_grad_clip_finalize): bit-identical to them when *scale_dev holds the
 * grad_scale they were given. */
int dei2i_adam_step_clip(const dei2i_adam_rec* table_dev, int count, int64_t max_n, float lr, float beta1, float beta2, float eps,
                         float bias_c1, float bias_c2_sqrt, const float* scale_dev, int coupled, float weight_decay, dei2i_stream s);
int dei2i_adam_step_clip_dev(const dei2i_adam_rec* table_dev, int count, int64_t max_n, const float* hyper_dev, const int* index_dev,
                             int rows, float beta1, float beta2, float eps, const float* scale_dev, int coupled, float weight_decay,
                             dei2i_stream s);
/* ---- state digest: every 32-bit word of a list of device tensors reduced to one 64-bit word, integer arithmetic mod 2^64:
 *   digest = sum_k sum_i splitmix64(splitmix64((k << 32) | i) + w[k][i]),  splitmix64(x): x += 0x9E3779B97F4A7C15;
 *   x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^= x >> 31
 * Row r of the table is tensor k = row0 + r: rec.p its memory (4-byte aligned), rec.n its count of 32-bit words (<= 2^32, like
 * max_n); rec.g / m / v are not read.  One launch over the table, grid = dei2i_state_digest_blocks(max_n) x count (count <= DEI2I_DIGEST_MAX_ROWS),
 * every workgroup storing its partial to partial_dev[row * blocks + block] (count * blocks words of scratch; no clearing, no
 * atomics), then one workgroup: out_dev[0] = (accumulate ? out_dev[0] : 0) + the sum of the partials.  A long list goes out in
 * several calls on one stream: row0 = the rows before, accumulate = 1 from the second call on; partial_dev may be the same. */
int dei2i_state_digest_blocks(int64_t max_n);
int dei2i_state_digest(const dei2i_adam_rec* table_dev, int count, int64_t max_n, int64_t row0, uint64_t* partial_dev, int accumulate,
                       uint64_t* out_dev, dei2i_stream s);
/* *index_dev += 1 (one thread): captured after a _dev update, it moves the next replay to the next row */
int dei2i_index_advance(int* index_dev, dei2i_stream s);
/* EMA of a network's parameters in place, one launch (stargan-v2 moving_average, core/solver.py:549-551): rec.p = the EMA copy,
 * rec.g = the trained parameter, rec.m / rec.v unused; p = torch.lerp(g, p, weight) with torch.lerp's two-sided formula */
int dei2i_ema_lerp(const dei2i_adam_rec* table_dev, int count, int64_t max_n, float weight, dei2i_stream s);
/* The same update with weight = weights_dev[*index_dev] (`rows` floats) -- the form a captured graph replays, the host rewriting the
 * rows between replays and dei2i_index_advance moving the index.  Bit-identical to the argument form given the same float; an
 * index outside [0, rows) leaves every tensor untouched. */
int dei2i_ema_lerp_dev(const dei2i_adam_rec* table_dev, int count, int64_t max_n, const float* weights_dev, const int* index_dev,
                       int rows, dei2i_stream s);

/* ---- DiffAugment (utils/diffaug.py) on fp32 NCHW images: one canonical-order policy run (color -> translation -> cutout) as
 * y = Cut . Trans . (L x + beta) per sample, L(x)[c] = a x[c] + b mean_c(x) + k mean_chw(x) (csrc/diffaug.hip).
 * tab: device array of N records; a = 1, b = k = beta = 0 without color, ty = tx = 0 without translation, ch = cw = 0 without
 * cutout (the cut window is rows [top, top + ch) x cols [left, left + cw)).  mode 0: forward; 1: forward without beta (linear part);
 * 2: adjoint (input gradient of src = the output gradient).  partial: dei2i_diffaug_partial_floats(N) floats when color != 0.
 * Deterministic (fixed-order reductions, no atomics).
 * One row of a run WITH cutout is left uncut by top = H, left = W (ch and cw belong to the run, not to the row): the window
 * [H, H + ch) x [W, W + cw) lies off the image, and in_hole / fwd_valid of csrc/diffaug.hip only test coordinates inside it, in
 * all three modes (dei2i_diffaug_draw_p writes such rows). */
typedef struct dei2i_diffaug_rec {
  float a, b, k, beta;
  int ty, tx, top, left;
} dei2i_diffaug_rec;
size_t dei2i_diffaug_partial_floats(int N);
int dei2i_diffaug(int mode, int N, int C, int H, int W, int ch, int cw, int color, const float* src, const dei2i_diffaug_rec* tab,
                  float* partial, float* dst, dei2i_stream s);
/* Fill tab[run][n] (runs x N records, n in [0, N)) on the device, as utils.diffaug.draw_params fills it on the host, from
 * Philox4x32-10: key = seed, counter words = (call low 32, call high 32, run | block << 16, row0 + n), call = *counter_dev as the
 * launch finds it; block 0 gives rb, rs, rc (x0..x2, float = (x >> 8) * 2^-24), block 1 ty, tx, cy, cx (x0..x3, integer in
 * [lo, lo + range) = lo + mulhi(x, range)).  run_flags: 3 bits per run, run r at bits [3r, 3r + 3), the policies the run holds; a
 * field whose policy is absent holds the identity.  One launch of one workgroup; it leaves *counter_dev (one 64-bit word of device
 * memory) greater by exactly 1 -- launches that share a counter must be ordered on one stream (or one captured graph).  The draw is
 * a pure function of (seed, call, run, row0 + n): rows [row0, row0 + N) of a call are that slice of the same call made for the
 * whole batch. */
#define DEI2I_DIFFAUG_COLOR 1
#define DEI2I_DIFFAUG_TRANSLATION 2
#define DEI2I_DIFFAUG_CUTOUT 4
#define DEI2I_DIFFAUG_MAX_RUNS 16
int dei2i_diffaug_draw(uint64_t seed, uint64_t* counter_dev, int runs, uint64_t run_flags, int N, int row0, int H, int W,
                       dei2i_diffaug_rec* tab, dei2i_stream s);
/* The same table with a gate per row and policy (adaptive discriminator augmentation): blocks 0 and 1 give the parameters exactly
 * as above, block 2 (counter word run | 2 << 16) gives three gate floats on the same grid, x0 for color, x1 for translation, x2
 * for cutout, and a policy of the run applies to the row iff (x >> 8) * 2^-24 < *p_dev (one fp32 word of device memory in [0, 1],
 * read by the launch: nothing crosses to the host).  A policy that does not apply leaves its identity in the record: a = 1,
 * b = k = beta = 0; ty = tx = 0; top = H, left = W.  The cut size ch x cw is an argument of dei2i_diffaug for the whole run, so
 * the empty window is the window moved off the image: rows [H, H + ch) x cols [W, W + cw) hold no pixel (i, j) or source
 * (i + ty, j + tx) of an H x W image, whatever the mode -- every hole test is made on coordinates inside the image.  p = 1 gives the
 * table of dei2i_diffaug_draw for the same (seed, call, run, row) bit for bit, p = 0 identity records only, and a row's parameters
 * do not depend on its gates.  One launch of one workgroup, no atomics; *counter_dev advances by exactly 1 under the ordering rule
 * above.  BAD_ARG: as dei2i_diffaug_draw, and a null p_dev. */
int dei2i_diffaug_draw_p(uint64_t seed, uint64_t* counter_dev, int runs, uint64_t run_flags, int N, int row0, int H, int W,
                         const float* p_dev, dei2i_diffaug_rec* tab, dei2i_stream s);

/* ---- the pixel-blitting policies (utils/diffaug.py: flip -> rot90; csrc/blit.hip) on fp32 NCHW images: per sample one element of
 * the dihedral group, code = f | k << 1 -- f = 1 mirrors left-right, then k quarter turns as torch.rot90(x, k, dims=(2, 3)).
 * codes_dev: N int32 words of device memory; the launch uses word & 7 and takes k = 0 when H != W, so no table, whatever it holds,
 * moves a read or a write outside the two N*C*H*W buffers.  inverse != 0 applies each sample's inverse element ((1, k) when f = 1,
 * (0, (4 - k) & 3) when f = 0): the adjoint of the forward, which is a permutation.  Even k copies rows (reversed or not; float4
 * when W % 4 == 0 and both pointers are 16-byte aligned), odd k transposes 32 x 32 tiles through LDS; the pattern is uniform within
 * a workgroup.  Deterministic, no atomics, one launch.  BAD_ARG: null pointers, N, C, H, W <= 0, N*C*H*W >= 2^40,
 * C*H*W >= 2^31 (the limits of dei2i_diffaug), and src and dst that overlap (in place is not supported). */
int dei2i_blit(int N, int C, int H, int W, const int* codes_dev, int inverse, const float* src, float* dst, dei2i_stream s);
/* Fill codes[b][n] (blit runs x N words, b counting the blit runs of the list in order, n in [0, N)) on the device from
 * Philox4x32-10: key = seed, counter words = (call low 32, call high 32, run | 3 << 16, row0 + n), run the run's index in the WHOLE
 * run list of the policy (blocks 0..2 of that word belong to dei2i_diffaug_draw); f = x0 >> 31, k = mulhi(x1, 4).  run_flags: 2 bits
 * per run of the whole list, run r at bits [2r, 2r + 2): the blit policies the run holds, 0 for a color / translation / cutout run
 * (no row in the table); a policy that is absent leaves its bits 0.  One launch of one workgroup, no atomics; it leaves *counter_dev
 * greater by exactly 1 under the ordering rule of dei2i_diffaug_draw, whose counter it shares: a diff_augment call with both kinds
 * of run launches dei2i_diffaug_draw FIRST (it sees call) and dei2i_blit_draw SECOND (it sees call + 1); a call with blit runs only
 * launches dei2i_blit_draw alone (call).  A pure function of (seed, call, run, row0 + n): rows [row0, row0 + N) are that slice of the
 * whole-batch call.  BAD_ARG: null pointers, runs outside 1..DEI2I_DIFFAUG_MAX_RUNS, flag bits beyond the runs, no blit run, N <= 0,
 * row0 < 0, row0 + N > 2^31, runs * N >= 2^24. */
#define DEI2I_BLIT_FLIP 1
#define DEI2I_BLIT_ROT90 2
int dei2i_blit_draw(uint64_t seed, uint64_t* counter_dev, int runs, uint64_t run_flags, int N, int row0, int* codes, dei2i_stream s);
/* The same table with a gate per row and policy: flip applies iff (x2 >> 8) * 2^-24 < *p_dev and rot90 iff (x3 >> 8) * 2^-24 <
 * *p_dev, x2 and x3 of the same Philox block; a policy that does not apply leaves its bits 0.  p = 1 gives the table of
 * dei2i_blit_draw bit for bit, p = 0 zeros only, and a row's f and k do not depend on its gates.  BAD_ARG: as dei2i_blit_draw, and a
 * null p_dev. */
int dei2i_blit_draw_p(uint64_t seed, uint64_t* counter_dev, int runs, uint64_t run_flags, int N, int row0, const float* p_dev,
                      int* codes, dei2i_stream s);

/* ---- the geometric policies (utils/diffaug.py: scale -> rotate -> aniso; csrc/warp.hip) on fp32 NCHW images: per sample ONE bilinear
 * resampling with a 2x2 matrix about the image centre.  With cx = (W - 1) / 2, cy = (H - 1) / 2, dx = j - cx, dy = i - cy, output
 * pixel (i, j) samples the input at
 *   u = (m00 dx + m01 dy) + (cx + tu),   v = (m10 dx + m11 dy) + (cy + tv)
 * in fp32, in exactly this association, without contraction; u0 = floor(u), fu = u - u0 (v alike) and
 *   dst[i][j] = ((t0 + t1) + t2) + t3,  t = weight * tap over (v0, u0), (v0, u0 + 1), (v0 + 1, u0), (v0 + 1, u0 + 1) with the weights
 *   (1 - fv)(1 - fu), (1 - fv) fu, fv (1 - fu), fv fu; a tap outside the image gives t = 0 (zero fill) and nothing is read for it.
 * The pixel is 0 when u or v is not finite or lies outside [-1, W) x [-1, H), tested in floating point before any conversion.
 * adjoint != 0 is the exact transpose with the forward's own weights: dst[y][x] = sum of weight(i, j -> y, x) * src[i][j] over the
 * output pixels (i, j) in ascending row-major order, starting from 0, the weight recomputed from (i, j) by the forward's function.
 * One thread owns one input pixel and searches a box of at most 19 x 19 output pixels: a gather, no atomics, one launch,
 * deterministic in both directions.
 * USABLE records: the six floats are finite, |m| <= 4 for each of the four matrix entries, and with det = m00 m11 - m01 m10 (in
 * double: both products exact, one rounding) det != 0 and |m| <= 4 |det| for each entry, i.e. every entry of the inverse is at most
 * 4 in magnitude -- that bounds the box.  A record that is not usable is applied as the IDENTITY (1, 0, 0, 1, 0, 0) in both
 * directions.  Drawn matrices have entries and inverse entries of at most 2 and never meet the gate.  No table, whatever it holds,
 * moves a read or a write outside the two N*C*H*W buffers, and every loop ends within the box bound.  tab_dev: N records of device
 * memory, each DEI2I_WARP_REC_WORDS = 8 32-bit words (32 bytes, the size of a dei2i_diffaug_rec: one upload carries both kinds):
 * the fp32 words m00, m01, m10, m11, tu, tv, then two pad words that the launch does not read.  BAD_ARG: null pointers,
 * N, C, H, W <= 0, N*C*H*W >= 2^40, C*H*W >= 2^31 (the limits of dei2i_diffaug), H or W > 2^16 (the size up to which the box
 * provably holds every contributing pixel: csrc/warp.hip), and src and dst that overlap. */
#define DEI2I_WARP_REC_WORDS 8
int dei2i_warp(int N, int C, int H, int W, const float* tab_dev, int adjoint, const float* src, float* dst, dei2i_stream s);
/* Fill tab[b][n] (warp runs x N records, b counting the warp runs of the list in order, n in [0, N)) on the device from Philox4x32-10:
 * key = seed, counter words = (call low 32, call high 32, run | 4 << 16, row0 + n), run the run's index in the WHOLE run list of the
 * policy (blocks 0..2 of that word belong to dei2i_diffaug_draw, block 3 to dei2i_blit_draw): x0 -> r_s, x1 -> r_t, x2 -> r_l, each
 * (x >> 8) * 2^-24.  In fp32 without contraction, with the accurate exp2f, sinf, cosf (not the fast forms):
 *   s = exp2f(r_s - 0.5);  t = (2 r_t - 1) * (float)pi, c = cosf(t), sn = sinf(t);  l = exp2f(r_l - 0.5)
 *   m00 = l * (c * s);  m01 = l * (-(sn * s));  m10 = (sn * s) / l;  m11 = (c * s) / l;  tu = tv = 0, pad0 = pad1 = 0
 * -- M = diag(l, 1/l) . R(t) . s I, both singular values in [1/2, 2].  run_flags: 3 bits per run of the whole list, run r at bits
 * [3r, 3r + 3): the warp policies the run holds, 0 for a run of another kind (no row in the table); a policy that is absent
 * contributes its identity exactly (s = 1; c = 1, sn = 0; l = 1).  One launch of one workgroup, no atomics; it leaves *counter_dev
 * greater by exactly 1 under the ordering rule of dei2i_diffaug_draw, whose counter it shares: a diff_augment call launches
 * dei2i_diffaug_draw FIRST, dei2i_blit_draw SECOND and dei2i_warp_draw THIRD, only those it has runs for, and each sees the count
 * the one before it left.  A pure function of (seed, call, run, row0 + n): rows [row0, row0 + N) are that slice of the whole-batch
 * call.  BAD_ARG: null pointers, runs outside 1..DEI2I_DIFFAUG_MAX_RUNS, flag bits beyond the runs, no warp run, N <= 0, row0 < 0,
 * row0 + N > 2^31, runs * N >= 2^24. */
#define DEI2I_WARP_SCALE 1
#define DEI2I_WARP_ROTATE 2
#define DEI2I_WARP_ANISO 4
int dei2i_warp_draw(uint64_t seed, uint64_t* counter_dev, int runs, uint64_t run_flags, int N, int row0, float* tab, dei2i_stream s);
/* The same table with a gate per row and policy: block 5 (counter word run | 5 << 16) gives x0 for scale, x1 for rotate, x2 for
 * aniso, and a policy of the run applies to the row iff (x >> 8) * 2^-24 < *p_dev (one fp32 word of device memory); one that does
 * not apply contributes its identity exactly.  Block 4 is drawn as without gates: p = 1 gives the table of dei2i_warp_draw bit for
 * bit, p = 0 identity records only, and a row's parameters do not depend on its gates.  BAD_ARG: as dei2i_warp_draw, and a null
 * p_dev. */
int dei2i_warp_draw_p(uint64_t seed, uint64_t* counter_dev, int runs, uint64_t run_flags, int N, int row0, const float* p_dev,
                      float* tab, dei2i_stream s);

/* ---- the controller of p (csrc/ada.hip; Karras et al. 2020: r_t = E[sign(D(real))] held at a target) ----
 * dei2i_ada_measure: one workgroup over n fp32 logits; pair_dev[0] = sum of (x > 0) - (x < 0), pair_dev[1] = n, two int64 words,
 * written, or added to when accumulate != 0.  NaN and +-0 count 0 towards the sum and 1 towards n.  Integer sums: exact and
 * independent of order (wave shuffles, then LDS; thread 0 stores).  BAD_ARG: null pointers, n <= 0, n >= 2^31.
 *
 * dei2i_ada_apply: one thread.  p_rt_dev: two fp32 words (p, rt = the last computed r_t).  acc_dev: four int64 words (sum_sign,
 * n_logits, rows, calls).  Each call adds pair_dev[0], pair_dev[1], rows and 1 to them; when calls reaches interval:
 *   rt = (float)sum_sign / (float)n_logits;  step = (float)rows * inv_images;
 *   p = min(max(p + (rt > target ? step : rt < target ? -step : 0), 0), p_max);  acc_dev[0..3] = 0
 * in fp32 without contraction (inv_images = 1 / (images per unit of p), computed once by the host).  Launches that share the
 * words are ordered on one stream or in one captured graph; neither launch reads on the host or allocates.  BAD_ARG: null
 * pointers, interval <= 0, rows <= 0, p_max outside [0, 1], target outside (-1, 1), inv_images negative or NaN. */
int dei2i_ada_measure(const float* logits, int64_t n, int64_t* pair_dev, int accumulate, dei2i_stream s);
int dei2i_ada_apply(const int64_t* pair_dev, int64_t rows, float* p_rt_dev, int64_t* acc_dev, int interval, float target,
                    float inv_images, float p_max, dei2i_stream s);

/* ---- device-drawn shifted patch masks of the MAE stage (utils/masks.py) and the mask-token fill (csrc/mask.hip) ----
 * The patch grid of an H x W image is GH x GW = (H / patch + 1) x (W / patch + 1) (H, W multiples of patch); pixel (i, j) of row n
 * is kept when keep[n][(i + rs) / patch][(j + cs) / patch] != 0, (rs, cs) = shift[0], shift[1] in [0, patch).
 *
 * dei2i_mask_draw fills shift_dev[2] (int32) and keep_dev[N * GH * GW] (one byte per patch, 1 = kept) for global rows
 * [row0, row0 + N) from Philox4x32-10: key = seed, counter words = (call low 32, call high 32, c2, c3), call = *counter_dev as the
 * launch finds it.  Shifts: c2 = 0xC0000000, c3 = 0, rs = mulhi(x0, patch), cs = mulhi(x1, patch) -- the same for every row.
 * Keep bits: patch t = gi * GW + gj of row n takes word x[t % 4] of c2 = 0x80000000 | t / 4, c3 = row0 + n;
 * kept = (x >> 8) * 2^-24 < keep_prob (keep_prob = 1 - mask_ratio as fp32).  Bit 31 of c2 keeps these streams apart from
 * dei2i_diffaug_draw's (run | block << 16) under a shared seed.  One launch of one workgroup; it leaves *counter_dev greater by
 * exactly 1 (the ordering rule of dei2i_diffaug_draw holds).  BAD_ARG: null pointers, N, GH, GW, patch <= 0, row0 < 0,
 * row0 + N > 2^31, GH * GW >= 2^26, keep_prob outside [0, 1].
 *
 * dei2i_mask_fill: filled[n,c,i,j] = kept ? imgs[n,c,i,j] : token[n*ts[0] + c*ts[1] + i*ts[2] + j*ts[3]] on fp32 NCHW; the token is
 * addressed by element strides (0 on a broadcast dim), a null token fills with 0.  mask_out (nullable) receives the (N,1,H,W) fp32
 * mask.  The shifts are read from device memory; a patch index they carry off the grid is clamped to it.
 *
 * dei2i_mask_fill_bwd: grad_full[c,i,j] (C * H * W floats) = sum over n, in ascending order, of grad_out[n,c,i,j] at the masked
 * pixels: the token's gradient before its reduction over the token's broadcast dims.  Deterministic (no atomics). */
int dei2i_mask_draw(uint64_t seed, uint64_t* counter_dev, int N, int row0, int GH, int GW, int patch, float keep_prob,
                    int* shift_dev, unsigned char* keep_dev, dei2i_stream s);
int dei2i_mask_fill(int N, int C, int H, int W, int patch, const int* shift_dev, const unsigned char* keep_dev, const float* imgs,
                    const float* token, const int64_t* token_strides, float* filled, float* mask_out, dei2i_stream s);
int dei2i_mask_fill_bwd(int N, int C, int H, int W, int patch, const int* shift_dev, const unsigned char* keep_dev,
                        const float* grad_out, float* grad_full, dei2i_stream s);

/* ---- device-drawn style embeddings of the SEAN generator (csrc/embed.hip) ----
 * The embeddings file {label combination: list of embeddings} is packed into one fp32 bank (bank_rows x embed_nc), the lists in
 * ascending combination index, and an int32 table (1 << label_nc) x 2 of (offset, count) per combination.  The combination index
 * of a label row is sum_i b_i << (label_nc - 1 - i), b_i = (int)labels[n][i]: the first label is the slowest digit
 * (torch.cartesian_prod order).  A row with some b_i outside {0, 1} is invalid.
 *
 * dei2i_embed_draw fills index_out[N][num_embeds] (int32) for global rows [row0, row0 + N) from Philox4x32-10: key = seed, counter
 * words = (call low 32, call high 32, 0xA0000000 | e / 4, row0 + n), call = *counter_dev as the launch finds it; slot e takes word
 * x[e % 4]: index = offset + mulhi(x, count).  A combination with count == 0 (the reference feeds zeros for an empty list), an
 * invalid row and a table entry that does not lie inside [0, table_total) write -1.  labels: contiguous fp32 N x label_nc.
 * *invalid_dev (one 64-bit word) grows by the number of invalid rows of the call.  One launch of one workgroup, no global atomics;
 * it leaves *counter_dev greater by exactly 1 (the ordering rule of dei2i_diffaug_draw holds, for invalid_dev too).  The draw is a
 * pure function of (seed, call, e, row0 + n, the row's labels).  BAD_ARG: null pointers, N <= 0, row0 < 0, row0 + N > 2^31,
 * label_nc outside 1..DEI2I_EMBED_MAX_LABEL_NC, num_embeds <= 0 or > 2^28, table_total < 0.
 *
 * dei2i_embed_gather: out[r][:] = bank[index[r]][:] for r < rows (rows = N * num_embeds), zeros for an index outside
 * [0, bank_rows) -- no address is formed from such an index.  float4 copies when embed_nc % 4 == 0 and bank and out are 16-byte
 * aligned, scalar ones otherwise.  BAD_ARG: null pointers, a size <= 0, rows * embed_nc or bank_rows * embed_nc >= 2^40. */
int dei2i_embed_draw(uint64_t seed, uint64_t* counter_dev, int N, int row0, int label_nc, int num_embeds, const float* labels,
                     const int* table, int64_t table_total, int* index_out, uint64_t* invalid_dev, dei2i_stream s);
int dei2i_embed_gather(int64_t rows, int embed_nc, const int* index, const float* bank, int64_t bank_rows, float* out, dei2i_stream s);

/* ---- validation metrics (csrc/metrics.hip): the sums PSNR, L1 and SSIM are made of, and the classifier's confusion counts ----
 * dei2i_image_metrics: x, y contiguous fp32 NCHW, H, W >= 11; mask (nullable) fp32 (N,1,H,W), a pixel is masked when its word is
 * not 0.  out[n][0..5] (float64) = sum of (x-y)^2, sum of |x-y| over the image's C*H*W elements; the same two over the masked
 * pixels' elements and their count (all 0 without a mask); the sum of SSIM over the C*(H-10)*(W-10) window positions -- Wang et al.
 * 2004: 11 x 11 Gaussian window, sigma 1.5, weights normalised to 1, no padding, C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = data_range,
 * SSIM = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx^2 + sy^2 + C2)) from the window means of x, y, x^2, y^2, xy.  One
 * workgroup per 32 x 32 tile of window positions and plane stores six float64 partials to ws (dei2i_image_metrics_ws_doubles
 * words, no clearing); a second launch sums them per image in a fixed order: no atomics, bit-reproducible, nothing read on the
 * host.  BAD_ARG: null x, y, ws or out, N, C <= 0, H or W < 11, N*C*H*W >= 2^40, C*H*W >= 2^31, data_range <= 0.
 *
 * dei2i_clf_counts: logits and targets contiguous fp32 (N, K).  DEI2I_CLF_MULTI (bce / mse, multi-label): class k of a row is
 * predicted when logit > 0 (a logit of exactly 0 is a negative) and wanted when target > 0.5.  DEI2I_CLF_ARGMAX (cce): the row
 * predicts the first argmax of its logits and wants the first argmax of its targets.  counts: 4*K + 1 int64 words, TP[K] | FP[K] |
 * FN[K] | TN[K] | the number of rows right in every class; the launch ADDS to them (the caller zeroes them once, a whole loader
 * sums without a host read).  One workgroup, a class's words written by one thread: no atomics.  BAD_ARG: null pointers, N, K <= 0,
 * N*K >= 2^31, another kind. */
#define DEI2I_CLF_MULTI 0
#define DEI2I_CLF_ARGMAX 1
int64_t dei2i_image_metrics_ws_doubles(int N, int C, int H, int W);
int dei2i_image_metrics(int N, int C, int H, int W, const float* x, const float* y, const float* mask, double data_range, double* ws,
                        double* out, dei2i_stream s);
int dei2i_clf_counts(int N, int K, const float* logits, const float* targets, int kind, int64_t* counts, dei2i_stream s);

/* ---- spectral normalisation of a conv weight (--use_spectral; torch.nn.utils.spectral_norm semantics, one power
 * iteration per training-mode forward) ----  W = weight_orig as a (Cout, K) fp32 matrix, u (Cout) / v (K) the module's
 * buffers (updated in place when iterate != 0); u_used / v_used receive the vectors sigma was computed with (the backward
 * pass needs them: later forwards iterate the buffers again); scal: 4 floats (|W^T u|, |W v|, sigma, -); w_eff = W / sigma.
 * backward: dW (+)= (G - sum(G . w_eff) * u v^T) / sigma (accumulate != 0 adds into dW).  scratch:
 * dei2i_spectral_scratch_floats(Cout, K) floats forward, 1024 floats backward. */
size_t dei2i_spectral_scratch_floats(int Cout, int K);
int dei2i_spectral_fwd(int Cout, int K, const float* W, float* u, float* v, int iterate, float* scratch, float* u_used,
                       float* v_used, float* scal, float* w_eff, dei2i_stream s);
int dei2i_spectral_bwd(int Cout, int K, const float* G, const float* w_eff, const float* u_used, const float* v_used,
                       const float* scal, float* scratch, float* dW, int accumulate, dei2i_stream s);

/* Eval-mode BatchNorm folded into the weights of the conv in front of it (the ConvBlock of architecture.py:79-118 with running
 * statistics -- the generator passes of the D step, defectgan_model.py:251-262, and inference): w_eff[co] = a[co] * W[co],
 * b_eff[co] = bias[co] - running_mean[co] * a[co], a = weight * rsqrt(running_var + eps).  W / w_eff: Cout x K fp32 (OIHW). */
int dei2i_fold_bn_weight(int Cout, int K, const float* W, const float* bn_weight, const float* bn_bias, const float* running_mean,
                         const float* running_var, float eps, float* w_eff, float* b_eff, dei2i_stream s);

/* ---- SPADE's label path, second stage, for all modules of a generator at once (csrc/label_path.hip) ----
 * normalization.py:17-37 with a constant label map (the 5 x 5 class image of networks/architecture.py SPADE): gamma | beta =
 * conv3x3(actv; mlp_gamma | mlp_beta) + bias per module, every module reading `hidden` channels at its offset `in_off` of ONE activation
 * tensor actv (N, 5, 5, ctot) bf16 (the modules' mlp_shared convs run as one conv over their concatenated filters).  bf16 only.
 * One table entry per module (<= 16); C = norm_nc (multiple of 16), hidden in {32, 64, 96, 128}.
 *   pack : gamma_weight / beta_weight (C, hidden, 3, 3 fp32) -> packed_fwd, packed_dgrad (dei2i_label_gb_packed_elems(C, hidden) bf16 each)
 *   fwd  : gb (N, 5, 5, 2C) bf16 = [gamma | beta]
 *   dgrad: dactv (N, 5, 5, ctot) bf16, the module's channel slice written from gb = dL/d(gb) (zeros when live == 0)
 *   wgrad: d_gamma_weight / d_beta_weight (C, hidden, 3, 3 fp32), d_gamma_bias / d_beta_bias (C) written in full, from gb = dL/d(gb) */
typedef struct dei2i_label_mod {
  const float* gamma_weight;
  const float* beta_weight;
  const float* gamma_bias;
  const float* beta_bias;
  void* packed_fwd;
  void* packed_dgrad;
  void* gb;
  float* d_gamma_weight;
  float* d_beta_weight;
  float* d_gamma_bias;
  float* d_beta_bias;
  int C;
  int in_off;
  int live;
  int reserved;
} dei2i_label_mod;
size_t dei2i_label_gb_packed_elems(int C, int hidden);
int dei2i_label_gb_pack(const dei2i_label_mod* mods, int n, int hidden, dei2i_stream s);
int dei2i_label_gb_fwd(const dei2i_label_mod* mods, int n, int hidden, int ctot, int N, const void* actv, dei2i_stream s);
int dei2i_label_gb_dgrad(const dei2i_label_mod* mods, int n, int hidden, int ctot, int N, void* dactv, dei2i_stream s);
int dei2i_label_gb_wgrad(const dei2i_label_mod* mods, int n, int hidden, int ctot, int N, const void* actv, dei2i_stream s);

/* ---- in-library kernel timing (bench.py roofline leg): HIP events around every launch of one kernel family ---- */
#define DEI2I_PROF_GATHER_GEMM 0  /* the other conv forward / dgrad kernels: gather GEMM v1 / v2, thin convs */
#define DEI2I_PROF_WGRAD 1
#define DEI2I_PROF_HALO_CONV 2   /* the halo-resident 3x3 conv kernels, forward / zero-boundary launches (not part of family 0) */
#define DEI2I_PROF_HALO_FOLD 3   /* their FOLD launches (input gradients of the reflect-padded convs: run during backward passes,
                                    i.e. beside the weight-gradient kernels of ops' side stream) */
/* on = 1: HIP events around every launch of the family + FLOP count; on = 2: launch and FLOP count only (no events: the
 * stream sees nothing extra, total_ms reads 0); on = k >= 3: events around every k-th launch only (a sample -- two event
 * records per launch break the stream's back-to-back dispatch); on = 0: off */
int dei2i_prof_enable(int family, int on);
/* (call BEFORE dei2i_prof_collect) how many launches were bracketed with events since enable, and their FLOPs: total_ms of
 * dei2i_prof_collect belongs to these */
int dei2i_prof_collect_timed(int family, int64_t* timed_launches, double* timed_flops);
/* synchronises the recorded events; returns launches, total ms and total algorithmic FLOPs since enable */
int dei2i_prof_collect(int family, int64_t* launches, double* total_ms, double* total_flops);

/* ---- fused conv + norm + act (BASELINE.json configs[1]; SURVEY.md Appendix B groups G3..G16) -------------------------
 * The normalisation + activation that the reference applies BETWEEN two convs (architecture.py:116-118: conv -> BatchNorm
 * -> LeakyReLU; architecture.py:241-245,343-350 with normalization.py:24-37: SPADE's InstanceNorm * (1+gamma) + beta ->
 * ReLU -> conv) runs inside the halo-resident conv kernels:
 *   - `stats` (epilogue): per-channel sum / sum of squares of the conv's stored output, one record per 8x32-pixel tile,
 *     (N, dei2i_conv2d_stats_chunks, 2, CoutS) fp32 -- the dei2i_moments_partial layout, consumed by the finalize kernels;
 *   - `pro` (operand path): the conv's INPUT is z = act(A[n*n_stride + c] * x + B[...]), act(v) = max(v,0) + slope*min(v,0),
 *     applied to the input halo in LDS; z is never written to memory.  BatchNorm: A = a, B = b of dei2i_bn_finalize_train / _eval,
 *     n_stride = 0, slope = 0.2.  SPADE on a constant label map: A, B, ring from dei2i_spade_prep, n_stride = CinS,
 *     slope = 0; `ring` holds z of the logical input's 2-pixel frame (whose gamma / beta differ per pixel),
 *     [N][dei2i_ring_pixels(H<<up, W<<up)][CinS] in the compute dtype.
 * bf16, 3x3, stride 1, pad 1 only; no fallback inside: ask dei2i_conv2d_fused_supported / _wgrad_pro_supported first. */
typedef struct dei2i_pro {
  const float* A;
  const float* B;
  int n_stride;
  float slope;
  const void* ring;
} dei2i_pro;
int dei2i_conv2d_fused_supported(const dei2i_conv* c, int want_pro);          /* 1 / 0 */
int dei2i_conv2d_stats_chunks(const dei2i_conv* c);                           /* records per image written to `stats` */
int dei2i_conv2d_fwd_fused(const dei2i_conv* c, const void* x, const void* w_packed, const float* bias, int act, void* y,
                           const dei2i_pro* pro, float* stats, dei2i_stream s);   /* pro, stats: either may be NULL */
int dei2i_conv2d_wgrad_pro_supported(const dei2i_conv* c);
/* dei2i_conv2d_wgrad_oihw for a conv whose input was normalised on the operand path: x is the UN-normalised tensor */
int dei2i_conv2d_wgrad_oihw_pro(const dei2i_conv* c, const void* x, const void* dy, float* scratch, size_t scratch_elems,
                                float* dw_oihw, int accumulate, const dei2i_pro* pro, dei2i_stream s);
/* SPADE -> nearest x2 upsample -> conv (architecture.py:241-245) with z kept at the SOURCE resolution: gamma / beta of a constant
 * label map only differ on the 2-pixel frame of the upsampled image, so z[y][x] = z_src[y >> 1][x >> 1] everywhere else; the
 * conv (c->up = 1) reads z_src through its fused upsample and the frame's pixels from `ring` (dei2i_spade_prep) -- the
 * upsampled, normalised tensor (4x the bytes) is never written or read.  dei2i_conv2d_wgrad_oihw_pro with pro->A = pro->B =
 * NULL and pro->ring set is the matching weight gradient (x = z_src). */
int dei2i_conv2d_ring_supported(const dei2i_conv* c);
int dei2i_conv2d_fwd_ring(const dei2i_conv* c, const void* z_src, const void* ring, const void* w_packed, const float* bias, int act,
                          void* y, float* stats, dei2i_stream s);
/* Backward reductions of the normalisation layer in FRONT of a conv, taken from the epilogue of that conv's input-gradient
 * launch (the dz tile is still on chip) instead of by dei2i_spade_bwd_partial / dei2i_bn_bwd_partial re-reading dz and x:
 *   kind 1  z = relu(IN(x)*(1+gamma)+beta) with the (N,5,5,2C) class table `gb` (normalization.py:24-37); mean / rstd (N,C);
 *           partial (N, chunks, 4, C) -- the record layout of dei2i_spade_bwd_partial, for dei2i_spade_bwd_apply; the 24 border
 *           classes of the table's gradient still come from dei2i_spade_bwd_border
 *   kind 2  z = act(a*y + b), BatchNorm + activation (architecture.py:116-118), `x` = y; a / b / mean / rstd (C);
 *           partial (N*chunks, 2, C) -- the record layout of dei2i_bn_bwd_partial, for dei2i_bn_bwd_apply
 * chunks = dei2i_conv2d_dgrad_norm_chunks(c) records per image.  `x` has the conv input's channel stride (c->CinS) and, with
 * `up`, half the resolution of the conv's input (SPADE behind a nearest x2 upsample; c describes the conv at the upsampled
 * size with c->up = 0).  bf16, stride-1 reflect-padded 3x3 convs on grids the 16 x 32 tile kernel takes: ask _supported first --
 * dei2i_conv2d_dgrad_input_norm has no fallback inside. */
typedef struct dei2i_epi_norm {
  int kind;
  int up;
  int act;
  int group_images;   /* kind 2: a / b / mean / rstd hold one row of C per group of this many images (BatchNorm statistics taken
                         per group of a batch that carries several passes); 0: one row for the whole batch */
  const void* x;
  const float* mean;
  const float* rstd;
  const void* gb;
  const float* a;
  const float* b;
  float* partial;
} dei2i_epi_norm;
int dei2i_conv2d_dgrad_norm_supported(const dei2i_conv* c);                   /* 1 / 0 */
int dei2i_conv2d_dgrad_norm_chunks(const dei2i_conv* c);
int dei2i_conv2d_dgrad_input_norm(const dei2i_conv* c, const void* dy, const void* wd_packed, void* dx, const dei2i_epi_norm* en,
                                  dei2i_stream s);
/* nn.AvgPool2d(2, 2) on NHWC (N, H, W, C), H and W even (architecture.py:157-168); out / dout: (N, H/2, W/2, C) */
int dei2i_avgpool2_fwd(int dtype, int N, int H, int W, int C, const void* x, void* out, dei2i_stream s);
int dei2i_avgpool2_bwd(int dtype, int N, int H, int W, int C, const void* dout, void* dx, dei2i_stream s);
/* the border-class half of dei2i_spade_bwd_partial alone (class mode): dgb_cls[n, cy, cx, :] for the 24 classes (cy, cx) != (2, 2) */
int dei2i_spade_bwd_border(int dtype, int N, int H, int W, int C, int up, const void* dz, const void* x, const float* mean,
                           const float* rstd, const void* gb, float slope, void* dgb_cls, dei2i_stream s);
/* out[n, p, c] = max(A[n, c] * x[n, p, c] + B[n, c], 0) + slope * min(..., 0): an affine + activation with per-IMAGE
 * coefficients (SPADE's interior class at the source resolution; HW pixels per image) */
int dei2i_affine_act_img_fwd(int dtype, int N, int HW, int C, const void* x, const float* A, const float* B, float slope, void* out,
                             dei2i_stream s);
size_t dei2i_ring_pixels(int H, int W);                                        /* 4*W + 4*(H-4) */
/* InstanceNorm finalize + SPADE coefficient preparation in one launch: mean / rstd (N,C) from the partial records (`chunks`
 * per image, HW = Hs*Ws pixels each image), A = rstd*(1+gamma_int), B = beta_int - mean*A for the interior class of the
 * (N,5,5,2C) table, and (ring != NULL) relu(IN(x)*(1+gamma)+beta) of the 2-pixel frame of the (Hs<<up, Ws<<up) image */
int dei2i_spade_prep(int dtype, int N, int Hs, int Ws, int C, int up, const void* x, const float* partial, int chunks, float eps,
                     const void* gb_table, float* mean, float* rstd, float* A, float* B, void* ring, dei2i_stream s);

/* ---- which kernel served a call: host-side launch counters per MFMA kernel family (tests assert the family, so a
 * fall-through from a tuned kernel to the generic GEMM cannot pass unnoticed).  dei2i_launch_counts copies up to n
 * counters and returns how many families exist; dei2i_kernel_name(i) names family i ("halo_conv", "gather_v2",
 * "gather_v1", "thin_cin", "thin_cout", "wgrad_halo", "wgrad_v2", "wgrad_v1", "wgrad_thin", "halo_conv_fp8",
 * "halo16_conv"). */
int dei2i_launch_counts(int64_t* out, int n);
void dei2i_launch_counts_reset(void);
const char* dei2i_kernel_name(int kid);

#ifdef __cplusplus
}
#endif
#endif /* DEI2I_HIP_H */
