/* vvae_hip.h -- C ABI of libvvae_hip.so: the MI355X (gfx950) kernels of the video-VAE hot path.
 *
 * The reference (floatingtrees/video-VAE) has no native code and no FFI: every op below replaces an
 * XLA-lowered Flax/JAX call.  Each entry point cites the reference call site it stands in for
 * (paths relative to the reference checkout).  INTEGRATION.md shows the Python-side binding.
 *
 * Conventions
 *   - plain pointers + sizes only; every buffer is BORROWED device memory owned by the caller;
 *   - activations are channels-last (n,t,h,w,c) seen as rows of `C` channels with row pitch `ld*`
 *     (in elements, >= C), so a channel slice of a wider buffer is a valid operand;
 *   - `dtype`: VVAE_DT_F32 (0) or VVAE_DT_BF16 (1) is the STORAGE type of activations; parameters and
 *     parameter gradients are always fp32 in Flax layout (Conv kernel (kt,kh,kw,Cin,Cout));
 *   - `stream` is a hipStream_t; everything is enqueued asynchronously on it, nothing synchronises;
 *   - return value: 0 on success, a hipError_t value, or VVAE_ERR_* (>= 1000);
 *   - process-global mutable state is limited to test / tuning hooks, none of which the product path calls:
 *     vvae_conv3d_force_generic, vvae_conv3d_deep_config, vvae_conv3d_roll_config, vvae_conv3d_wgrad_config, vvae_gemm_tn_use_big_tiles,
 *     vvae_gemm_nt_persistent, vvae_gemm_nt_prefetch, vvae_gemm_pp_final_ring, vvae_gemm_pp_ablate, vvae_temporal_attn_mfma_enable,
 *     vvae_temporal_attn_mfma_config, vvae_temporal_attn_mfma32_enable (each documented at its declaration; tests/test_host.py holds the
 *     list), plus one cache: vvae_linear_residual_bf16 / vvae_linear_residual_wt_bf16 keep the
 *     hipBLASLt handle and the solution the library's heuristic chose per (shape, pitches) behind a mutex; everything else is a pure function of its arguments.
 */
#ifndef VVAE_HIP_H
#define VVAE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VVAE_DT_F32 0
#define VVAE_DT_BF16 1
#define VVAE_ERR_BAD_ARG 1001
#define VVAE_ERR_WORKSPACE 1002
#define VVAE_ERR_LIBRARY 1003

/* ---- Conv3d, SAME padding, stride 1, odd kernel: nnx.Conv at train/unet.py:13-21 (3x3x3 ConvBlock3D),
 *      :111-113 (3x7x7 patch_mixer), :144-153 (1x1x1 final_conv) and their autodiff (dgrad, wgrad). ---- */
size_t vvae_conv3d_workspace_bytes(int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw, int dtype,
                                   int which /* 0 fwd, 1 dgrad, 2 wgrad */);
int vvae_conv3d_fwd(const void* x, int ldx, const float* w, const float* bias, void* y, int ldy,
                    int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw, int dtype,
                    void* ws, size_t ws_bytes, void* stream);
int vvae_conv3d_dgrad(const void* dy, int lddy, const float* w, void* dx, int lddx,
                      int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw, int dtype,
                      void* ws, size_t ws_bytes, void* stream);
int vvae_conv3d_wgrad(const void* x, int ldx, const void* dy, int lddy, float* dw, float* dbias,
                      int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw, int dtype,
                      void* ws, size_t ws_bytes, void* stream);
void vvae_conv3d_force_generic(int on);   /* test hook: 1 = bypass the bf16 fast path */
/* the any-shape fp32-matrix-core path, exported so tests can cross-check the fast path against it */
int vvae_conv3d_fwd_generic(const void* x, int ldx, const float* w, const float* bias, void* y, int ldy,
                            int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw, int dtype, void* stream);
int vvae_conv3d_dgrad_generic(const void* dy, int lddy, const float* w, void* dx, int lddx,
                              int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw, int dtype, void* stream);
/* no atomics: one fp32 partial dW per voxel chunk in ws (vvae_conv3d_wgrad_generic_ws_bytes), folded in index order */
size_t vvae_conv3d_wgrad_generic_ws_bytes(int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw);
int vvae_conv3d_wgrad_generic(const void* x, int ldx, const void* dy, int lddy, float* dw, float* dbias,
                              int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw, int dtype,
                              void* ws, size_t ws_bytes, void* stream);
int vvae_conv3d_deep_config(int on);               /* test/tuning hook: deep (K-split waves) rolling fwd/dgrad kernel on/off (off: per-frame kernel) */
int vvae_conv3d_roll_config(int on, int tchunk);   /* test/tuning hook: rolling time-column fwd/dgrad kernel on/off, frames per workgroup */
int vvae_conv3d_wgrad_config(int cob16, int blocks); /* tuning hook: 16 output channels per wgrad workgroup (default 0), persistent grid size (0 = per-config default) */
int vvae_conv3d_bf16_supported(int Cin, int Cout, int kt, int kh, int kw, int ld_in, int ld_out, int which, int flags);
size_t vvae_conv3d_bf16_ws_bytes(int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw, int which);
/* flags (pack and forward calls of one layer must agree): bit 0 = input-gradient form; bits 8-15 = how many of the layer's K channels
   (Cin forward, Cout for the input gradient) are real when tensor and weights are zero-padded to 16 (0 = all).  The 3x7x7 patch mixer
   with 12 real channels (train/unet.py:111-113) then multiplies K = 3*7*12 = 252 instead of 336; other values are accepted and ignored. */
int vvae_conv3d_pack_bf16(const float* w, void* ws, size_t ws_bytes, int Cin, int Cout, int kt, int kh, int kw,
                          int flags, void* stream);
/* n <= 64 packings in one launch (every conv layer of the UNet, forward + input-gradient forms: the weights change once per
   optimizer step); host arrays of device pointers / ints, kt = 3, kw = kh in {3, 7}. */
int vvae_conv3d_pack_grouped_bf16(const float* const* w, void* const* ws, const size_t* ws_bytes, const int* Cin, const int* Cout,
                                  const int* kh, const int* flags, int n, void* stream);
int vvae_conv3d_fwd_bf16(const void* x, int ldx, const float* w, const float* bias, void* y, int ldy,
                         int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw, int flags,
                         int prepacked, void* ws, size_t ws_bytes, void* stream);
/* vvae_conv3d_fwd_bf16, _gn and _cat2 are three forms of one launch path (conv_fwd_like in conv3d_bf16.hip): it validates pointers
   (x, x2 16-byte, y, y2 8-byte aligned), pitches (input side % 8, produced side % 4, each at least the channels its tensor holds), the
   partial buffer's eligibility and then the workspace, and tries the rolling, the deep and the per-frame kernel in that order; the
   per-frame kernel takes neither a second tensor nor gn_part nor a real-channel count. */
/* Forward Conv3d that also emits the GroupNorm statistics of its (rounded) output -- ConvBlock3D's conv + norm statistics in one
   pass (reference train/unet.py:13-23).  vvae_conv3d_gn_blocks: rows per sample of the partial buffer (0 = layer not eligible,
   use vvae_gn_stats); gn_part: N * blocks * groups * 2 floats, consumed by vvae_gn_finalize. */
int vvae_conv3d_gn_blocks(int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw, int ld_in, int ld_out, int groups);
int vvae_conv3d_fwd_bf16_gn(const void* x, int ldx, const float* w, const float* bias, void* y, int ldy,
                            int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw,
                            int prepacked, void* ws, size_t ws_bytes, float* gn_part, int groups, void* stream);
size_t vvae_conv3d_wgrad_bf16_ws_bytes(int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw);
int vvae_conv3d_wgrad_bf16(const void* x, int ldx, const void* dy, int lddy, float* dw, float* dbias,
                           int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw,
                           void* ws, size_t ws_bytes, void* stream);
/* The decoder's concat([up, skip], channels) + conv1 (reference train/unet.py:79-81) at 16 + 16 channels WITHOUT the joint tensor: the
   conv reads its input channels from two dense tensors (x: the first c_split, x2: the rest), its input gradient writes two dense
   tensors (y, y2) and its weight gradient stages X from both.  (A producer that fills a 32-byte channel half of 64-byte voxels
   runs at a third of the HBM rate; see tools/convt_pitch_probe.py.)  which: 0 forward (y2 = NULL; gn_part optional, as in
   vvae_conv3d_fwd_bf16_gn), 1 input gradient (x = dY, x2 = NULL).  ws: packed weights (vvae_conv3d_pack_bf16 / _grouped). */
int vvae_conv3d_cat2_supported(int Cin, int Cout, int c_split, int kt, int kh, int kw);
int vvae_conv3d_fwd_bf16_cat2(const void* x, int ldx, const void* x2, int ldx2, const float* bias, void* y, int ldy, void* y2, int ldy2,
                              int c_split, int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw, int which,
                              const void* ws, size_t ws_bytes, float* gn_part, int groups, void* stream);
int vvae_conv3d_wgrad_bf16_cat2(const void* x, int ldx, const void* x2, int ldx2, int c_split, const void* dy, int lddy, float* dw,
                                float* dbias, int N, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw, void* ws,
                                size_t ws_bytes, void* stream);
/* out[c] = sum over V rows of x[v][c] (bias gradients) */
int vvae_colsum_blocks(long V);   /* rows of vvae_colsum's partial buffer */
/* out[c] = sum over V rows of x[v][c]; part: fp32 scratch, vvae_colsum_blocks(V) x C floats; two stages, no atomics: bitwise reproducible */
int vvae_colsum(const void* x, int ld, long V, int C, float* out, float* part, int dtype, void* stream);

/* ---- the rl flavour's latent gate (train/rl_model.py:136-145): pair doubling + Bernoulli frame masks + fill (1 - mask) + z mask, one launch each way.
 *      z fp32 (B2/2, T, per), prob fp32 (B2/2, T), u fp32 (B2, T), fill fp32 (LD) -> comp bf16 (B2, T, per), mask fp32 (B2, T);
 *      bwd: dcomp bf16 -> dz fp32 (B2/2, T, per) and vvae_rl_gate_blocks(...) partial rows of d fill (LD floats each).  per = hw * LD. ---- */
int vvae_rl_gate_ok(int B2, int T, long per, int LD);
int vvae_rl_gate_blocks(int B2, int T, long per);
int vvae_rl_gate_fwd(const float* z, const float* prob, const float* u, const float* fill, void* comp, float* mask, int B2, int T, long per,
                     int LD, void* stream);
int vvae_rl_gate_bwd(const void* dcomp, const float* mask, float* dz, float* part, int B2, int T, long per, int LD, void* stream);

/* ---- zero-pad (unpad = 0) / cut back (unpad = 1) the last two dims of n <= 8 small contiguous fp32 tensors in one launch: the UNet's
 *      12-channel weights on the 16-channel matrix-core kernels (train/unet.py:98-104).  pad: src (rows, s0, s1) -> dst (rows, d0, d1);
 *      unpad: src (rows, d0, d1) -> dst (rows, s0, s1).  Host arrays of device pointers / ints. ---- */
int vvae_pad_last2_grouped(const float* const* src, float* const* dst, const long* rows, const int* s0, const int* s1, const int* d0,
                           const int* d1, int n, int unpad, void* stream);

/* ---- 1x1x1 convolutions onto 3 channels as HBM streams (UNet.final_conv train/unet.py:144-153,188; the PatchUnEmbedding
 *      down-projection train/layers.py:60-79).  Reached through vvae_conv3d_{fwd,dgrad,wgrad}; V = voxels, Cin in {12, 16}. ---- */
int vvae_conv_pointwise_supported(int Cin, int Cout, int kt, int kh, int kw, int ldx, int dtype, const void* x);
size_t vvae_conv_pointwise_ws_bytes(long V, int Cin, int Cout);
int vvae_conv_pointwise_fwd(const void* x, int ldx, const float* w, const float* bias, void* y, int ldy, long V, int Cin, int Cout,
                            int dtype, void* stream);
/* y = addend + conv(x) + bias (addend: V rows of Cout channels, pitch ldadd, or NULL): the decoder's coarse + UNet(features), train/model.py:97 */
int vvae_conv_pointwise_fwd_add(const void* x, int ldx, const float* w, const float* bias, const void* addend, int ldadd, void* y, int ldy,
                                long V, int Cin, int Cout, int dtype, void* stream);
int vvae_conv_pointwise_dgrad(const void* dy, int lddy, const float* w, void* dx, int lddx, long V, int Cin, int Cout, int dtype,
                              void* stream);
/* dx = addend + dy W^T (addend: V rows of Cin channels, pitch ldadd, or NULL): the gradient of the tensor's other consumer joins inside the launch */
int vvae_conv_pointwise_dgrad_add(const void* dy, int lddy, const float* w, const void* addend, int ldadd, void* dx, int lddx, long V, int Cin,
                                  int Cout, int dtype, void* stream);
int vvae_conv_pointwise_wgrad(const void* x, int ldx, const void* dy, int lddy, float* dw, float* dbias, long V, int Cin, int Cout,
                              int dtype, void* ws, size_t ws_bytes, void* stream);

/* ---- dst_i (cols_i, rows_i) = src_i (rows_i, cols_i)^T for n <= 64 contiguous bf16 matrices (dims multiples of 64) in one launch: the
 *      (out, in) shadows of the Linear kernels that vvae_gemm_nt_bf16 multiplies in the forward pass, refreshed once per optimizer step. ---- */
int vvae_transpose_grouped_bf16(const void* const* src, void* const* dst, const int* rows, const int* cols, int n, void* stream);

/* The scalar end of the recon + KL loss, value and gradients in one launch (reference train/legacy/training_loop_adversarial.py:100-124:
 * selection density against 1 / max_compression_rate with magnified negatives, MSE + gamma1 selection + gamma2 KL).
 * mse_ps fp32 (B, mse_cols), kl_ps fp32 (B, kl_cols): the per-sample MSE / KL terms as >= 1 partial sums each (summed here in index order: the
 * per-workgroup partials of vvae_masked_mse_mae_fwd, the per-frame partials of vvae_encoder_head_fwd, or one column); selection, mask fp32 (B, T)
 * contiguous.  out fp32 [5] = loss, MSE, selection_loss, kl_loss, mean kept-frame density.  grads fp32 [2 B + B T] = d loss / d (per-sample MSE) |
 * d loss / d (per-sample KL) | d loss / d selection.  B <= 1024. */
int vvae_loss_tail_plain(const float* mse_ps, int mse_cols, const float* kl_ps, int kl_cols, const float* selection, const float* mask, int B, int T,
                         float max_compression_rate, float magnify_negatives_rate, float gamma1, float gamma2, float* out,
                         float* grads, void* stream);

/* The same for the pair / REINFORCE loss of the rl flavour (train/rl_nonadversarial.py:130-186; samples 2k, 2k + 1 are a pair): mse, mae fp32
 * (B2, cols) partial sums, perc fp32 [B2] or NULL, kl fp32 [B2], sel (probabilities) / act (sampled actions) / mask fp32 (B2, T).  out fp32 [9] = loss,
 * MSE, perceptual, selection_loss, kl_loss, mean density, mean trajectory probability, rl_loss, MAE.  grads fp32 [4 B2 + B2 T] = d loss / d mse |
 * mae | perc | kl (per sample) | sel.  kl: (B2, kl_cols) partial sums of the per-sample term (kl_cols = 1: the term itself).  B2 even, <= 1024. */
int vvae_loss_tail_rl(const float* mse, const float* mae, int cols, const float* perc, const float* kl, int kl_cols, const float* sel, const float* act,
                      const float* mask, int B2, int T, float max_compression_rate, float magnify_negatives_rate, float gamma1,
                      float gamma2, float gamma3, float gamma4, float rl_loss_weight, float* out, float* grads, void* stream);

/* ---- The encoder's heads and the latent gate in train mode, one launch each way; rl 0 = the model.py flavour (reference train/model.py:53-59,
 *      121-133; train/layers.py:226-252), rl 1 = the rl flavour (train/rl_model.py:50-60,119-147); vvae_encoder_head_eval_fwd below takes the same flag.
 *      log_var = log(softplus(v)), selection logits = Linear(hw -> 1)(Linear(ld -> 1)(mean)) + 1, z = mean + eps exp(log_var / 2), and the
 *      per-frame share of the KL term.  One workgroup per frame; bf16 tensors, fp32 parameters.
 *      model: sel = round(sigmoid(logits + log(u / (1 - u)))) with the straight-through gradient, comp = fill (1 - sel) + z sel.
 *      rl: the selection is the probability sigmoid(logits) rounded to bf16; every clip is doubled into a pair (samples 2k, 2k + 1 of the outputs)
 *      whose members draw their own Bernoulli frame mask u < probability and gate the shared latent with it.  B2 = B (model) or 2B (rl).
 *      mean, v bf16 (B, T, HW, LD) contiguous; w1 (LD), b1 (1), w2 (HW), b2 (1), fill (LD) fp32; u fp32 (B2 T); eps fp32 (B, T, HW, LD);
 *      mask fp32 rows of T, mask_pitch elements apart per sample (rl: per clip).  fwd -> logvar, comp bf16 (B2, T, HW, LD); sel fp32 (B2 T) (rl: the
 *      pair-doubled probability); y (model: the noisy logit, rl: the logits) fp32 (B T); s1 fp32 (B T, HW); kl_frame fp32 (B2, T); rl only, NULL
 *      otherwise: mean2 bf16 (2B, T, HW, LD), mask2 fp32 (2B T).  bwd: logvar, y, s1 from the forward, sel its selection (rl: its mask2);
 *      dcomp bf16 (B2, T, HW, LD) / dsel fp32 (B2 T) (rl: the gradient at the pair-doubled probability) / gkl fp32 at
 *      [i gkl_pitch_b + t gkl_pitch_t] for i < B2 / dlv_ext bf16 (B, T, HW, LD), each may be NULL
 *      -> dmean, dv bf16 (B, T, HW, LD); one partial row per frame of part1 (B T, LD) = dW1, part2 (B T, HW) = dW2, part3 (B T, LD) = d fill and
 *      partb (2, B T, 4) = [db1 0 0 0] rows, then [db2 0 0 0] rows.  HW % 4 == 0, LD % 8 == 0; mask_pitch 0 = one mask row for all samples. ---- */
int vvae_encoder_head_ok(int B, int T, int HW, int LD);
int vvae_encoder_head_fwd(const void* mean, const void* v, const float* w1, const float* b1, const float* w2, const float* b2,
                          const float* u, const float* eps, const float* mask, long mask_pitch, const float* fill, int rl, void* logvar,
                          void* mean2, void* comp, float* sel, float* mask2, float* y, float* s1, float* kl_frame, int B, int T, int HW,
                          int LD, void* stream);
int vvae_encoder_head_bwd(const void* mean, const void* v, const void* logvar, const float* eps, const float* mask, long mask_pitch, const float* fill,
                          const float* w1, const float* w2, const float* y, const float* s1, const float* sel, const void* dcomp,
                          const float* dsel, const float* gkl, long gkl_pitch_b, long gkl_pitch_t, const void* dlv_ext, int rl, void* dmean,
                          void* dv, float* part1, float* part2, float* part3, float* partb, int B, int T, int HW, int LD, void* stream);

/* The eval heads (reference train/model.py:121-131 with train=False; train/rl_model.py:50-60 without the pair doubling), forward only, one
 *      workgroup per frame; the shapes vvae_encoder_head_ok takes.  mean, v bf16 (B, T, HW, LD) contiguous (v may be NULL when logvar is);
 *      w1 (LD), b1 (1), w2 (HW), b2 (1), fill (LD) fp32; u fp32 (B T) uniforms or NULL; rl 0 = model flavour: sel = rint(sigmoid(logits)), u ignored;
 *      rl 1: prob = sigmoid(logits) rounded to bf16, sel = u < prob (u given) else rint(prob).  mask fp32 rows of T, mask_pitch elements apart per
 *      sample (0: one row for all), or NULL: sel = 0 on every frame it marks 0 (padding is gated to the fill token).  -> logvar = log(softplus(v)) bf16 when non-NULL;
 *      comp = fill (1 - sel) + mean sel bf16; sel fp32 (B T) in {0, 1}; prob fp32 (B T) (rl only, required there). */
int vvae_encoder_head_eval_fwd(const void* mean, const void* v, const float* w1, const float* b1, const float* w2, const float* b2,
                               const float* u, const float* mask, long mask_pitch, const float* fill, int rl, void* logvar, void* comp,
                               float* sel, float* prob, int B, int T, int HW, int LD, void* stream);

/* Reconstruction metrics per frame (no reference counterpart: the standard PSNR / SSIM of a clip against its reconstruction).  x, y (B, T, H, W, C)
 *      contiguous, each VVAE_DT_F32 or VVAE_DT_BF16 (x_dtype, y_dtype independent), element-aligned; both converted to fp32 and, with clamp != 0,
 *      clamped to [0, 1].  mask fp32 (B T), nonzero = valid frame; a masked frame is never read.  -> mse, psnr, ssim fp32 (B T):
 *      mse = mean over H W C of (x - y)^2, psnr = 10 log10(1 / max(mse, 1e-10)), ssim = Wang et al. 2004 with an 11-tap Gaussian window
 *      (sigma 1.5, separable, normalised), valid positions only (rows / columns 5 .. n - 6), C1 = 0.01^2, C2 = 0.03^2, averaged over the
 *      positions and channels; all three 0 on masked frames.  part: scratch of vvae_recon_metrics_part_floats(B, T, H, W, C) floats, written
 *      before it is read.  Two launches (the per-band pass and the fold over the bands); deterministic, bitwise reproducible.
 *      supported: H, W >= 11, 1 <= C <= 4, W C <= 2048.  part_floats returns 0 for a shape the kernel does not take. */
int vvae_recon_metrics_supported(int H, int W, int C, int x_dtype, int y_dtype);
size_t vvae_recon_metrics_part_floats(int B, int T, int H, int W, int C);
int vvae_recon_metrics_fwd(const void* x, int x_dtype, const void* y, int y_dtype, const float* mask, float* mse, float* psnr, float* ssim,
                           float* part, int B, int T, int H, int W, int C, int clamp, void* stream);
/* vvae_recon_metrics_fwd for frames of any width 11 <= W <= 8192 (1 <= C <= 4, H >= 11, B T <= 65535), same definition and arguments.  A shape
 * vvae_recon_metrics_fwd takes runs that entry (bitwise its results); wider rows run column strips (a third grid dimension): each strip reads
 * at most 2048 values of a row, a 5-column halo on each side included; the strips' SSIM columns partition 5 .. W - 6 and their squared-error
 * columns 0 .. W - 1; one partial pair per (frame, strip, band), folded in that order.  part: vvae_recon_metrics_wide_part_floats floats. */
int vvae_recon_metrics_wide_supported(int H, int W, int C, int x_dtype, int y_dtype);
size_t vvae_recon_metrics_wide_part_floats(int B, int T, int H, int W, int C);
int vvae_recon_metrics_wide_fwd(const void* x, int x_dtype, const void* y, int y_dtype, const float* mask, float* mse, float* psnr,
                                float* ssim, float* part, int B, int T, int H, int W, int C, int clamp, void* stream);
/* Multi-scale SSIM per frame (Wang, Simoncelli, Bovik 2003; metrics.ms_ssim states the definition).  x, y, mask, clamp as above.  `scales` = M
 *      levels, 1 .. 5; level j + 1 is the 2 x 2 mean of level j, ((v00 + v01) + (v10 + v11)) 0.25 in fp32, an odd trailing row or column
 *      dropped (H' = H / 2, W' = W / 2).  Per level and channel c, with the window, moments and constants of vvae_recon_metrics_fwd:
 *      CS = (2 sxy + C2) / (sx + sy + C2), S = (2 mx my + C1) / (mx^2 + my^2 + C1) CS, cs_j[c] and ssim_j[c] their means over the valid
 *      positions.  -> ms_ssim fp32 (B T) = mean over c of prod_{j < M - 1} max(cs_j[c], 0)^w_j max(ssim_{M-1}[c], 0)^w_{M-1}, the powers
 *      and the product in double, the weights w0 .. w4 (non-negative; those past `scales` ignored) used as given; terms fp32 (B T, M, C)
 *      or NULL: the unclamped cs_j[c] for j < M - 1 and ssim_{M-1}[c].  Both 0 on masked frames, which are never read.
 *      ws: scratch of vvae_ms_ssim_ws_floats(B, T, H, W, C, scales) floats (the fp32 pyramid of both operands, then the partial sums of
 *      every level), 16-B aligned for the wide accesses; every word is written before it is read.  2 M launches: M moment passes (one
 *      (S, CS) pair per frame, strip, band and channel, summed in a fixed order), M - 1 pools, one fold; no atomics, no memset, no
 *      allocation; bitwise reproducible.  supported: 1 <= C <= 4, 1 <= M <= 5, min(H, W) >> (M - 1) >= 11, W <= 8192; the entries with
 *      B, T also need B T <= 65535.  ws_floats returns 0 for a shape the kernels do not take. */
int vvae_ms_ssim_supported(int H, int W, int C, int scales, int x_dtype, int y_dtype);
size_t vvae_ms_ssim_ws_floats(int B, int T, int H, int W, int C, int scales);
int vvae_ms_ssim_fwd(const void* x, int x_dtype, const void* y, int y_dtype, const float* mask, float* ms_ssim, float* terms, float* ws,
                     int B, int T, int H, int W, int C, int scales, double w0, double w1, double w2, double w3, double w4, int clamp,
                     void* stream);
/* SSIM as a training loss: the per-frame SSIM of vvae_recon_metrics_fwd and its gradient with respect to y (metrics.ssim_grad_reference states
 *      the definition).  x (B / video_div, T, H, W, C) the clip, y (B, T, H, W, C) its reconstruction, contiguous, each VVAE_DT_F32 or
 *      VVAE_DT_BF16; sample i of y is compared with sample i / video_div of x (video_div >= 1 divides B).  mask fp32 (B T) per frame of y,
 *      nonzero = valid; a masked frame is never read.  ws: vvae_ssim_loss_ws_floats(B, T, H, W, C) floats, 16-B aligned: per frame, map and
 *      channel (H - 10) rows of W rounded up to 4 floats (12 bytes per valid position and channel, plus that rounding), then the forward's
 *      partial sums; every word that is read was written by the forward.
 *   fwd -> ssim fp32 (B T), bit for bit vvae_recon_metrics_fwd's for the same operands (the same kernel body, plan and fold), 0 on masked
 *      frames; it also stores, at every valid position p and channel, with a1 = 2 mx my + C1, a2 = 2 sxy + C2, b1 = mx^2 + my^2 + C1,
 *      b2 = sx + sy + C2, S = a1 a2 / (b1 b2):  A = dS/dmy = 2 mx (a2 - a1) / (b1 b2) + 2 my S (1 / b2 - 1 / b1),  Bm = dS/d(g * y^2) = -S / b2,
 *      Cm = dS/d(g * x y) = 2 a1 / (b1 b2).  Two launches.
 *   bwd: gout fp32 (B T), the upstream gradient per frame -> dy, y's shape and dtype (fp32, or bf16 rounded once):
 *      dy(q) = gout[f] / (C (H - 10)(W - 10)) [ (G^T A)(q) + 2 y(q) (G^T Bm)(q) + x(q) (G^T Cm)(q) ], G^T the 11 x 11 window applied to the map
 *      zero-extended by 5 on every side; with clamp != 0, x and y are clamped to [0, 1] and dy is 0 where y lies strictly outside [0, 1].
 *      Every element of dy is written exactly once, zeros on masked frames and where gout[f] == 0 (those frames' maps are not read).  One
 *      launch in gather form: no atomics, no memset, no allocation, a fixed summation order; bitwise reproducible, safe in a captured graph.
 *      dy may overlap none of x, y, mask, gout, ws (VVAE_ERR_BAD_ARG).
 *   supported: the one-strip shapes, H, W >= 11, 1 <= C <= 4, W C <= 2048; the entries with B, T also need B T <= 65535.  ws_floats and
 *      band_rows (the rows per workgroup of both passes, what a test needs to choose a height of several bands) return 0 otherwise.
 *      A refused call (VVAE_ERR_BAD_ARG) launches nothing. */
int vvae_ssim_loss_supported(int H, int W, int C, int x_dtype, int y_dtype);
size_t vvae_ssim_loss_ws_floats(int B, int T, int H, int W, int C);
int vvae_ssim_loss_band_rows(int B, int T, int H, int W, int C);
int vvae_ssim_loss_fwd(const void* x, int x_dtype, const void* y, int y_dtype, const float* mask, float* ssim, float* ws, int B, int T, int H,
                       int W, int C, int video_div, int clamp, void* stream);
int vvae_ssim_loss_bwd(const void* x, int x_dtype, const void* y, int y_dtype, const float* mask, const float* gout, const float* ws, void* dy,
                       int B, int T, int H, int W, int C, int video_div, int clamp, void* stream);

/* Spatial tiling (video_vae_amd/tiling.py): frames (N, T, H, W, C) cut into overlapping S x S tiles and blended back.  Grid per axis of length L:
 * n = 1 if L <= S, else ceil((L - o) / (S - o)), 0 <= o <= S / 2; start_i = i (L - S) / (n - 1) (integer division), 0 for n == 1.  Tiles are
 * numbered flat = window ny nx + ty nx + tx.  ny, nx must be what (H, W, S, overlap) give.
 *   gather: src uint8 (N, T, H, W, C) contiguous; lut fp32 [256], the value of each byte (the caller's u8 -> fp32 conversion, e.g. / 255);
 *     dst fp32 (count, T, S, S, C), 16-B aligned: tiles first .. first + count - 1.  Source indices past the frame clamp to its last row /
 *     column (edge replication).  supported: 1 <= C <= 4, S C % 4 == 0.
 *   both: H, W <= 16384.
 *   blend: tiles (N ny nx, T, S, S, C) contiguous, dtype VVAE_DT_F32 / VVAE_DT_BF16 -> out fp32 (N, T, H, W, C) contiguous.  Per axis the
 *     weight of tile i at in-tile position p is min(1, (p + 0.5) / r) with r = end_{i-1} - start_i, times min(1, (S - p - 0.5) / r) with
 *     r = end_i - start_{i+1}, each factor only where that overlap is positive; out = sum_k w_y w_x tile_k / sum_k w_y w_x over the covering
 *     tiles in ascending k, fp32.  Every output word is written once: no atomics, no memset; bitwise reproducible. */
int vvae_tile_gather_supported(int H, int W, int C, int S, int overlap);
int vvae_tile_gather_u8(const void* src, const float* lut, float* dst, int N, int T, int H, int W, int C, int S, int overlap, int ny, int nx,
                        int first, int count, void* stream);
int vvae_tile_blend_supported(int H, int W, int C, int S, int overlap, int dtype);
int vvae_tile_blend(const void* tiles, int dtype, float* out, int N, int T, int H, int W, int C, int S, int overlap, int ny, int nx,
                    void* stream);
/* Temporal windows (tiling.WindowPlan): a clip of L frames in windows of `frames` frames on the same grid as the tiles' axes (n_windows =
 * 1 if L <= frames, else ceil((L - t_overlap) / (frames - t_overlap)), 0 <= t_overlap <= frames / 2; window w starts at w (L - frames) /
 * (n_windows - 1)); each window is cut into the ny nx tiles above.
 *   window_blend: tiles (ring, ny nx, frames, S, S, C) contiguous, dtype VVAE_DT_F32 / VVAE_DT_BF16, window w in slot w % ring -> out fp32
 *     (L, H, W, C) contiguous, frames f_lo .. f_hi - 1 (every word written, no word outside them).  Weight of (w, ty, tx) at in-window
 *     frame q and in-tile (py, px): (w_t(w, q) w_y(ty, py)) w_x(tx, px), in that order, each factor as the tile blend's per axis; out =
 *     sum weight tile / sum weight over the covering (w, ty, tx) in ascending order, fp32 accumulation, no atomics, bitwise reproducible.
 *     A frame one window covers (w_t = 1) gets exactly vvae_tile_blend's value.  The windows covering [f_lo, f_hi) must be at most `ring`
 *     consecutive ones.  supported: as vvae_tile_blend, L <= 16384, at most 4 windows / tiles over one position of an axis. */
int vvae_window_blend_supported(int L, int frames, int t_overlap, int H, int W, int C, int S, int overlap, int dtype);
int vvae_window_blend(const void* tiles, int dtype, int ring, float* out, int L, int frames, int t_overlap, int n_windows, int f_lo, int f_hi,
                      int H, int W, int C, int S, int overlap, int ny, int nx, void* stream);
/* Temporal-difference error of consecutive frames (metrics.temporal_mse).  x, y (B, T, H, W, C) contiguous, each VVAE_DT_F32 or VVAE_DT_BF16,
 *      element-aligned; converted to fp32 and, with clamp != 0, clamped to [0, 1].  -> tmse fp32 (B, T - 1): tmse[b, t - 1] = mean over H W C of
 *      ((y_t - y_{t-1}) - (x_t - x_{t-1}))^2 for t = 1 .. T - 1 (nothing is launched or written for T == 1).  part: scratch of
 *      vvae_temporal_mse_part_floats(B, T, H, W, C) floats, written before it is read.  Two launches (per-chunk partial sums in a fixed
 *      order, then a fold over a pair's chunks in a fixed order); no atomics, bitwise reproducible.  supported: 1 <= C <= 4, H W C <= 2^30. */
int vvae_temporal_mse_supported(int H, int W, int C, int x_dtype, int y_dtype);
size_t vvae_temporal_mse_part_floats(int B, int T, int H, int W, int C);
int vvae_temporal_mse_fwd(const void* x, int x_dtype, const void* y, int y_dtype, float* tmse, float* part, int B, int T, int H, int W, int C,
                          int clamp, void* stream);
/* Scene-cut detection (video_vae_amd/scenes.py).  clip uint8 (L, H, W, 3) RGB contiguous.  tabs int32, 256 entries per table, built by the
 * caller: space 0 (HSV, OpenCV's 8-bit RGB -> HSV): [sdiv | hdiv | hbin | sbin], sdiv[i] = round((255 << 12) / i), hdiv[i] =
 * round((180 << 12) / (6 i)), both 0 at 0; bin of a pixel = hbin[H] hist_size + sbin[S].  space 1 (gray, Y = (4899 R + 9617 G + 1868 B + 8192)
 * >> 14): [gbin], bin = gbin[Y].  Every bin table entry must lie in 0 .. hist_size - 1.
 *   -> counts uint32 (L, bins), bins = hist_size^2 (HSV) or hist_size (gray): exact pixel counts; corr float64 (L - 1,): cv2.HISTCMP_CORREL of
 *      counts[f] and counts[f + 1] on the raw counts (s12 - s1 s2 / N over sqrt((s11 - s1^2 / N)(s22 - s2^2 / N)), N = bins, the sums exact
 *      64-bit integers; 1.0 when |denominator| <= DBL_EPSILON); not read for L == 1.
 *   part: scratch of vvae_scene_hist_part_bytes(L, H, W, hist_size, space) bytes (0: none needed, may be NULL), written before it is read.
 *   Up to three launches (per-chunk LDS histograms, a fold over a frame's chunks, the correlations); no global atomics, no fill launch,
 *   bitwise reproducible.  supported: 1 <= H <= 16384, 1 <= W <= 8192, hist_size 1 .. 64 (HSV) or 1 .. 256 (gray). */
int vvae_scene_hist_supported(int H, int W, int hist_size, int space);
size_t vvae_scene_hist_part_bytes(int L, int H, int W, int hist_size, int space);
int vvae_scene_hist_fwd(const void* clip, const int* tabs, unsigned* counts, double* corr, void* part, int L, int H, int W, int hist_size,
                        int space, void* stream);
/* The correlations alone, of counts uint32 (L, bins) already computed (1 <= bins <= 4096, L >= 2): corr float64 (L - 1,) as above, one launch. */
int vvae_scene_hist_corr(const unsigned* counts, double* corr, int L, int bins, void* stream);
/* Crop + bilinear resize of uint8 frames (video_vae_amd/data.py: resize_reference_u8, the host path's bytes).  src uint8 (n, H, W, C)
 * contiguous -> dst uint8 (n, out_h, out_w, C) contiguous: the crop [top, top + crop_h) x [left, left + crop_w) of every frame, resized
 * with half-pixel centres and clamped edge taps.  Per axis (input extent I, output extent O), fp32, round to nearest, nothing fused:
 * scale = float(I) / float(O); src = scale * (float(d) + 0.5f) - 0.5f, 0 when negative; i0 = min((int)src, I - 1), i1 = i0 + (i0 < I - 1);
 * l1 = src - float(i0), l0 = 1.0f - l1.  v = (a0 * ((b0 * s00) + (b1 * s01))) + (a1 * ((b0 * s10) + (b1 * s11))) with (a0, a1) the row
 * and (b0, b1) the column weights; out = v rounded to nearest even, clamped to 0 .. 255.  Equal extents copy.  One launch for any n; every
 * output byte written once, no byte outside dst touched: no atomics, no memset, no workspace; bitwise reproducible.
 * supported: every extent (H, W, crop, out) 1 .. 16384, 1 <= C <= 4, crop_h <= H, crop_w <= W; the launcher also refuses a crop that
 * does not lie inside the frame. */
int vvae_crop_resize_supported(int H, int W, int C, int crop_h, int crop_w, int out_h, int out_w);
int vvae_crop_resize_u8(const uint8_t* src, uint8_t* dst, int n, int H, int W, int C, int top, int left, int crop_h, int crop_w, int out_h,
                        int out_w, void* stream);
/* The same crop and resize, normalised: with q the byte vvae_crop_resize_u8 writes for an element, dst holds float(q) / 255.0f, a correctly
 * rounded IEEE fp32 division, as fp32 (dst_is_bf16 = 0) or rounded to nearest even to bf16 (dst_is_bf16 != 0); dst (n, out_h, out_w, C)
 * contiguous, aligned to its element.  It is the training loader's front end in one launch: u8.float() / 255 -> compute dtype behind the
 * resize.  Same refusals and guarantees as the u8 entry: one launch for any n, every output element written once, no atomics, no memset,
 * no workspace; safe inside a captured hipGraph. */
int vvae_crop_resize_norm(const uint8_t* src, void* dst, int dst_is_bf16, int n, int H, int W, int C, int top, int left, int crop_h,
                          int crop_w, int out_h, int out_w, void* stream);
/* Colour conversion between 8-bit Y'CbCr planes (YUV4MPEG2 clips) and RGB (video_vae_amd/y4m.py: yuv_to_rgb_reference and
 * rgb_to_yuv_reference are the definition, matched byte for byte; int32 arithmetic only).  chroma 0 = 4:2:0 (planes CH x CW, CH = (H + 1) / 2,
 * CW = (W + 1) / 2), 1 = 4:4:4 (H x W), 2 = mono (no chroma planes; u, v not read); siting 0 = centre, 1 = mpeg2 (horizontally co-sited;
 * 4:2:0 only, ignored otherwise); matrix 0 = bt601, 1 = bt709; full_range 0 = limited (luma 16 .. 235), else full.
 *   to_rgb: y (n, H, W), u, v (n, CH, CW) uint8, rows dense inside a frame; frame f of y at y + f y_frame_stride bytes, of u and v at
 *      u + f c_frame_stride and v + f c_frame_stride: the planes of frame records uploaded as they lie in a file, FRAME lines included.
 *      Bases and strides (>= 0) may have any alignment.  -> rgb uint8 (n, H, W, 3) contiguous.
 *   rgb_to_yuv: rgb uint8 (n, H, W, 3) contiguous -> y (n, H, W), u, v (n, CH, CW) uint8 contiguous; chroma 0 (centre siting) or 1.
 *   One launch for any n; every output byte written once, no byte outside the outputs touched: no atomics, no memset, no workspace;
 *   bitwise reproducible; safe inside a captured hipGraph.  supported: H, W 1 .. 16384, chroma 0 .. 2. */
int vvae_yuv_supported(int H, int W, int chroma);
int vvae_yuv_to_rgb_u8(const uint8_t* y, const uint8_t* u, const uint8_t* v, long y_frame_stride, long c_frame_stride, uint8_t* rgb, int n,
                       int H, int W, int chroma, int siting, int matrix, int full_range, void* stream);
int vvae_rgb_to_yuv(const uint8_t* rgb, uint8_t* y, uint8_t* u, uint8_t* v, int n, int H, int W, int chroma, int matrix, int full_range,
                    void* stream);
/* The training loader's front end on Y'CbCr planes, one launch: window -> RGB -> bilinear resize -> / 255 (video_vae_amd/y4m.py:
 * Y4MClip.window and window_to_rgb_reference are the definition of the operands and of the conversion; the resize and the division are
 * vvae_crop_resize_norm's with the window as the whole frame; the result is their composition bit for bit, with no RGB intermediate).
 *   y (n, H, W): the luma crop.  u, v: 4:2:0 (n, H / 2 + 3, W / 2 + 3), window row k = chroma row clamp((top >> 1) - 1 + k, 0, CH - 1) of the
 *      frame and columns likewise with left and CW, so the kernel clamps nothing; 4:4:4 (n, H, W); mono: not read.  All uint8, dense.
 *   clip_params int32 (ceil(n / frames_per_clip), 4) on the device: (top & 1, left & 1, full_range, 0); frame f uses row f / frames_per_clip.
 *   dst (n, out_h, out_w, 3) contiguous, fp32 or bf16 (dst_is_bf16 != 0), aligned to its element.  chroma, siting, matrix as above.
 *   One launch for any n; every output element written once, nothing outside dst touched, no byte outside the planes read: no atomics, no
 *   memset, no workspace; bitwise reproducible; safe inside a captured hipGraph.  supported: every extent 1 .. 16384, chroma 0 .. 2.
 *   vvae_yuv_window_span: the output pixels of a row that one workgroup spans (for tests and tools). */
int vvae_yuv_window_supported(int H, int W, int chroma, int out_h, int out_w);
int vvae_yuv_window_span(void);
int vvae_yuv_window_resize_norm(const uint8_t* y, const uint8_t* u, const uint8_t* v, const int* clip_params, void* dst, int dst_is_bf16,
                                int n, int frames_per_clip, int H, int W, int chroma, int siting, int matrix, int out_h, int out_w, void* stream);
/* Plane-wise metrics of two sets of 8-bit Y'CbCr planes (video_vae_amd/plane_metrics.py states the definition).  a = the reference, b = the
 * test; the planes of each are taken as vvae_yuv_to_rgb_u8 takes them: y (n, H, W), u, v (n, CH, CW) uint8, rows dense inside a frame,
 * frame f of y at y + f y_stride bytes, of u and v at u + f c_stride and v + f c_stride, any base alignment (the two operands may differ).
 * chroma 0 = 4:2:0, 1 = 4:4:4, 2 = mono (u, v not read).  -> sse int64 (n, 3): the exact sums of (a - b)^2 over the Y, U and V planes
 * (0 for the chroma of mono); ssim_y fp32 (n): the SSIM of vvae_recon_metrics_fwd of the Y planes as one-channel frames y / 255.
 *      ws: scratch of vvae_plane_metrics_ws_bytes(n, H, W, chroma) bytes, 8-byte aligned; every word that is read was written by the
 *      launch before.  Y is read once per operand (a band's halo rows again, from cache), nothing of plane size is written; dword loads
 *      where an operand's address lies on a dword, bytes elsewhere, no byte outside the planes read.  Three launches for any n (two for
 *      mono); no atomics, no memset, no allocation; bitwise reproducible; safe inside a captured hipGraph.
 *      supported: 11 <= H, W <= 8192, chroma 0 .. 2; ws_bytes returns 0 for a shape the kernels do not take. */
int vvae_plane_metrics_supported(int H, int W, int chroma);
size_t vvae_plane_metrics_ws_bytes(int n, int H, int W, int chroma);
int vvae_plane_metrics_u8(const uint8_t* ay, const uint8_t* au, const uint8_t* av, long a_y_stride, long a_c_stride, const uint8_t* by,
                          const uint8_t* bu, const uint8_t* bv, long b_y_stride, long b_c_stride, long long* sse, float* ssim_y, void* ws,
                          int n, int H, int W, int chroma, void* stream);
/* Latent quantiser (video_vae_amd/quant.py: quantise_reference is the definition, matched bit for bit).  latent (frames, hw, ld) bf16 or fp32
 * contiguous, 16-byte aligned; keep fp32 (frames,): nonzero = quantise the frame.  bits 2 .. 8, qmax = 2^(bits - 1) - 1.  Per kept frame and
 * channel c, fp32, every operation rounded on its own: amax = max_i |x[i, c]|; dead (amax zero, not finite or < 1e-30f): step 0, codes 0;
 * else inv = float(qmax) / amax, step = amax / float(qmax) (IEEE divisions, once per channel), q = clamp(rint(x inv), -qmax, qmax) with ties
 * to even.
 *   -> codes int8 (frames, hw, ld), 8-byte aligned; step fp32 (frames, ld); counts uint32 (frames, 256), counts[f][q + 128] = elements of
 *      frame f with code q; dequantise != 0: float(q) step, rounded to the latent's dtype, written over the kept frames of latent.
 *   A frame whose keep flag is zero is not read or written in latent; its codes, steps and counts are zeros.  One launch, one workgroup per
 *   frame; every output element written by every launch; LDS integer atomics only: no global atomics, no memset, no workspace; bitwise
 *   reproducible; safe inside a captured hipGraph.  supported: hw >= 1, ld a multiple of 8 in 8 .. 1024, hw ld <= 2^30. */
int vvae_latent_quantise_supported(int hw, int ld, int dtype);
int vvae_latent_quantise(void* latent, int dtype, const float* keep, int8_t* codes, float* step, unsigned* counts, int frames, int hw, int ld,
                         int bits, int dequantise, void* stream);
/* The same quantiser inside the train step (quant.fake_quant_reference is the definition, matched bit for bit), out of place: src and dst
 * (frames, hw, ld) bf16 or fp32, contiguous, 16-byte aligned, disjoint (src == dst or overlapping buffers: VVAE_ERR_BAD_ARG).  A frame whose
 * keep flag is nonzero: dst = float(q) step rounded to the dtype, through the integer code (a code 0 gives +0.0); any other frame: dst = src,
 * copied as 16-byte words.  src is only read, every element of dst is written; no codes and no steps are written.  counts_or_null: uint32
 * (frames, 256) as above (zeros for a dropped frame), or null for none.  Shapes: vvae_latent_quantise_supported.  One launch, one workgroup
 * per frame, 16-byte stores, LDS integer atomics only: no global atomics, no memset, no workspace; bitwise reproducible; safe inside a
 * captured hipGraph. */
int vvae_latent_fake_quant(const void* src, void* dst, int dtype, const float* keep, unsigned* counts_or_null, int frames, int hw, int ld,
                           int bits, void* stream);
/* The rate term of quantisation-aware training (quant.rate_reference is the definition): the cost table cost256 fp32 (256,), bits per code
 * at index q + 128 (quant.rate_cost_reference), interpolated linearly at the unrounded code.  Per kept frame and live channel c, with amax,
 * dead and inv those of the quantiser, fp32, every operation rounded on its own: v = x inv[c], k = clamp(floor(v), -qmax, qmax - 1),
 * d = C[k + 129] - C[k + 128], term = C[k + 128] + (v - k) d, slope = d inv[c]; a dead channel gives 0 and 0.
 *   vvae_latent_rate: rate fp32 (frames,) = the sum of the frame's terms (per-thread sums in a fixed order, then one fixed-order workgroup
 *   reduction), 0 for a frame whose keep flag is zero, which is not read.
 *   vvae_latent_rate_grad: grad (frames, hw, ld) of x's dtype = g[f] slope rounded to the dtype, g fp32 (frames,); a frame whose keep flag
 *   or g[f] is zero is written as zero words and x is not read there.  grad overlapping x: VVAE_ERR_BAD_ARG.
 * x (frames, hw, ld) bf16 or fp32, contiguous, 16-byte aligned (so is grad), only read.  Shapes: vvae_latent_quantise_supported.  One launch
 * each, one workgroup per frame, every output element written by every launch; LDS integer atomics only: no float atomics, no global
 * atomics, no memset, no workspace; bitwise reproducible; safe inside a captured hipGraph. */
int vvae_latent_rate(const void* x, int dtype, const float* keep, const float* cost256, float* rate, int frames, int hw, int ld, int bits,
                     void* stream);
int vvae_latent_rate_grad(const void* x, int dtype, const float* keep, const float* cost256, const float* g, void* grad, int frames, int hw,
                          int ld, int bits, void* stream);
/* Interleaved rANS over the quantiser's codes (video_vae_amd/entropy.py: encode_reference / decode_reference are the definition, matched on
 * every word, count and state): 32-bit states, 16-bit words, scale 2^12, lower bound 2^16, 64 lanes; symbol i of a frame (code + qmax,
 * row-major over (hw, ld)) belongs to lane i mod 64 and step i div 64.  freq uint16 (2 qmax + 1,) sums to 4096 and is positive on every
 * code that occurs in a coded frame.  One wavefront per frame, grid = frames; the words move between lanes by ballot and v_mbcnt only.
 *   encode: codes int8 (frames, hw, ld), keep fp32 (frames,) -> words uint16 (frames, cap), cap = ceil(hw ld / 64) 64: frame f's stream,
 *      in the order the decoder reads it, is the LAST n_words[f] entries of its row (the head of the row is not written); n_words int32
 *      (frames,); state uint32 (frames, 64).  A frame whose keep flag is zero is not read: n_words 0, states 2^16.
 *   decode: words uint16 (total_words,), offsets int64 (frames,), n_words, state, freq as above -> codes int8 (frames, hw, ld); ok int32
 *      (frames,): 1 when the frame's stream lies inside words, every word of it was consumed and every lane ended at 2^16.  No read leaves
 *      [offsets[f], offsets[f] + n_words[f]) cut to [0, total_words); past its end a read yields 0.
 *   No global atomics, no memset, no workspace; bitwise reproducible; safe inside a captured hipGraph.  supported: bits 2 .. 8, hw >= 1,
 *   ld >= 1, hw ld <= 2^30. */
int vvae_rans_supported(int hw, int ld, int bits);
int vvae_rans_encode(const int8_t* codes, const float* keep, const uint16_t* freq, uint16_t* words, int* n_words, uint32_t* state, int frames,
                     int hw, int ld, int bits, void* stream);
int vvae_rans_decode(const uint16_t* words, long total_words, const long* offsets, const int* n_words, const uint32_t* state,
                     const uint16_t* freq, int8_t* codes, int* ok, int frames, int hw, int ld, int bits, void* stream);
/* The context coder (entropy.py: encode_context_reference / decode_context_reference, matched on every count, word, state and code): the
 * coder above with K = 4 tables freq4 uint16 (4, 2 qmax + 1), every row summing to 4096.  With E[j] = sum_c |code[j, c]| the energy of token
 * j, a symbol of token j uses table 0 when j < grid_w and table 1 + (E[j - grid_w] > thr0) + (E[j - grid_w] > thr1) otherwise.
 *   counts: codes, keep -> counts int32 (frames, 4, 256), counts[f][ctx][code + 128] (the quantiser's histogram layout per context); zeros
 *      for a frame whose keep flag is zero, which is not read.  One workgroup per frame, LDS integer adds; the caller sums the frames.
 *   encode_ctx / decode_ctx: the arguments and results of vvae_rans_encode / vvae_rans_decode.  One wavefront per frame; the energies live
 *      in LDS (encode: computed first, one more read of the frame; decode: added up from the decoded codes as the steps proceed).
 *      slot_form 0: a byte per slot (the symbol) and a second read of the context's table; 1: four full slot tables, 64 KB of dynamic LDS;
 *      -1: the full tables while frames <= the device's CUs (the shorter chain), the compact ones beyond (three waves a CU instead of
 *      one).  Both forms compute the same.
 *   No global atomics, no memset, no workspace; bitwise reproducible; safe inside a captured hipGraph.  supported: vvae_rans_supported,
 *   hw <= 4096 (the energies are 16 KB of LDS), grid_w >= 1 and (grid_w - 1) ld >= 63 (every symbol of the token above is decoded in an
 *   earlier step than any symbol of the token below it). */
int vvae_rans_context_supported(int hw, int ld, int bits, int grid_w);
int vvae_rans_context_counts(const int8_t* codes, const float* keep, int* counts, int frames, int hw, int ld, int bits, int grid_w, int thr0,
                             int thr1, void* stream);
int vvae_rans_encode_ctx(const int8_t* codes, const float* keep, const uint16_t* freq4, uint16_t* words, int* n_words, uint32_t* state,
                         int frames, int hw, int ld, int bits, int grid_w, int thr0, int thr1, void* stream);
int vvae_rans_decode_ctx(const uint16_t* words, long total_words, const long* offsets, const int* n_words, const uint32_t* state,
                         const uint16_t* freq4, int8_t* codes, int* ok, int frames, int hw, int ld, int bits, int grid_w, int thr0, int thr1,
                         int slot_form, void* stream);
/* The temporal coder (entropy.py: encode_temporal_reference / decode_temporal_reference, matched on every count, word, state and code): nine
 * tables freq9 (9, 2 qmax + 1); a frame that starts a chain uses row 0, a chained frame the row 1 + #{k : q_prev > thr[k]} of the code at
 * the same token and channel of the frame before it.  thr: 7 ascending integers on the HOST (kernel arguments).
 *   counts: codes, keep, prev int32 (frames,) (the frame a kept frame is coded against, -1 for a chain start; an index that names no frame
 *      counts as -1) -> counts int32 (frames, 9, 256), counts[f][row][code + 128]; zeros for a frame whose keep flag is zero, which is not
 *      read.  One workgroup per frame; runs of equal (row, code) are added to an LDS histogram with integer adds.
 *   encode_temporal: the arguments and results of vvae_rans_encode, and prev.  One wavefront per frame (the encoder knows every code).
 *   decode_temporal: the arguments and results of vvae_rans_decode, and chain_start int32 (chains + 1,) on the device: chain c holds the
 *      frames chain_start[c] .. chain_start[c + 1] - 1; the chains partition the frames (then every code and ok is written; an entry
 *      outside 0 .. frames is cut to it).  One wavefront per chain decodes its frames in order, each lane reading back the code it stored
 *      at the same step of the frame before; ok is one flag per frame.  Compact slot tables (a byte per slot), 50 KB of LDS a wave.
 *   No global atomics, no memset, no workspace; bitwise reproducible; safe inside a captured hipGraph.  supported: vvae_rans_supported. */
int vvae_rans_temporal_supported(int hw, int ld, int bits);
int vvae_rans_temporal_counts(const int8_t* codes, const float* keep, const int* prev, int* counts, int frames, int hw, int ld, int bits,
                              const int* thr, void* stream);
int vvae_rans_encode_temporal(const int8_t* codes, const float* keep, const int* prev, const uint16_t* freq9, uint16_t* words, int* n_words,
                              uint32_t* state, int frames, int hw, int ld, int bits, const int* thr, void* stream);
int vvae_rans_decode_temporal(const uint16_t* words, long total_words, const long* offsets, const int* n_words, const uint32_t* state,
                              const uint16_t* freq9, int8_t* codes, int* ok, const int* chain_start, int chains, int frames, int hw, int ld,
                              int bits, const int* thr, void* stream);

/* ---- y = silu(x) over a contiguous bf16 tensor of n elements (n % 8 == 0): the activation between the MLP's two Linear layers
 *      (train/layers.py:186-189). ---- */
int vvae_silu_bf16(const void* x, void* y, long n, void* stream);
/* Read-only query, used by the launcher itself: workgroups of 256 for nvec = n / 8 vectors (four per lane and trip, then a grid stride). */
int vvae_silu_blocks(long nvec);

/* ---- Linear + bias + residual in one library product: y (M,N) = x (M,K) w (K,N) + bias (N) + res (M,N), bf16, fp32 accumulation.
 *      The Linear that closes an attention / MLP branch followed by `x = x + branch` (train/layers.py:212-221, 151, 189): hipBLASLt
 *      reads the residual stream as its C operand (beta = 1, C != D), so the add costs no pass of its own.  bias: NULL / bf16 / fp32
 *      (bias_dtype); res: NULL = plain Linear; ws: device scratch for the library (16-byte aligned; 0 allowed). ---- */
int vvae_linear_residual_bf16(const void* x, int ldx, const void* w, int ldw, const void* bias, int bias_dtype, const void* res, int ldr,
                              void* y, int ldy, int M, int N, int K, void* ws, size_t ws_bytes, void* stream);
/* The same product with the weight given as its (N, K) row-major transpose, pitch ldwt >= K (the optimizer's second bf16 shadow). */
int vvae_linear_residual_wt_bf16(const void* x, int ldx, const void* wt, int ldwt, const void* bias, int bias_dtype, const void* res, int ldr,
                                 void* y, int ldy, int M, int N, int K, void* ws, size_t ws_bytes, void* stream);

/* ---- PatchUnEmbedding's "b t (h w) (p1 p2 cu) -> b t (h p1) (w p2) cu" (train/layers.py:48) fused with the zero padding of the
 *      channel axis from cu to c (the multiple of 16 the conv kernels take), and its transpose.  frames = b*t; bf16; cu, c % 4 == 0. ---- */
int vvae_unpatch_pad_fwd(const void* x, void* y, long frames, int h, int w, int p, int cu, int c, int dtype, void* stream);
int vvae_unpatch_pad_bwd(const void* g, void* gx, long frames, int h, int w, int p, int cu, int c, int dtype, void* stream);

/* ---- GroupNorm(G, eps) + SiLU: nnx.GroupNorm + nnx.silu at train/unet.py:22-23,28-29.
 *      sums: fp64 [N][G][2] (sum, sum of squares) produced by vvae_gn_stats; S = voxels per sample. ---- */
size_t vvae_gn_part_floats(int N, long S, int C);   /* fp32 scratch floats for `part` below (per-workgroup partial sums) */
int vvae_gn_stats(const void* x, int ldx, int N, long S, int C, int G, double* sums, float* part, int dtype, void* stream);
int vvae_gn_finalize(const float* part, int N, int nblk, int G, double* sums, void* stream);   /* second half of vvae_gn_stats for partials written by vvae_conv3d_fwd_bf16_gn */
int vvae_gn_silu_fwd(const void* x, int ldx, void* y, int ldy, const double* sums, const float* gamma, const float* beta,
                     int N, long S, int C, int G, float eps, int dtype, void* stream);
/* silu(GroupNorm(x)) and its (1,2,2) max-pool in one launch (conv2 -> GN -> SiLU -> max_pool of an encoder level, train/unet.py:44-51):
 * y (N,T,H,W,C) pitch ldy, pool (N,T,H/2,W/2,C) pitch ldp; `sums` as for vvae_gn_silu_fwd. */
int vvae_gn_silu_pool_supported(int H, int W, int C, int G, int ldx, int ldy, int ldp, int dtype);
int vvae_gn_silu_pool_fwd(const void* x, int ldx, void* y, int ldy, void* pool, int ldp, const double* sums, const float* gamma,
                          const float* beta, int N, int T, int H, int W, int C, int G, float eps, int dtype, void* stream);
int vvae_gn_silu_bwd(const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx, const double* sums,
                     const float* gamma, const float* beta, double* csum /* fp64 [N][C][2] scratch */, float* part,
                     float* dgamma, float* dbeta, int N, long S, int C, int G, float eps, int dtype, void* stream);

/* ---- max-pool (1,2,2)/(1,2,2): nnx.max_pool at train/unet.py:50.  NT = n*t planes; H, W = input size.
 *      bwd: dx = (dskip ? dskip : 0) + scatter(dpool) to the first arg-max of each window. ---- */
int vvae_maxpool_1x2x2_fwd(const void* x, int ldx, void* y, int ldy, int NT, int H, int W, int C, int dtype, void* stream);
int vvae_maxpool_1x2x2_bwd(const void* x, int ldx, const void* dpool, int lddp, const void* dskip, int ldds,
                           void* dx, int lddx, int NT, int H, int W, int C, int dtype, void* stream);
/* Read-only queries, used by the two launchers themselves.  vvae_pool_vec: elements per lane this operand (pointer p, pitch ld) allows,
 * 8 (bf16) or 4 (fp32) where C and ld are multiples of it and p is 16-byte aligned, else 1 (also for an unknown dtype); a launch runs the
 * vector form only if every operand of it returns the vector width.  vvae_pool_blocks: workgroups of 256 for `items` lane items
 * (NT * H/2 * W/2 * C / vec); the kernels walk the items with a grid stride. */
int vvae_pool_vec(const void* p, int ld, int C, int dtype);
int vvae_pool_blocks(long items);

/* ---- ConvTranspose kernel (1,2,2) strides (1,2,2): nnx.ConvTranspose at train/unet.py:61-69,78.
 *      out[2i+d] = x[i] * K[1-d] per spatial axis (kernel NOT flipped).  H, W = input (low) resolution. ---- */
int vvae_convt_1x2x2_fwd(const void* x, int ldx, const float* w, const float* bias, void* y, int ldy,
                         int NT, int H, int W, int Cin, int Cout, int dtype, void* stream);
int vvae_convt_1x2x2_dgrad(const void* dy, int lddy, const float* w, void* dx, int lddx,
                           int NT, int H, int W, int Cin, int Cout, int dtype, void* stream);
size_t vvae_convt_1x2x2_wgrad_ws_bytes(int NT, int H, int W, int Cin, int Cout);   /* per-chunk fp32 partials, folded in index order (no atomics) */
int vvae_convt_1x2x2_wgrad(const void* x, int ldx, const void* dy, int lddy, float* dw,
                           int NT, int H, int W, int Cin, int Cout, int dtype, void* ws, size_t ws_bytes, void* stream);
/* bf16 MFMA path (weights in registers, no LDS) for the UNet decoder shapes 128->64, 64->32, 32->16:
 * dgrad = 0: x -> y (+bias); dgrad = 1: "x" is dy (2H x 2W, Cout), "y" is dx (H x W, Cin).  ws: packed weights. */
/* bf16 matrix-core weight + bias gradient of the same layer (128->64, 64->32, 32->16): deterministic slab reduction. */
int vvae_convt_wgrad_bf16_supported(int Cin, int Cout, int ldx, int lddy);
size_t vvae_convt_wgrad_bf16_ws_bytes(int NT, int H, int W, int Cin, int Cout);
int vvae_convt_1x2x2_wgrad_bf16(const void* x, int ldx, const void* dy, int lddy, float* dw, float* dbias, int NT, int H, int W,
                                int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int vvae_convt_bf16_supported(int Cin, int Cout, int ld_in, int ld_out);
size_t vvae_convt_bf16_ws_bytes(int Cin, int Cout);
int vvae_convt_1x2x2_bf16(const void* x, int ldx, const float* w, const float* bias, void* y, int ldy,
                          int NT, int H, int W, int Cin, int Cout, int dgrad, void* ws, size_t ws_bytes, void* stream);
/* dgrad bit 8 (0x100): ws already holds that direction's packed weights, written by this call for n <= 16 kernels in one launch
 * (host arrays of device pointers / ints; ws[i] >= vvae_convt_bf16_ws_bytes(Cin[i], Cout[i]) bytes): once per optimizer step. */
int vvae_convt_pack_grouped_bf16(const float* const* w, void* const* ws, const int* Cin, const int* Cout, const int* dgrad, int n, void* stream);

/* ---- temporal attention core: q_norm/k_norm + RoPE + masked softmax(QK^T/sqrt(D))V,
 *      train/layers.py:159-170 (called from FactoredAttention, layers.py:212-213).
 *      qkv (A,T,3*heads*D) pitch ld; mask uint8 (ceil(A/mask_div), T) 1 = attend, or NULL. ---- */
int vvae_temporal_attn_fwd(const void* qkv, int ld, void* out, int ldo, const float* q_scale, const float* k_scale,
                           const float* cos_table, const float* sin_table, const uint8_t* mask, int mask_div,
                           int A, int T, int heads, int D, float eps, int dtype, void* stream);
size_t vvae_temporal_attn_bwd_ws_bytes(int A, int heads, int D);   /* partial rows of the q/k-norm scale gradients (no atomics) */
int vvae_temporal_attn_bwd(const void* qkv, int ld, const void* dout, int lddo, void* dqkv, int lddq,
                           const float* q_scale, const float* k_scale, const float* cos_table, const float* sin_table,
                           const uint8_t* mask, int mask_div, float* dq_scale, float* dk_scale,
                           int A, int T, int heads, int D, float eps, int dtype, void* ws, size_t ws_bytes, void* stream);

/* lane-per-frame form of the same core for head_dim D in {8,16,32,64} (the production path): forward also writes the
 * row log-sum-exp `lse` (A*heads, T) fp32; backward consumes (out, lse) and writes per-workgroup partials of the
 * cos_table / sin_table of the _fast, qk_prep and spatial entry points: fp32 values ALREADY rounded to the activation dtype.
 * q_norm / k_norm scale gradients: dscale_part (vvae_temporal_attn_fast_blocks(...), 2*D) fp32, summed by the caller.
 * inner = 1: sequences contiguous (A,T,C).  inner = hw: tensors are (b,t,hw,C), sequence a = b*hw+i strides over frames
 * (no transpose copies around the temporal half of FactoredAttention). */
int vvae_temporal_attn_fast_supported(int T, int D, int ld, int ldo, int dtype);
int vvae_temporal_attn_fast_blocks(int A, int T, int heads, int D, int dtype);
int vvae_temporal_attn_mfma_enable(int on);   /* test hook: 0 = keep bf16 / T = 16 / head_dim 64 on the VALU kernels (default 1: matrix cores) */
int vvae_temporal_attn_mfma_config(int max_workgroups);   /* test / tuning hook: cap on the persistent workgroups of one launch of the T = 16 matrix-core
                                                            kernels; 0 (default) = as many as the chip keeps resident.  Results do not depend on it */
int vvae_temporal_attn_mfma32_enable(int on);   /* test hook: 0 = T = 32 / 64 temporal attention on the VALU kernels again */
int vvae_temporal_attn_fwd_fast(const void* qkv, int ld, void* out, int ldo, float* lse, const float* q_scale,
                                const float* k_scale, const float* cos_table, const float* sin_table, const uint8_t* mask,
                                int mask_div, int inner, int A, int T, int heads, int D, float eps, int dtype, void* stream);
int vvae_temporal_attn_bwd_fast(const void* qkv, int ld, const void* out, int ldo, const void* dout, int lddo, const float* lse,
                                void* dqkv, int lddq, const float* q_scale, const float* k_scale, const float* cos_table,
                                const float* sin_table, const uint8_t* mask, int mask_div, int inner, float* dscale_part,
                                int A, int T, int heads, int D, float eps, int dtype, void* stream);

/* ---- q/k-norm + RoPE prep around a library attention core (spatial half of FactoredAttention, train/layers.py:153-170,217-221).
 *      fwd: qkv (tokens, 3*heads*D) -> out (tokens, 2*heads*D) = [rope(q_norm(q)) | rope(k_norm(k))]; RoPE position = token % S.
 *      bwd: (dq', dk', dv) with element strides (token, head) -> dqkv (tokens, 3*heads*D), all three sections, one launch;
 *           scale-gradient partials part (vvae_qk_prep_blocks(...), 2, D) fp32: [dq_scale | dk_scale], summed by the caller. ---- */
int vvae_qk_prep_supported(int D, int dtype);
int vvae_qk_prep_blocks(long tokens, int heads, int D);
int vvae_qk_prep_fwd(const void* qkv, int ld, void* out, int ldo, const float* q_scale, const float* k_scale,
                     const float* cos_table, const float* sin_table, long tokens, int S, int heads, int D, float eps,
                     int dtype, void* stream);
int vvae_qk_prep_bwd(const void* qkv, int ld, const void* dq, long dq_ts, long dq_hs, const void* dk, long dk_ts, long dk_hs,
                     const void* dv, long dv_ts, long dv_hs, void* dqkv, int lddq, const float* q_scale, const float* k_scale,
                     const float* cos_table, const float* sin_table, float* part, long tokens, int S, int heads, int D,
                     float eps, int dtype, void* stream);

/* ---- fused spatial attention (sequence = h*w patches of a frame, train/layers.py:153-170,217-221): q/k-norm + RoPE +
 *      softmax(QK^T/sqrt(D))V in one kernel per direction; bf16, head_dim 64, S % 32 == 0, S <= 256, no mask.
 *      qkv (A*S, 3*heads*D) row pitch ld; out (A*S, heads*D) row pitch ldo; lse2 fp32 (A*heads, S) (base-2 log-sum-exp). ---- */
int vvae_spatial_attn_supported(int S, int D, int dtype);
int vvae_spatial_attn_fwd(const void* qkv, int ld, void* out, int ldo, float* lse2, const float* q_scale, const float* k_scale,
                          const float* cos_table, const float* sin_table, int A, int S, int heads, int D, float eps, int dtype,
                          void* stream);
/* part: fp32 (A*heads, 2, D) per-(sequence, head) partials of [dq_scale | dk_scale]; dqkv fully written (q, k, v sections). */
int vvae_spatial_attn_bwd(const void* qkv, int ld, const void* out, int ldo, const void* dout, int lddo, const float* lse2,
                          void* dqkv, int lddq, const float* q_scale, const float* k_scale, const float* cos_table,
                          const float* sin_table, float* part, int A, int S, int heads, int D, float eps, int dtype, void* stream);

/* ---- LayerNorm(eps, fast variance, fp32 stats): nnx.LayerNorm at train/layers.py:17,152,155-156,178.
 *      x row r at x + (r / inner) * outer_pitch + (r % inner) * inner_pitch (elements); y, dy, dx contiguous (rows, C).
 *      bwd writes per-workgroup partials part (vvae_layernorm_bwd_blocks(...), 2, C): [sum dy*xhat | sum dy]. ---- */
int vvae_layernorm_supported(int C, int dtype);
int vvae_layernorm_bwd_blocks(long rows, int C, int dtype);
int vvae_delay_us(int us, void* stream);   /* measurement aid: occupy the stream for ~us microseconds (1..1000), see ops.KernelTimer */
int vvae_layernorm_fwd(const void* x, void* y, const float* gamma, const float* beta, float* mean, float* rstd,
                       const void* addend, void* xsum, long rows, int C, int inner, long outer_pitch, long inner_pitch, float eps,
                       int dtype, void* stream);   /* addend/xsum non-NULL: normalise round(x + addend), write the sum to xsum */
int vvae_layernorm_bwd(const void* x, const void* dy, const float* gamma, const float* mean, const float* rstd, const void* dres,
                       void* dx, float* part, long rows, int C, int inner, long outer_pitch, long inner_pitch, int dtype,
                       void* stream);

/* ---- reparameterise + KL: train/model.py:124-128, train/rl_nonadversarial.py:146-147. ---- */
size_t vvae_loss_part_floats(int B, long M);   /* fp32 scratch floats for `part` below (M = elements per sample): per-workgroup
                                                  partial sums, folded in fixed order -- no float atomics, bitwise reproducible */
int vvae_reparam_kl_fwd(const void* mean, const void* logvar, const float* eps, const float* mask, float* z, float* kl,
                        float* part, int B, int T, long per, int dtype, void* stream);
int vvae_reparam_kl_bwd(const void* mean, const void* logvar, const float* eps, const float* mask, const float* dz,
                        const float* gkl, void* dmean, void* dlogvar, int B, int T, long per, int dtype, void* stream);

/* ---- masked MSE / MAE: train/rl_nonadversarial.py:114-121.  video sample = b / video_div (pair doubling).  mse = mae = NULL: no fold, the
 *      caller reads part = [mse (B, chunks) | mae (B, chunks)], chunks = vvae_loss_part_floats / (2 B). ---- */
int vvae_masked_mse_mae_fwd(const void* video, const void* recon, const float* mask, float* mse, float* mae,
                            float* part, int B, int T, long P, int video_div, int dtype, void* stream);
int vvae_masked_mse_mae_bwd(const void* video, const void* recon, const float* mask, const float* gmse, const float* gmae,
                            void* drecon, int B, int T, long P, int video_div, int dtype, void* stream);

/* ---- weight-gradient GEMM of the dense layers (nnx.Linear under autodiff, train/layers.py:15,142-151,179-189):
 *      C[M][N] fp32 = sum_k A[k][m] * B[k][n], db[n] = sum_k B[k][n]; A (K,M), B (K,N) bf16 token-major. ---- */
int vvae_gemm_tn_supported(int M, int N, int K, int lda, int ldb);
size_t vvae_gemm_tn_ws_bytes(int M, int N, int K);
int vvae_gemm_tn_bf16(const void* A, int lda, const void* B, int ldb, float* C, float* db, int M, int N, int K,
                      void* ws, size_t ws_bytes, void* stream);
/* Grouped form: n <= 64 weight gradients that share K in one launch, one whole-K 256x256 tile per workgroup (no split-K slabs,
 * no reduction pass): C_i (M_i, N_i) fp32 contiguous = A_i^T B_i, db_i (N_i) or NULL; M_i, N_i % 256 == 0, K % 32 == 0.  The arrays
 * are host arrays of device pointers / ints. */
int vvae_gemm_tn_grouped_bf16(const void* const* A, const int* lda, const void* const* B, const int* ldb, float* const* C,
                              float* const* db, const int* M, const int* N, int n, int K, void* stream);
int vvae_gemm_tn_use_big_tiles(int on);   /* test hook: 0 = 128x128 kernel for every shape */

/* ---- optimiser: optax.chain(clip_by_global_norm, adam) at train/rl_nonadversarial.py:248-251. ---- */
/*      The global norm is reduced without atomics: vvae_sqnorm_partials writes vvae_sqnorm_blocks(n) fp64 partial sums of squares,
 *      every workgroup of vvae_adam_clip_step folds them in one fixed order (so every rank of a data-parallel job, holding the
 *      same all-reduced gradient, applies the bitwise-same clip factor) and the total lands in *gnorm_sq_out.
 *      acc (n fp32) or NULL, in both entries: the gradient is g[i] + acc[i] (gradient accumulation: acc the fp32 sum of the earlier
 *      micro-steps, so the last one of a cycle needs no fold pass of its own; gscale then carries 1 / K).  g and a given acc 16-byte aligned
 *      for the norm.  ema (n fp32) or NULL: the same pass also advances a weight average, ema = ema_decay * ema + (1 - ema_decay) * p_new,
 *      p_new the fp32 parameter of this step; ema_decay in [0, 1) (a host scalar per step), and 0 with ema NULL, else VVAE_ERR_BAD_ARG.
 *      acc and ema select compile-time variants of one kernel each, same grid, fold and clip factor: p, m, v, the shadow and *gnorm_sq_out
 *      come out bitwise the same with and without ema. */
int vvae_sqnorm_blocks(long n);
int vvae_sqnorm_partials(const float* g, const float* acc, long n, double* part, void* stream);
int vvae_adam_clip_step(float* p, const float* g, const float* acc, float* m, float* v, void* p_bf16, long n, const double* gnorm_part,
                        int nparts, double* gnorm_sq_out, float gscale, float max_norm, float lr, float b1, float b2, float eps,
                        long count, float* ema, float ema_decay, void* stream);
/*      Gradient accumulation (optax.MultiSteps semantics, fp32 sum in arrival order).  vvae_grad_fold_f32: dst = (overwrite ? 0 : dst) + src
 *      over n floats with 16-byte accesses (scalar where an operand is not 16-byte aligned), nothing outside [0, n) touched; NULL,
 *      dst == src or n <= 0: VVAE_ERR_BAD_ARG. */
int vvae_grad_fold_f32(float* dst, const float* src, long n, int overwrite, void* stream);
/*      a <-> b over n floats in one pass; a_bf16 (n bf16, or NULL) = bf16(new a).  Evaluation with the averaged weights swaps them into
 *      the parameter buffer and back, so no pointer held by a captured graph changes. */
int vvae_swap_refresh_f32(float* a, float* b, void* a_bf16, long n, void* stream);
int vvae_cast_f32_to_bf16(const float* x, void* y, long n, void* stream);
/* ---- dense-layer GEMM, both operands K-contiguous: C (M,N) bf16 = epi(A (M,K) . B (N,K)^T + bias), fp32 accumulation.
 *      Linear forward (B = transposed bf16 weight shadow) and input gradient (B = the weight itself) of nnx.Linear at
 *      train/layers.py:15,142-151,179-189.  epi 0 none; 1 + res (residual add); 2 SiLU, rounded pre-activation -> C2;
 *      3 * silu'(res) (res = saved pre-activation).  The elementwise tail acts on the bf16-rounded linear output. ---- */
int vvae_gemm_nt_supported(int M, int N, int K, int lda, int ldb, int ldc);
int vvae_gemm_nt_bf16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, const float* bias, const void* res,
                      int ldr, void* C2, int ldc2, int epi, int M, int N, int K, void* stream);
/* The same product on the second kernel form (csrc/gemm_pp.hip: all LDS-DMA staging issued from the read phases -- the token operand through a
 * ring of three slots by waves 4-7, the weight operand through two by waves 0-3 -- so that the MFMA phases are bare MFMAs; one stream of k-tiles over
 * the tiles a workgroup walks; a per-wave epilogue under the partner wave's MFMA phase).  Arguments and results as vvae_gemm_nt_bf16 (bit for
 * bit); additionally K >= 128 and N <= 1536 (N a multiple of 192) or 2048 (of 128): the bias vector of the launch is staged in LDS. */
int vvae_gemm_pp_supported(int M, int N, int K, int lda, int ldb, int ldc);
int vvae_gemm_pp_bf16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, const float* bias, const void* res,
                      int ldr, void* C2, int ldc2, int epi, int M, int N, int K, void* stream);
/* Timing-only hook of the -DPP_ABLATION build of vvae_gemm_pp_bf16 (tools/pp_ablation.py): bit 0 no DMA, bit 1 no fragment reads, bit 2 no MFMAs
 * in the plain product's main loop (wrong results); the shipped library ignores it. */
int vvae_gemm_pp_ablate(int bits);
/* Tuning hook of vvae_gemm_pp_bf16: 1 (default) = the last epilogue of a launch goes through the idle operand rings, all units of a wave at once; 0 = unit by unit. */
int vvae_gemm_pp_final_ring(int on);
/* Test / tuning hook: 0 = one tile per workgroup, 1 = persistent workgroups over tiles b, b + 256, ... (default). */
int vvae_gemm_nt_persistent(int on);
/* Test / tuning hook: L2 prefetch distance (k-tiles of 64) of the token panel in vvae_gemm_nt_bf16 (default 3, 0 = off); epilogue kinds 0 and 2
 * (plain, SiLU pair) prefetch at that distance, 1 and 3 never do. */
int vvae_gemm_nt_prefetch(int dist);

/* out[c] = sum_r part[r][c] in fixed order: folds the per-workgroup partial rows of the backward kernels (cols % 4 == 0). */
int vvae_sum_rows(const float* part, int rows, int cols, float* out, void* stream);
/* n <= 64 partial buffers folded in one launch: part[i] fp32 (rows[i], cols[i]); columns [0, n0[i]) -> d0[i], the rest -> d1[i] (or NULL). */
int vvae_fold_rows_grouped(const void* const* part, float* const* d0, float* const* d1, const int* rows, const int* cols,
                           const int* n0, int n, void* stream);
/* n <= 64 contiguous fp32 ranges copied in one launch (gradients landing in the optimizer's flat buffer; replaces the
   per-parameter copies of optax's tree_map update path, reference train/rl_nonadversarial.py:233-236) */
int vvae_copy_grouped(const float* const* src, float* const* dst, const long* count, int n, void* stream);

/* Test hook: y[i] = x[i ^ o] within each group of 64 floats (o in {1,2,4,8,16,32}, n % 64 == 0), yd likewise in fp64 (scaled by
   1.000000001): the VALU-only lane exchange (DPP + v_permlane16/32_swap) every wave-level reduction of this library uses. */
int vvae_selftest_xor_lane(const float* x, float* y, double* yd, int n, int o, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VVAE_HIP_H */
