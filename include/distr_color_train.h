/*
 * distr_color_train.h -- C ABI of libdistr.so, part 10: the colour stage's decoder list, written out, and the photometric loss of a
 * batch of colour images. Included by distr.h; new functions only (DISTR_ABI_VERSION and every struct stay as they are).
 *
 * The colour image of a view reaches the colour decoder only through decode_color on the surface points of its valid pixels
 * (core/sdfrenderer/renderer_rgb.py:30-33; Zdepth is detached, has_zdepth_grad=False), and with lights the colour is multiplied by the
 * pixel's shading term s (renderer_rgb.py:121-124). So for any loss on the colour image and every parameter theta_c of the colour decoder
 *     dL/dtheta_c = sum over the valid pixels of view v of (g_rgb[pixel] * s[pixel]) . d rgb(x; theta_c) / d theta_c
 * -- the list and the upstream that give distr_color_stage_backward_batch its g_latent_cat. The call below hands both to the caller, who
 * runs the layer-wise train path (distr_train.h, a described net with out_dim = 3) on them for the weight gradients. No decoder
 * arithmetic here. The SDF decoder's weights get nothing from the colour image: the points are constants of the colour stage.
 */
#ifndef DISTR_COLOR_TRAIN_H_
#define DISTR_COLOR_TRAIN_H_

#include "distr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Valid on the forward and backward workspaces as distr_color_stage_backward_batch of the SAME cfg and nviews left them, when that call
 * had a non-NULL g_latent_cat (otherwise the upstream was never written); reads both, changes neither. P = H * W; N_v = the valid pixels
 * of view v. For view v and list position r < N_v (the valid pixels in row-major order):
 *   xyz_out[v][r][0..2]  the surface point as the forward built it, x = M^T (c + d z);
 *   up_out[v][r][0..2]   the upstream of the decoder's output at that point: g_rgb of the pixel, times s as ONE f32 product with lights;
 *   index_out[v][r]      the pixel (may be NULL);
 *   counts_dev[v] = N_v.
 * Rows at or beyond N_v are not written. cap >= P is the row stride of the three arrays. One kernel, grid (ceil(P / 256), nviews), plain
 * vector stores, no atomics, no host read: the same bytes on every run, and every view's rows are those of its own nviews = 1 call.
 * DISTR_ERR_INVALID_ARG: null pointers, nviews outside 1..DISTR_MAX_VIEWS, cap < P; DISTR_ERR_WORKSPACE: a workspace smaller than
 * distr_color_stage_workspace_bytes names; DISTR_ERR_UNSUPPORTED: row bands, as the stage refuses them. The checks are host code. */
int distr_color_stage_samples_export_batch(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, const void* ws_fwd_dev,
                                           size_t ws_fwd_bytes, const void* ws_bwd_dev, size_t ws_bwd_bytes, float* xyz_out, float* up_out,
                                           int32_t* index_out, int64_t cap, int32_t* counts_dev, void* stream);

/* ---- The photometric loss of nviews colour images (P = H * W pixels each, at most 2^24): the masked L1 and the SSIM term of the reference's
 * compute_loss_color(use_ssim=True) (core/utils/loss_utils.py:188-209, core/utils/pytorch_ssim/ssim.py:4-35), forward and backward, in one
 * launch sequence. rgb_dev[v][P][3], gt_dev[v][P][3], mask_dev[v][P], gt_mask_dev[v][P] (uint8, nonzero = valid).
 *   overlap = mask & gt_mask, N_v its pixels; l1_out[v] = mean |rgb - gt| over the overlap's 3 N_v entries; for SSIM both images are zeroed
 *   off the overlap, the five 3 x 3 zero-padded box means are always divided by 9, C1 = 0.01^2, C2 = 0.03^2, ssim = n / (d + 1e-12), and
 *   ssim_out[v] = the mean over 3 H W of clamp((1 - ssim) / 2, 0, 1) (written when want_ssim != 0); overlap_out[v] = N_v (int32).
 *   A view with an empty overlap gives l1 = 0 and a zero L1 gradient (the reference yields NaN or raises there): overlap_out shows it.
 * Backward: g_l1[v], g_ssim[v] (either may be NULL: that term carries no gradient) and overlap_dev = the forward's overlap_out ->
 * g_rgb_out[v][P][3], zero off the overlap; gt and the masks are observations. Two passes (the per-pixel partials of ssim with respect to
 * mu_y, E[y^2], E[xy]; their 3 x 3 gather plus the L1 sign term). No float atomics, fixed summation orders: the same bytes on every run,
 * and every view's values are those of its own nviews = 1 call.
 * distr_color_loss_workspace_bytes(H, W, nviews, backward): the bytes of the forward (backward == 0) or backward workspace; 0 for sizes
 * the calls refuse. DISTR_ERR_INVALID_ARG: null pointers, sizes, nviews outside 1..DISTR_MAX_VIEWS; DISTR_ERR_WORKSPACE: a null or short
 * workspace. The checks are host code. */
size_t distr_color_loss_workspace_bytes(int32_t H, int32_t W, int32_t nviews, int32_t backward);
int distr_color_loss_forward_batch(distr_ctx* ctx, int32_t H, int32_t W, int32_t nviews, const float* rgb_dev, const uint8_t* mask_dev,
                                   const float* gt_dev, const uint8_t* gt_mask_dev, int32_t want_ssim, float* l1_out, float* ssim_out,
                                   int32_t* overlap_out, void* ws_dev, size_t ws_bytes, void* stream);
int distr_color_loss_backward_batch(distr_ctx* ctx, int32_t H, int32_t W, int32_t nviews, const float* rgb_dev, const uint8_t* mask_dev,
                                    const float* gt_dev, const uint8_t* gt_mask_dev, const int32_t* overlap_dev, const float* g_l1,
                                    const float* g_ssim, float* g_rgb_out, void* ws_dev, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DISTR_COLOR_TRAIN_H_ */
