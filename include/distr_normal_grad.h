/*
 * distr_normal_grad.h -- C ABI of libdistr.so, part 5: the decoder-path term of the autograd normals' backward. Included by distr.h; new
 * functions only (DISTR_ABI_VERSION and every struct stay as they are).
 *
 * The reference's render_normal differentiates the decoder with create_graph=True (core/utils/decoder_utils.py:76-92,
 * core/sdfrenderer/renderer.py:880-910), so a loss on the autograd normals reaches the shape code and the camera through the decoder a
 * second time. distr_render_backward keeps the gradient of `R @ normal` with respect to R (renderer.py:978) and omits that term; the call
 * below computes it, exactly, for callers that want it (raw normals: normalize_normal = 0; with unit normals the term is zero by scale
 * invariance). For a ReLU decoder the second-order path collapses to one upstream scalar on the decoder's value f at every surface sample,
 *     g_f = -2 f (g . h) / (1 - f^2),   h = the pixel's raw normal, g = dL/dh (g_normal pulled back through the x flip, R and M_normal),
 * zero where |f| > clamp_dist, followed by the first-order decoder backward at the surface point M^T (cam_pos + ray * Zdepth) with Zdepth
 * detached (has_zdepth_grad=False, renderer.py:895).
 *
 * Additive: the call works on the saved forward workspace of the SAME cfg and inputs (before or after distr_render_backward_batch, which
 * it neither calls nor changes), writes outputs of its own, and the caller adds them to those of distr_render_backward_batch.
 * Per view and deterministic: one compaction of the valid pixels by a scan in a fixed order, one segmented point-list backward with a
 * segment per view, camera sums in a fixed order, no float atomics, no host read -- every view's outputs are byte for byte those of its
 * own nviews = 1 call, and the same on every run.
 *
 * view_flags (HOST array [nviews] of DISTR_VIEW_GRAD_*, or NULL = cfg's) is checked like distr_render_forward_batch checks it and changes
 * nothing: render() hands no_grad_camera to render_depth only (renderer.py:964); render_normal rebuilds the camera position and the rays
 * from R and T with their gradients (renderer.py:881-882, 977), so a view rendered with no_grad_camera gets this term's g_R and g_T like
 * any other view.
 *
 * Refused, with text in distr_last_error: use_depth2normal (no such term), want_normal = 0, save_for_backward = 0 (DISTR_ERR_INVALID_ARG);
 * a row band (rows != 0), arith != DISTR_ARITH_F32, more than 2^30 pixels in all views (DISTR_ERR_UNSUPPORTED). With normalize_normal != 0
 * the outputs are set to zero and no decoder work is launched.
 */
#ifndef DISTR_NORMAL_GRAD_H_
#define DISTR_NORMAL_GRAD_H_

#include "distr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of `ws_dev` of distr_render_normal_grad_backward_batch for nviews views of cfg (the same refusals) */
int distr_render_normal_grad_workspace_bytes(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, size_t* bytes);

/* ws_fwd_dev: the nviews x forward_bytes workspace the forward of the same cfg and inputs left (read only);
 * g_normal_dev[nviews][H*W][3]: upstream gradient of the normal images; outputs (any may be NULL): g_latent_dev[nviews][code length],
 * g_R_dev[nviews][9], g_T_dev[nviews][3]; a view without a valid pixel gets zeros. nviews == 1 is the single-view form. */
int distr_render_normal_grad_backward_batch(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, const int32_t* view_flags,
                                            const void* ws_fwd_dev, size_t ws_fwd_bytes, const float* g_normal_dev, float* g_latent_dev,
                                            float* g_R_dev, float* g_T_dev, void* ws_dev, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DISTR_NORMAL_GRAD_H_ */
