/*
 * distr_render_train.h -- C ABI of libdistr.so, part 9: the render backward's gradient-sample list, written out. Included by distr.h; new
 * functions only (DISTR_ABI_VERSION and every struct stay as they are).
 *
 * distr_render_backward_batch turns the upstream gradients of a render into a list of gradient-carrying samples per view: the selected
 * rows of every ray (get_min_sdf_sample, get_sample_on_marching_zdepth_along_ray: core/sdfrenderer/renderer.py:386, 415), each with the
 * scalar `coef` = dL/df that reaches the decoder's value f at the sample's point, and behind them one combined pad sample at the origin
 * when padded rows carry a coefficient. Every march evaluation of the reference is detached (renderer.py:488, 547), so for any loss on
 * zdepth, depth, min_sdf and depth2normal normals
 *     dL/dtheta = sum over the list of coef * d f(x; theta) / d theta
 * for every parameter theta of the decoder: the shape code (distr_render_backward's g_latent) and the weights alike. The call below hands
 * the list to the caller, who runs the layer-wise train path (distr_train.h) on it for the weight gradients. No decoder arithmetic here.
 *
 * Valid on the forward and backward workspaces as distr_render_backward_batch of the SAME cfg and nviews left them; reads both, changes
 * neither. One kernel, grid (ceil(distr_render_max_samples / 256), nviews), plain vector stores, no atomics, no host read: the same
 * bytes on every run, and every view's rows are those of its own nviews = 1 call.
 */
#ifndef DISTR_RENDER_TRAIN_H_
#define DISTR_RENDER_TRAIN_H_

#include "distr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows a view's list can hold: P * buffer_size + 1 (P = pixels of the rendered band); 0 for a cfg the render calls refuse */
int64_t distr_render_max_samples(const distr_render_cfg* cfg);

/* For view v and list position r < count_v: xyz_dev[v][r][0..2] = the sample's point exactly as the backward kernel builds it (pixel or
 * coarse-ray centre -> ray -> camera position + ray * z, through M; the origin for the pad sample), coef_dev[v][r] = its coefficient,
 * src_dev[v][r] (may be NULL) = its encoded source: the pixel for a full-resolution row, level << 28 | step << 24 | ray for a coarse
 * row, -1 for the pad sample. counts_dev[v] = count_v. Rows at or beyond count_v are not written. cap >= distr_render_max_samples(cfg)
 * is the row stride of the three arrays.
 * DISTR_ERR_INVALID_ARG: null pointers, save_for_backward == 0, nviews outside 1..DISTR_MAX_VIEWS, cap too small;
 * DISTR_ERR_WORKSPACE: a workspace smaller than nviews x the size distr_workspace_bytes names. */
int distr_render_samples_export_batch(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, const void* ws_fwd_dev,
                                      size_t ws_fwd_bytes, const void* ws_bwd_dev, size_t ws_bwd_bytes, float* xyz_dev, float* coef_dev,
                                      int32_t* src_dev, int64_t cap, int32_t* counts_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DISTR_RENDER_TRAIN_H_ */
