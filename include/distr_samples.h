/*
 * distr_samples.h -- C ABI of libdistr.so, part 3: an observed depth (and normal) map back-projected into SDF samples of the decoder,
 * the supervision terms of a DeepSDF-style fit to depth scans. Included by distr.h; the reference's counterpart is
 * SDFRenderer_deepsdf (core/sdfrenderer/renderer_deepsdf.py:10-64): get_samples (:14-43) and get_freespace_samples (:45-64).
 *
 * Same conventions as distr.h: caller-owned device buffers and workspaces, everything enqueued on `stream`, DISTR_OK or a negative
 * code with text in distr_last_error. Only distr_depth_samples_count synchronises the stream: it returns the number of valid pixels
 * of every view so that the caller can allocate the lists (the reference's boolean indexing synchronises at the same place).
 *
 * Views and lists. A call takes nviews (1..DISTR_MAX_VIEWS) views of one image size: RT_dev[v] (3, 4) row-major = [R | T],
 * depth_dev[v][H*W], normal_dev[v][H*W][3]. Valid pixels are 0 < depth < 1e5; view v has N_v of them, taken in row-major pixel
 * order, and Npre_v = N_0 + ... + N_(v-1) before it. With m = 2 (DISTR_SAMPLES_SURFACE) or m = cfg->number
 * (DISTR_SAMPLES_FREESPACE) list entries per valid pixel, view v owns the m * N_v consecutive entries from m * Npre_v on, laid out
 * [k][i]: k = 0 (p + offset) / 1 (p - offset), or the draw; i = the view's valid pixel. L = m * (N_0 + ... + N_(nviews-1)).
 *   SURFACE    p = M^T (cam_pos + ray * zdepth), zdepth = depth / calib_map, offset = M^T n * eta_i;
 *              out = f(p + offset) - eta_i | f(p - offset) + eta_i;    draws_dev = eta_map: N_v floats per view, at Npre_v
 *   FREESPACE  p_k = M^T (cam_pos + ray * zdepth * ratio_k,i);  out = f(p_k);
 *              draws_dev = ratio: [number][N_v] floats per view, at number * Npre_v
 * f = the decoder clamped to +-clamp_dist. The library draws no random numbers: the caller supplies them.
 *
 * Determinism: list positions come from a scan in a fixed order, the camera gradient from sums in a fixed order, nothing from an
 * atomic: the same bytes on every run, and every view's slice of every output (gradients included) is byte for byte what a
 * stand-alone call of that view gives.
 */
#ifndef DISTR_SAMPLES_H_
#define DISTR_SAMPLES_H_

#include "distr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DISTR_SAMPLES_SURFACE 0   /* get_samples            renderer_deepsdf.py:14-43 */
#define DISTR_SAMPLES_FREESPACE 1 /* get_freespace_samples  renderer_deepsdf.py:45-64 */
#define DISTR_SAMPLES_MAX_NUMBER 64

typedef struct distr_samples_cfg {
  uint32_t struct_size; /* sizeof(distr_samples_cfg) */
  int32_t H, W;         /* img_hw */
  float K_inv[9];       /* float32(inv(K)), row-major */
  float M[9];           /* transform_matrix (3x3); the points and the normals are multiplied by its transpose */
  float clamp_dist;     /* decoder outputs are clamped to +-clamp_dist; < 0: no clamp */
  int32_t mode;         /* DISTR_SAMPLES_* */
  int32_t number;       /* FREESPACE: draws per valid pixel (1..DISTR_SAMPLES_MAX_NUMBER); SURFACE: ignored */
} distr_samples_cfg;

/* Bytes of count_bytes (distr_depth_samples_count), and -- given the counts that call returned (HOST array [nviews]; NULL: only
 * count_bytes is written) -- of the forward and backward workspaces. Any of the three outputs may be NULL. */
int distr_depth_samples_workspace_bytes(distr_ctx* ctx, const distr_samples_cfg* cfg, int32_t nviews, const int64_t* counts,
                                        size_t* count_bytes, size_t* forward_bytes, size_t* backward_bytes);

/* Compacts the valid pixels: index_dev[v][0 .. N_v) (int32, capacity [nviews][H*W]) = the valid pixels of view v in row-major order,
 * counts[v] (HOST) = N_v. Synchronises `stream`. index_dev is what forward and backward read: keep it untouched. */
int distr_depth_samples_count(distr_ctx* ctx, const distr_samples_cfg* cfg, int32_t nviews, const float* depth_dev, int32_t* index_dev,
                              int64_t* counts, void* ws_dev, size_t ws_bytes, void* stream);

/* Point list, ONE decoder evaluation over the whole list, epilogue. With a code per view the evaluation is the segmented one of
 * distr_multi.h, a segment per view: still one launch sequence, every view's slice byte for byte its own call.
 *   latent_dev + v * latent_stride (floats; 0 = one code shared by all views)
 *   normal_dev   SURFACE only (FREESPACE: may be NULL)
 *   xyz_dev[L][3]  the point list in the decoder's frame (output; the backward reads it)
 *   out_dev[L]     the samples */
int distr_depth_samples_forward(distr_ctx* ctx, const distr_samples_cfg* cfg, int32_t nviews, const int64_t* counts,
                                const int32_t* index_dev, const float* latent_dev, int64_t latent_stride, const float* RT_dev,
                                const float* depth_dev, const float* normal_dev, const float* draws_dev, float* xyz_dev, float* out_dev,
                                void* ws_dev, size_t ws_bytes, void* stream);

/* g_out_dev[L] (upstream gradient of out_dev) -> g_latent_dev[nviews][C] (per view: a shared code's gradient is the sum over v, left
 * to the caller) and g_RT_dev[nviews][3][4]; either may be NULL. depth and normal are observations: no gradient. index_dev, xyz_dev
 * and all inputs as in the forward. The decoder's backward is one segmented launch sequence too (distr_mlp_backward_multi's), for a
 * shared code and a code per view alike. */
int distr_depth_samples_backward(distr_ctx* ctx, const distr_samples_cfg* cfg, int32_t nviews, const int64_t* counts,
                                 const int32_t* index_dev, const float* latent_dev, int64_t latent_stride, const float* RT_dev,
                                 const float* depth_dev, const float* draws_dev, const float* xyz_dev, const float* g_out_dev,
                                 float* g_latent_dev, float* g_RT_dev, void* ws_dev, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DISTR_SAMPLES_H_ */
