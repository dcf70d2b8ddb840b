/*
 * distr_multi.h -- C ABI of libdistr.so, part 4: the decoder on a SEGMENTED point list -- many shape codes in one launch sequence.
 * Included by distr.h. distr_mlp_eval / distr_mlp_grad / distr_mlp_backward (distr.h) take one shape code per call; a fit of S shapes
 * to SDF samples, or a batch of views with a code each, would issue S launch sequences of a few thousand points, each filling a
 * fraction of the chip. The calls below take the S point lists back to back instead.
 *
 * Segments. nseg (1..DISTR_MAX_VIEWS) segments lie one after the other in xyz_dev; segment s has counts_host[s] >= 0 points
 * (counts_host is a HOST array, as for distr_depth_samples_*; at most 2^30 points in all) and the shape code at
 * latent_dev + s * latent_stride (latent_stride 0: one code for all segments, else >= the code length). Outputs use the same order.
 *
 * What is identical to what. Every segment runs on 64-point tiles of its own (no tile holds points of two segments), so its slice
 * of every output is byte for byte what the single-code call gives for that segment alone. g_latent_dev (may be NULL) is
 * [nseg][code length]: row s = the sum over segment s's points, in the tile order of its stand-alone call; zeros for an empty
 * segment. With a shared code the caller adds the rows up, as for distr_render_backward_batch. No float atomics: the same bytes on
 * every run. f32 arithmetic only.
 *
 * Same conventions as distr.h. Refused: nseg outside 1..DISTR_MAX_VIEWS, a negative count, a null pointer, a latent_stride between 1
 * and the code length - 1 (DISTR_ERR_INVALID_ARG); a workspace that is too small (DISTR_ERR_WORKSPACE); no decoder
 * (DISTR_ERR_NO_DECODER); more than 2^30 points (DISTR_ERR_UNSUPPORTED). The *_workspace_bytes functions return 0 for an nseg or
 * counts that the calls refuse; distr_mlp_grad_multi takes the size of distr_mlp_multi_workspace_bytes.
 */
#ifndef DISTR_MULTI_H_
#define DISTR_MULTI_H_

#include "distr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* workspace of distr_mlp_eval_multi / distr_mlp_grad_multi, and of distr_mlp_backward_multi */
size_t distr_mlp_multi_workspace_bytes(int32_t nseg, const int64_t* counts_host);
size_t distr_mlp_backward_multi_workspace_bytes(int32_t nseg, const int64_t* counts_host);
/* decode_sdf: sdf_dev[sum counts]; clamp_dist < 0 = no clamp */
int distr_mlp_eval_multi(distr_ctx* ctx, int32_t nseg, const int64_t* counts_host, const float* latent_dev, int64_t latent_stride,
                         const float* xyz_dev, float clamp_dist, float* sdf_dev, void* ws_dev, size_t ws_bytes, void* stream);
/* the unclamped decoder and d f / d xyz per point: sdf_dev[sum counts], grad_dev[sum counts][3] */
int distr_mlp_grad_multi(distr_ctx* ctx, int32_t nseg, const int64_t* counts_host, const float* latent_dev, int64_t latent_stride,
                         const float* xyz_dev, float* sdf_dev, float* grad_dev, void* ws_dev, size_t ws_bytes, void* stream);
/* backward of distr_mlp_eval_multi: g_sdf[sum counts] -> g_xyz[sum counts][3] (may be NULL), g_latent[nseg][code length] (may be NULL);
 * clamp >= 0: zero gradient where |f| > clamp */
int distr_mlp_backward_multi(distr_ctx* ctx, int32_t nseg, const int64_t* counts_host, const float* latent_dev, int64_t latent_stride,
                             const float* xyz_dev, const float* g_sdf, float clamp, float* g_xyz, float* g_latent, void* ws_dev,
                             size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DISTR_MULTI_H_ */
