/*
 * distr_color_batch.h -- C ABI of libdistr.so, part 6: the colour decoder on a SEGMENTED point list, and the colour stage of a batch of
 * rendered views (SDFRenderer_color.render_color + compute_shading_maps, core/sdfrenderer/renderer_rgb.py:20-67, for up to
 * DISTR_MAX_VIEWS views in one launch sequence). Included by distr.h. Same conventions as distr.h: caller-owned device buffers,
 * everything enqueued on `stream`, no allocation, no host read, no float atomics -- the same bytes on every run.
 *
 * ---- 1. distr_color_eval / distr_color_backward on a segmented list: the colour counterpart of distr_multi.h.
 * nseg (1..DISTR_MAX_VIEWS) segments lie one after the other in xyz_dev; segment s has counts_host[s] >= 0 points (HOST array) and the
 * [shape code | colour code] at latent_cat_dev + s * latent_stride (floats; 0: one code for all segments, else >= 256 + color_size).
 * Every segment runs on 64-point tiles of its own, so its slice of rgb / g_xyz is byte for byte what distr_color_eval /
 * distr_color_backward give for that segment alone; g_latent_cat (may be NULL) is [nseg][256 + color_size]: row s = the sum over segment
 * s's tiles in tile order, zeros for an empty segment (a shared code's rows are added by the caller). Refusals as in distr_multi.h.
 */
#ifndef DISTR_COLOR_BATCH_H_
#define DISTR_COLOR_BATCH_H_

#include "distr.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t distr_color_multi_workspace_bytes(int32_t nseg, const int64_t* counts_host);
size_t distr_color_backward_multi_workspace_bytes(int32_t nseg, const int64_t* counts_host);
/* rgb_dev[sum counts][3] */
int distr_color_eval_multi(distr_ctx* ctx, int32_t nseg, const int64_t* counts_host, const float* latent_cat_dev, int64_t latent_stride,
                           const float* xyz_dev, float* rgb_dev, void* ws_dev, size_t ws_bytes, void* stream);
/* g_rgb[sum counts][3] -> g_xyz[sum counts][3] (may be NULL), g_latent_cat[nseg][256 + color_size] (may be NULL) */
int distr_color_backward_multi(distr_ctx* ctx, int32_t nseg, const int64_t* counts_host, const float* latent_cat_dev, int64_t latent_stride,
                               const float* xyz_dev, const float* g_rgb, float* g_xyz, float* g_latent_cat, void* ws_dev, size_t ws_bytes,
                               void* stream);

/* ---- 2. The colour stage of nviews rendered views (P = H * W pixels each; cfg gives H, W, K_inv and the point transform M, nothing
 * else of it is read; row bands are refused). Inputs are what distr_render_forward_batch wrote, as plain buffers:
 *   R_dev[v][9], T_dev[v][3], zdepth_dev[v][P], mask_dev[v][P] (uint8), normal_dev[v][P][3] (the transformed normal image; read only
 *   when lights are given), latent_cat_dev + v * latent_stride (0: shared).
 * Forward: the valid pixels of every view are compacted in row-major order by a fixed-order scan (the counts stay on the device); a
 * thread per valid pixel recomputes its ray and forms x = M^T (c + d z); ONE segmented colour evaluation (segment v = the N_v points
 * from point v * P on, tiles of its own); one kernel per pixel writes rgb_dev[v][P][3], zero off the mask. With lights the colour is
 * multiplied by  s = sum_m e_m ((R l_m) . n),  l_m = (L_m - q) / |L_m - q|,  q = c + d z (WITHOUT M^T, renderer_rgb.py:54), n = the
 * normal image's pixel. Every view's bytes are those of its own nviews = 1 call.
 *   ws_dev: forward_bytes of distr_color_stage_workspace_bytes; it keeps the index, the points and the unshaded colours for the
 *   backward and must stay untouched until that has run.
 *   index_out[v][P] (int32: the first N_v entries of row v), xyz_out[nviews * P][3] (view v from point v * P on), totals_out[nviews]
 *   (int32, N_v): optional copies for inspection, each may be NULL.
 * Backward: g_rgb[v][P][3] -> g_latent_cat[v][256 + color_size] (a row per view also for a shared code; NULL: the colours are treated
 * as constants and only the shading terms are returned), g_R[v][9], g_T[v][3], g_normal[v][P][3] (written only with lights; zero off
 * the mask); any output may be NULL. The decoder backward is one segmented launch with upstream g_rgb * s; its point gradients go back
 * through M^T, q = d z + c, the ray normalisation and c = -R^T T, and the shading's own terms (g_s = sum_c g_rgb_c colour_c: g_n, the
 * explicit R of R l_m, g_q through the normalisation of L_m - q) join the same per-pixel g_q and the same ordered sums (per thread a
 * serial run, an LDS tree, block partials in block order). zdepth carries no gradient; lights and energies are observations. */
typedef struct distr_color_lights {
  uint32_t struct_size;          /* sizeof(distr_color_lights) */
  int32_t nlights;               /* M >= 0 per view; 0: no shading, the other fields are not read */
  const float* locations_dev;    /* [nviews or 1][M][3] */
  int64_t location_stride;       /* floats between two views' light sets; 0: one set shared by all views */
  const float* energies_dev;     /* [nviews or 1][M] */
  int64_t energy_stride;         /* floats between two views' energies; 0: shared */
} distr_color_lights;

int distr_color_stage_workspace_bytes(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, size_t* forward_bytes,
                                      size_t* backward_bytes);
int distr_color_stage_forward_batch(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, const float* R_dev, const float* T_dev,
                                    const float* zdepth_dev, const uint8_t* mask_dev, const float* normal_dev,
                                    const float* latent_cat_dev, int64_t latent_stride, const distr_color_lights* lights,
                                    float* rgb_dev, void* ws_dev, size_t ws_bytes, int32_t* index_out, float* xyz_out,
                                    int32_t* totals_out, void* stream);
int distr_color_stage_backward_batch(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, const float* R_dev, const float* T_dev,
                                     const float* zdepth_dev, const float* normal_dev, const float* latent_cat_dev,
                                     int64_t latent_stride, const distr_color_lights* lights, const void* ws_fwd_dev,
                                     size_t ws_fwd_bytes, const float* g_rgb, float* g_latent_cat, float* g_R, float* g_T,
                                     float* g_normal, void* ws_bwd_dev, size_t ws_bwd_bytes, void* stream);

/* Relighting without re-marching: nframes light sets on ONE rendered view. color_dev[P][3] = the unshaded colour image, the other
 * inputs as above for one view; lights: [nframes or 1][M][3] / [nframes or 1][M] with the strides counting frames; out_dev[f][P][3] =
 * color * s_f, byte for byte the lit distr_color_stage_forward_batch of that view with frame f's lights. Forward only. */
int distr_color_relight(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nframes, const float* R_dev, const float* T_dev,
                        const float* zdepth_dev, const uint8_t* mask_dev, const float* normal_dev, const float* color_dev,
                        const distr_color_lights* lights, float* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DISTR_COLOR_BATCH_H_ */
