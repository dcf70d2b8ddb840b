/*
 * distr_live_order.h -- C ABI of libdistr.so, part 8: the ordered live list of the full-resolution march, seen from outside. Included by
 * distr.h; new functions only (DISTR_ABI_VERSION and every struct stay as they are). Statistics and test read-backs: nothing here changes a
 * render.
 *
 * The setup kernels enumerate the pixels of an image (of every pyramid level's grid, of a row band) in blocks: a workgroup of 256 threads
 * covers a 16 x 16 pixel block, each of its four wavefronts one 8 x 8 sub-block, row-major inside. The blocks tile the grid row-major;
 * distr_block_grid gives their number, distr_block_pixel the pixel of one thread.
 *
 * A step of the recursive marchers whose 64-ray role has work keeps its live list in the order of the list it read (DISTR_LIVE_ORDER, default
 * 1). distr_debug_live_list reads the list a step left behind; distr_get_kstep_stats what the compacted 64-ray tiles
 * executed.
 */
#ifndef DISTR_LIVE_ORDER_H_
#define DISTR_LIVE_ORDER_H_

#include "distr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* number of 16 x 16 blocks that cover a grid of w x h pixels (w, h >= 1); 0 for an empty grid */
int32_t distr_block_grid(int32_t w, int32_t h);

/* pixel (row-major index y * w + x) of thread `thread` (0..255) of block `block` (0 .. distr_block_grid - 1), or -1: the thread's
 * position lies outside the grid ("no ray"), or an argument is out of range */
int32_t distr_block_pixel(int32_t w, int32_t h, int32_t block, int32_t thread);

/* k-steps of the compacted 64-ray forward tiles of the forward that used `ws_dev`, per march launch in launch order (the coarse levels'
 * steps, coarsest level first, then the full-resolution steps -- the order of distr_get_live_counts). out[3 i + 0] = tiles, out[3 i + 1] =
 * k-steps executed, out[3 i + 2] = k-steps of as many dense tiles; a launch without compacted tiles reports zeros. A k-step = 16 rows of a
 * layer's k-loop, weighted by the layer's output blocks per wave (768 per dense tile). *n = launches; at most `cap` of them are written. */
int distr_get_kstep_stats(distr_ctx* ctx, const distr_render_cfg* cfg, const void* ws_dev, int64_t* out, int32_t cap, int32_t* n, void* stream);

/* the same three figures for the 32-ray tiles of the step kernel's 32-ray role (exact f32), per FULL-RESOLUTION step only (out[3 t + ..],
 * t = 0 .. fine steps - 1; *n = fine steps): a compacted tile (DISTR_COMPACT32, default 1, on top of DISTR_DENSE_COMPACT) adds the k-steps
 * it executed, a dense one 768. These tiles are not part of distr_get_kstep_stats. */
int distr_get_kstep32_stats(distr_ctx* ctx, const distr_render_cfg* cfg, const void* ws_dev, int64_t* out, int32_t cap, int32_t* n, void* stream);

/* test aids: the 32-point tile as the step kernel's 32-ray role runs it (compacted or dense by the two knobs, read at distr_create), on a
 * point list of 32-point tiles -- distr_debug_mlp_layer / distr_debug_tile_timing (distr.h) for the 32-ray tile, same arguments and outputs
 * (ts_dev[ceil(n / 32)][40]). */
int distr_debug_mlp_layer32(distr_ctx* ctx, const float* latent_dev, const float* xyz_dev, int64_t n, int layer, float* out_dev, void* ws_dev,
                            size_t ws_bytes, void* stream);
int distr_debug_tile_timing32(distr_ctx* ctx, const float* latent_dev, const float* xyz_dev, int64_t n, float* sdf_dev, long long* ts_dev,
                              void* ws_dev, size_t ws_bytes, void* stream);

/* test only: the live list full-resolution step `step` (0 .. fine steps - 2) read and the one it left for step + 1. Renders ONE view of
 * cfg up to and including that step into `ws_dev` (a forward workspace; no outputs are written), then copies both lists to the HOST arrays
 * read[cap] / left[cap] and their lengths to *nread / *nleft (entries = pixel indices). *ordered = 1 when the step kept the list in order,
 * 0 when it appended atomically. */
int distr_debug_live_list(distr_ctx* ctx, const distr_render_cfg* cfg, const float* latent_dev, const float* R_dev, const float* T_dev,
                          int32_t step, int32_t* read, int32_t* left, int32_t cap, int32_t* nread, int32_t* nleft, int32_t* ordered,
                          void* ws_dev, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DISTR_LIVE_ORDER_H_ */
