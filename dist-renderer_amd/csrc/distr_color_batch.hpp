// distr_color_batch.hpp -- the colour stage of a batch of rendered views (include/distr_color_batch.h; reference: render_color and
// compute_shading_maps, core/sdfrenderer/renderer_rgb.py:20-67, which run once per view): the kernels around ONE segmented evaluation
// of the colour decoder (k_color / k_color_bwd with a tile table, distr_kernels.hpp).
//
//   forward
//   1 k_cb_count      per view, per block of MTILE pixels: number of valid pixels (the render's final mask, a plain u8 image)
//   2 k_samp_top_scan (distr_samples.hpp) per view: exclusive scan of the block counts, the view's total N_v behind them
//   3 k_cb_compact    the valid pixels of view v in row-major order -> index[v][0 .. N_v); pos[v][pixel] = its list position, -1 off the mask
//   4 k_cb_points     per valid pixel: the ray again (make_ray), x = M^T (c + d z) -> xyz[v * P + i]
//   5 k_ng_seg_table  (distr_normal_grad.hpp) the tile table from the DEVICE counts: segment v = N_v points at v * P
//     (k_latent_consts on the colour decoder, k_color over nviews * ceil(P / 64) tiles: a tile behind the last segment leaves at seg_find)
//   6 k_cb_epilogue   per pixel: rgb = colour of its list entry (times the shading term s when lights are given), zero off the mask;
//                     grid.y = view. The relighting call runs the same kernel body with grid.y = frame on one view's colour IMAGE.
//   backward
//   7 k_cb_bwd_pre    per pixel: upstream of the decoder g_rgb * s -> g_col[list entry]; g_normal = g_s sum_m e_m R l_m (zero off the mask)
//     (k_latent_consts, k_ng_seg_table, k_color_bwd, k_points_latent_grad)
//   8 k_cb_cam_bwd    per valid pixel: g_q = M g_x + the shading's g_q; g_d = z g_q, g_c = g_q; the explicit R of R l_m; 12 sums per block
//   9 k_cb_cam_fin    per view: the block sums in block order, then c = -R^T T: g_R = ray part - T (x) g_c, g_T = -R g_c
//   after the backward, on request (weight gradients of the colour decoder)
//  10 k_cb_export     per valid pixel: its point, its upstream g_col and its pixel, out of the two workspaces into the caller's arrays
//
// Shading term of a pixel (renderer_rgb.py:54-62, 122-123): q = c + d z (no M^T), u_m = L_m - q, l_m = u_m / |u_m|,
//   s = sum_m e_m ((R l_m) . n),  n = the transformed normal image's pixel.  With g_s = sum_c g_rgb_c colour_c:
//   g_n = g_s sum_m e_m R l_m;   g_R[j][i] += g_s sum_m e_m n_j l_m,i;   g_l_m = g_s e_m R^T n;   g_q = -sum_m (g_l_m - l_m (l_m . g_l_m)) / |u_m|.
//
// No atomics and no host read: list positions come from a scan in a fixed order, sums from fixed trees (thread-serial run -> LDS tree ->
// block order). Every kernel indexes (block, view): a view's blocks, tiles and trees are those of its own call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "distr_kernels.hpp"    // make_ray, make_point, ray_backward_acc
#include "distr_samples.hpp"    // MB / MPER / MTILE, Cam12, block_sum12, k_samp_top_scan

namespace distr {
namespace cbatch {

using samples::MB;
using samples::MPER;
using samples::MTILE;
using samples::Cam12;

struct Geo {                 // per call
  int H, W, P;               // P = H * W
  float Ki[9], M[9];
};

struct Cams {                // per view: R[v][9], T[v][3], zdepth[v][P], normal[v][P][3] (null without lights)
  const float* R;
  const float* T;
  const float* zdepth;
  const float* normal;
  int64_t vstride;           // pixels between two views' images: P for a batch of views, 0 for the frames of one view (relight)
};

struct Lights {              // M lights per view (or frame): loc[v * lstride + 3 m], en[v * estride + m]; strides 0: shared
  const float* loc;
  const float* en;
  int64_t lstride, estride;
  int M;
};

DISTR_GLOBAL void __launch_bounds__(MB) k_cb_count(const uint8_t* __restrict__ mask, int P, int nb, int* __restrict__ btot) {
  __shared__ int lds[MB];
  const int v = blockIdx.y;
  const uint8_t* m = mask + (size_t)v * P;
  const int base = blockIdx.x * MTILE + threadIdx.x * MPER;
  int s = 0;
  for (int q = 0; q < MPER && base + q < P; ++q) s += m[base + q] ? 1 : 0;
  int tot;
  mesh::block_excl_scan(s, lds, &tot);
  if (threadIdx.x == 0) btot[(size_t)v * nb + blockIdx.x] = tot;
}

DISTR_GLOBAL void __launch_bounds__(MB) k_cb_compact(const uint8_t* __restrict__ mask, int P, int nb, const int* __restrict__ boff,
                                                     int32_t* __restrict__ index, int32_t* __restrict__ pos) {
  __shared__ int lds[MB];
  const int v = blockIdx.y;
  const uint8_t* m = mask + (size_t)v * P;
  const int base = blockIdx.x * MTILE + threadIdx.x * MPER;
  int s = 0;
  for (int q = 0; q < MPER && base + q < P; ++q) s += m[base + q] ? 1 : 0;
  int tot;
  int at = boff[(size_t)v * nb + blockIdx.x] + mesh::block_excl_scan(s, lds, &tot);
  int32_t* out = index + (size_t)v * P;      // at < the view's count <= P
  int32_t* po = pos + (size_t)v * P;
  for (int q = 0; q < MPER && base + q < P; ++q) {
    const bool on = m[base + q] != 0;
    po[base + q] = on ? at : -1;
    if (on) out[at++] = base + q;
  }
}

// an index entry outside the image (a forward workspace that is not this call's) reads pixel 0, never out of bounds
__device__ __forceinline__ int valid_pixel(const Geo& G, int pix) { return (unsigned)pix < (unsigned)G.P ? pix : 0; }

struct PixelGeo { RayGeo g; float c[3], q[3], z; };

// ray of pixel `pix`, camera position c = -R^T T (the order of k_prep), q = d z + c (the order of make_point)
__device__ __forceinline__ PixelGeo pixel_geo(const Geo& G, const float* __restrict__ R, const float* __restrict__ T, float z, int pix) {
  float Rr[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Rr[k] = R[k];
  PixelGeo pg;
  pg.g = make_ray(G.Ki, Rr, (float)(pix % G.W), (float)(pix / G.W));
#pragma unroll
  for (int i = 0; i < 3; ++i) pg.c[i] = -(Rr[0 * 3 + i] * T[0] + Rr[1 * 3 + i] * T[1] + Rr[2 * 3 + i] * T[2]);
  pg.z = z;
#pragma unroll
  for (int i = 0; i < 3; ++i) pg.q[i] = pg.g.d[i] * z + pg.c[i];
  return pg;
}

// grid (blocks of MB valid pixels, views)
DISTR_GLOBAL void __launch_bounds__(MB) k_cb_points(const Geo G, const Cams C, const int32_t* __restrict__ index, const int* __restrict__ totals,
                                                    float* __restrict__ xyz) {
  const int v = blockIdx.y;
  const int i = blockIdx.x * MB + threadIdx.x;
  if (i >= min(totals[v], G.P)) return;
  const size_t vo = (size_t)v * G.P;
  const int pix = valid_pixel(G, index[vo + i]);
  const PixelGeo pg = pixel_geo(G, C.R + 9 * v, C.T + 3 * v, C.zdepth[vo + pix], pix);
  float p[3];
  make_point(G.M, pg.c, pg.g.d, pg.z, p);
  float* x = xyz + 3 * (vo + i);
  x[0] = p[0]; x[1] = p[1]; x[2] = p[2];
}

// one light of one pixel: l = (L - q) / |L - q| and 1 / |L - q|
struct LightDir { float l[3], inv; };
__device__ __forceinline__ LightDir light_dir(const float* __restrict__ Lm, const float* q) {
  LightDir d;
  const float u[3] = {Lm[0] - q[0], Lm[1] - q[1], Lm[2] - q[2]};
  const float len = sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  d.inv = 1.0f / len;
#pragma unroll
  for (int k = 0; k < 3; ++k) d.l[k] = u[k] / len;
  return d;
}

// s = sum_m e_m ((R l_m) . n), the lights in their order
__device__ __forceinline__ float shading_term(const Lights& L, int64_t set, const float* __restrict__ R, const float* q, const float* n) {
  const float* loc = L.loc + set * L.lstride;
  const float* en = L.en + set * L.estride;
  float s = 0.f;
  for (int m = 0; m < L.M; ++m) {
    const LightDir d = light_dir(loc + 3 * m, q);
    float lam = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) lam += (R[j * 3 + 0] * d.l[0] + R[j * 3 + 1] * d.l[1] + R[j * 3 + 2] * d.l[2]) * n[j];
    s += en[m] * lam;
  }
  return s;
}

// grid (blocks of MB pixels, views or frames). LIST: col = the colour list of the segmented evaluation (entry v * P + pos); else the colour
// IMAGE of the one view (pixel). C.vstride = 0 keeps every frame on view 0's camera and images.
template <bool LIST>
DISTR_GLOBAL void __launch_bounds__(MB) k_cb_epilogue(const Geo G, const Cams C, const Lights L, const uint8_t* __restrict__ mask,
                                                      const int32_t* __restrict__ pos, const float* __restrict__ col, float* __restrict__ rgb) {
  const int f = blockIdx.y;
  const int pix = blockIdx.x * MB + threadIdx.x;
  if (pix >= G.P) return;
  const int v = C.vstride ? f : 0;
  const size_t vo = (size_t)v * G.P;
  float* o = rgb + 3 * ((size_t)f * G.P + pix);
  if (!mask[vo + pix]) { o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; return; }
  const float* c = col + 3 * (LIST ? vo + pos[vo + pix] : vo + pix);
  float s = 1.0f;
  if (L.M > 0) {
    const PixelGeo pg = pixel_geo(G, C.R + 9 * v, C.T + 3 * v, C.zdepth[vo + pix], pix);
    s = shading_term(L, f, C.R + 9 * v, pg.q, C.normal + 3 * (vo + pix));
  }
  if (L.M > 0) { o[0] = c[0] * s; o[1] = c[1] * s; o[2] = c[2] * s; }
  else { o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; }
}

// grid (blocks of MB pixels, views): g_col[list entry] = g_rgb * s (null: the colours are constants); g_normal (null without lights)
DISTR_GLOBAL void __launch_bounds__(MB) k_cb_bwd_pre(const Geo G, const Cams C, const Lights L, const int32_t* __restrict__ pos,
                                                     const float* __restrict__ col, const float* __restrict__ g_rgb, float* __restrict__ g_col,
                                                     float* __restrict__ g_normal) {
  const int v = blockIdx.y;
  const int pix = blockIdx.x * MB + threadIdx.x;
  if (pix >= G.P) return;
  const size_t vo = (size_t)v * G.P;
  const int at = pos[vo + pix];
  float* gn = g_normal ? g_normal + 3 * (vo + pix) : nullptr;
  if ((unsigned)at >= (unsigned)G.P) {      // off the mask (-1)
    if (gn) { gn[0] = 0.f; gn[1] = 0.f; gn[2] = 0.f; }
    return;
  }
  const float* g = g_rgb + 3 * (vo + pix);
  float s = 1.0f;
  if (L.M > 0) {
    const float* R = C.R + 9 * v;
    const PixelGeo pg = pixel_geo(G, R, C.T + 3 * v, C.zdepth[vo + pix], pix);
    s = shading_term(L, v, R, pg.q, C.normal + 3 * (vo + pix));
    if (gn) {
      const float* c = col + 3 * (vo + at);
      const float gs = g[0] * c[0] + g[1] * c[1] + g[2] * c[2];
      const float* loc = L.loc + (int64_t)v * L.lstride;
      const float* en = L.en + (int64_t)v * L.estride;
      float a[3] = {0.f, 0.f, 0.f};
      for (int m = 0; m < L.M; ++m) {
        const LightDir d = light_dir(loc + 3 * m, pg.q);
#pragma unroll
        for (int j = 0; j < 3; ++j) a[j] += en[m] * (R[j * 3 + 0] * d.l[0] + R[j * 3 + 1] * d.l[1] + R[j * 3 + 2] * d.l[2]);
      }
      gn[0] = gs * a[0]; gn[1] = gs * a[1]; gn[2] = gs * a[2];
    }
  }
  if (g_col) {
    float* o = g_col + 3 * (vo + at);
    if (L.M > 0) { o[0] = g[0] * s; o[1] = g[1] * s; o[2] = g[2] * s; }
    else { o[0] = g[0]; o[1] = g[1]; o[2] = g[2]; }
  }
}

// grid (blocks of MTILE valid pixels, views): part[v][block][12]. x = M^T q, q = d z + c: g_q = M g_x (g_xyz null: the colours are
// constants) + the shading's g_q; g_d = z g_q, g_c = g_q; the explicit R term of R l_m goes straight into the ray part's nine sums.
DISTR_GLOBAL void __launch_bounds__(MB) k_cb_cam_bwd(const Geo G, const Cams C, const Lights L, const int32_t* __restrict__ index,
                                                     const int* __restrict__ totals, const float* __restrict__ col, const float* __restrict__ g_rgb,
                                                     const float* __restrict__ g_xyz, int nblk, float* __restrict__ part) {
  __shared__ float lds[MB];
  const int v = blockIdx.y, N = min(totals[v], G.P);
  if ((int64_t)blockIdx.x * MTILE >= N) return;       // (block-uniform; k_cb_cam_fin reads the blocks that hold pixels only)
  const size_t vo = (size_t)v * G.P;
  const float* R = C.R + 9 * v;
  const float* loc = L.loc + (int64_t)v * L.lstride;
  const float* en = L.en + (int64_t)v * L.estride;
  const int base = blockIdx.x * MTILE + threadIdx.x * MPER;
  Cam12 acc;
#pragma unroll
  for (int k = 0; k < 12; ++k) acc.a[k] = 0.f;
  for (int t = 0; t < MPER && base + t < N; ++t) {
    const int i = base + t;
    const int pix = valid_pixel(G, index[vo + i]);
    const PixelGeo pg = pixel_geo(G, R, C.T + 3 * v, C.zdepth[vo + pix], pix);
    float gq[3] = {0.f, 0.f, 0.f};
    if (g_xyz) {
      const float* gp = g_xyz + 3 * (vo + i);
#pragma unroll
      for (int j = 0; j < 3; ++j) gq[j] = G.M[j * 3 + 0] * gp[0] + G.M[j * 3 + 1] * gp[1] + G.M[j * 3 + 2] * gp[2];
    }
    if (L.M > 0) {
      const float* c = col + 3 * (vo + i);
      const float* g = g_rgb + 3 * (vo + pix);
      const float* n = C.normal + 3 * (vo + pix);
      const float gs = g[0] * c[0] + g[1] * c[1] + g[2] * c[2];
      float rn[3];                                    // R^T n
#pragma unroll
      for (int k = 0; k < 3; ++k) rn[k] = R[0 * 3 + k] * n[0] + R[1 * 3 + k] * n[1] + R[2 * 3 + k] * n[2];
      for (int m = 0; m < L.M; ++m) {
        const LightDir d = light_dir(loc + 3 * m, pg.q);
        const float w = gs * en[m];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
#pragma unroll
          for (int k = 0; k < 3; ++k) acc.a[j * 3 + k] += w * n[j] * d.l[k];
        }
        const float gl[3] = {w * rn[0], w * rn[1], w * rn[2]};
        const float dot = d.l[0] * gl[0] + d.l[1] * gl[1] + d.l[2] * gl[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) gq[k] -= (gl[k] - d.l[k] * dot) * d.inv;
      }
    }
    float gd[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      gd[j] = gq[j] * pg.z;
      acc.a[9 + j] += gq[j];
    }
    ray_backward_acc(pg.g, gd, acc.a);
  }
  const Cam12 tot = samples::block_sum12(acc, lds);
  if (threadIdx.x < 12) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 12; ++k) t = (int)threadIdx.x == k ? tot.a[k] : t;
    part[((size_t)v * nblk + blockIdx.x) * 12 + threadIdx.x] = t;
  }
}

// one block per view: the view's block sums in block order (thread t: blocks t, t + MB, ...; then the tree) -> g_R[v][9], g_T[v][3]
DISTR_GLOBAL void __launch_bounds__(MB) k_cb_cam_fin(const Geo G, const Cams C, const int* __restrict__ totals, const float* __restrict__ part,
                                                     int nblk, float* __restrict__ g_R, float* __restrict__ g_T) {
  __shared__ float lds[MB];
  const int v = blockIdx.x;
  const int nb = min((min(totals[v], G.P) + MTILE - 1) / MTILE, nblk);
  Cam12 acc;
#pragma unroll
  for (int k = 0; k < 12; ++k) acc.a[k] = 0.f;
  for (int b = threadIdx.x; b < nb; b += MB) {
    const float* p = part + ((size_t)v * nblk + b) * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) acc.a[k] += p[k];
  }
  const Cam12 tot = samples::block_sum12(acc, lds);
  if (threadIdx.x == 0) {
    const float* R = C.R + 9 * v;
    const float* T = C.T + 3 * v;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (g_R) g_R[9 * v + j * 3 + i] = tot.a[j * 3 + i] - T[j] * tot.a[9 + i];
      if (g_T) g_T[3 * v + j] = -(R[j * 3 + 0] * tot.a[9] + R[j * 3 + 1] * tot.a[10] + R[j * 3 + 2] * tot.a[11]);
    }
  }
}

// The decoder list of the backward, written out (distr_color_stage_samples_export_batch, include/distr_color_train.h): grid (blocks of MB
// list positions, views). Row r < N_v of view v: the point k_cb_points built, the upstream k_cb_bwd_pre wrote and the pixel, from
// [v * P + r] of the workspaces to [v * cap + r] of the outputs; rows at or beyond N_v are not touched. counts[v] = N_v, the scan's total.
// Reads both workspaces, changes neither.
DISTR_GLOBAL void __launch_bounds__(MB) k_cb_export(int P, const int* __restrict__ totals, const int32_t* __restrict__ index,
                                                    const float* __restrict__ xyz, const float* __restrict__ g_col, float* __restrict__ xyz_out,
                                                    float* __restrict__ up_out, int32_t* __restrict__ index_out, int64_t cap,
                                                    int32_t* __restrict__ counts) {
  const int v = blockIdx.y;
  const int N = max(min(totals[v], P), 0);          // (P <= cap: checked by the host)
  if (blockIdx.x == 0 && threadIdx.x == 0) counts[v] = N;
  const int i = blockIdx.x * MB + threadIdx.x;
  if (i >= N) return;
  const size_t from = (size_t)v * P + i, to = (size_t)v * (size_t)cap + i;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    xyz_out[3 * to + k] = xyz[3 * from + k];
    up_out[3 * to + k] = g_col[3 * from + k];
  }
  if (index_out) index_out[to] = index[from];
}

}  // namespace cbatch
}  // namespace distr
