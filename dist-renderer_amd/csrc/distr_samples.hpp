// distr_samples.hpp -- depth maps back-projected into SDF samples (reference: core/sdfrenderer/renderer_deepsdf.py:10-64,
// SDFRenderer_deepsdf.get_samples / get_freespace_samples): the kernels around one decoder evaluation on a point list.
//
//   1 k_samp_count    per view, per block of MTILE pixels: number of valid pixels (0 < depth < 1e5)
//   2 k_samp_top_scan per view: exclusive scan of the block counts, the view's total behind them (what the host reads, once)
//   3 k_samp_compact  block-local scan again: the valid pixels of view v, in row-major order, into index[v][0 .. N_v)
//   4 k_samp_points   per valid pixel: ray and camera position from R, T, K^-1 (make_ray / make_point of the march), zdepth = depth / calib,
//                     then the point list of the decoder: SURFACE p + eta M^T n | p - eta M^T n, FREESPACE number points at zdepth * ratio
//     (decoder evaluation on the whole list: k_march<eval>, distr_api.hip)
//   5 k_samp_epilogue SURFACE: f(p + o) - eta, f(p - o) + eta, in place
//   backward (after the point-list backward, k_bwd<pointgrad>, has written g_xyz):
//   6 k_samp_cam_bwd  per valid pixel: g_xyz of its points pulled back through M^T, the ray normalisation and R^T h (float64); 12 sums per block
//   7 k_samp_cam_fin  per view: the block sums in block order, then g_R = ray part - T (x) g_c, g_T = -R g_c
//
// Positions come from scans in a fixed order and sums from fixed trees (per-thread serial run -> LDS tree -> block order): no atomics,
// the same bytes on every run. Lists are per view: view v's N_v pixels own m N_v consecutive list entries (m = 2 or `number`) starting
// at m * (N_0 + ... + N_(v-1)); inside a view the list is [k][i] (k = 0 pos / 1 neg, or the draw; i = valid pixel). Every kernel indexes
// (block, view) -> a view's blocks and trees are those of a stand-alone call of that view.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "distr_kernels.hpp"    // make_ray, make_point
#include "distr_mesh.hpp"       // block_excl_scan, MB / MPER / MTILE

namespace distr {
namespace samples {

using mesh::MB;
using mesh::MPER;
using mesh::MTILE;

constexpr int MODE_SURFACE = 0;     // DISTR_SAMPLES_SURFACE
constexpr int MODE_FREESPACE = 1;   // DISTR_SAMPLES_FREESPACE

struct Geo {                        // per call
  int H, W, P;                      // P = H * W
  float Ki[9], M[9];
  int mode, m;                      // m = list entries per valid pixel: 2 (SURFACE) or `number` (FREESPACE)
};

struct Views {                      // per view: valid pixels and the view's first valid pixel in the concatenated order (host knowledge)
  int32_t n[DISTR_MAX_VIEWS];
  int32_t off[DISTR_MAX_VIEWS];
};

__device__ __forceinline__ bool depth_valid(float d) { return d > 0.f && d < 1e5f; }

DISTR_GLOBAL void __launch_bounds__(MB) k_samp_count(const float* __restrict__ depth, int P, int nb, int* __restrict__ btot) {
  __shared__ int lds[MB];
  const int v = blockIdx.y;
  const float* d = depth + (size_t)v * P;
  const int base = blockIdx.x * MTILE + threadIdx.x * MPER;
  int s = 0;
  for (int q = 0; q < MPER && base + q < P; ++q) s += depth_valid(d[base + q]) ? 1 : 0;
  int tot;
  mesh::block_excl_scan(s, lds, &tot);
  if (threadIdx.x == 0) btot[(size_t)v * nb + blockIdx.x] = tot;
}

// one block per view: boff[v][b] = sum of btot[v][0..b), totals[v] = the view's count
DISTR_GLOBAL void __launch_bounds__(MB) k_samp_top_scan(const int* __restrict__ btot, int nb, int* __restrict__ boff, int* __restrict__ totals) {
  __shared__ int lds[MB];
  const int v = blockIdx.x;
  int carry = 0;
  for (int b0 = 0; b0 < nb; b0 += MB) {
    const int b = b0 + threadIdx.x;
    const int x = b < nb ? btot[(size_t)v * nb + b] : 0;
    int tot;
    const int ex = mesh::block_excl_scan(x, lds, &tot);
    if (b < nb) boff[(size_t)v * nb + b] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) totals[v] = carry;
}

DISTR_GLOBAL void __launch_bounds__(MB) k_samp_compact(const float* __restrict__ depth, int P, int nb, const int* __restrict__ boff,
                                                       int* __restrict__ index) {
  __shared__ int lds[MB];
  const int v = blockIdx.y;
  const float* d = depth + (size_t)v * P;
  const int base = blockIdx.x * MTILE + threadIdx.x * MPER;
  int s = 0;
  for (int q = 0; q < MPER && base + q < P; ++q) s += depth_valid(d[base + q]) ? 1 : 0;
  int tot;
  int at = boff[(size_t)v * nb + blockIdx.x] + mesh::block_excl_scan(s, lds, &tot);
  int* out = index + (size_t)v * P;          // at < the view's count <= P
  for (int q = 0; q < MPER && base + q < P; ++q)
    if (depth_valid(d[base + q])) out[at++] = base + q;
}

// an index entry outside the image (counts that are not those of distr_depth_samples_count) reads pixel 0, never out of bounds
__device__ __forceinline__ int valid_pixel(const Geo& G, int pix) { return (unsigned)pix < (unsigned)G.P ? pix : 0; }

struct PixelGeo { RayGeo g; float c[3]; float z; };

// ray of pixel `pix`, camera position c = -R^T T (the order of k_prep), zdepth = depth / calib_map
__device__ __forceinline__ PixelGeo pixel_geo(const Geo& G, const float* RT, const float* __restrict__ depth, int pix) {
  float R[9], T[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int i = 0; i < 3; ++i) R[j * 3 + i] = RT[j * 4 + i];
    T[j] = RT[j * 4 + 3];
  }
  PixelGeo pg;
  pg.g = make_ray(G.Ki, R, (float)(pix % G.W), (float)(pix / G.W));
#pragma unroll
  for (int i = 0; i < 3; ++i) pg.c[i] = -(R[0 * 3 + i] * T[0] + R[1 * 3 + i] * T[1] + R[2 * 3 + i] * T[2]);
  pg.z = depth[pix] / pg.g.calib;
  return pg;
}

// grid (blocks of MB valid pixels, views). draws: SURFACE eta_map[off_v + i]; FREESPACE ratio[m * off_v + k * N_v + i]
DISTR_GLOBAL void __launch_bounds__(MB) k_samp_points(const Geo G, const Views VW, const int* __restrict__ index, const float* __restrict__ RT,
                                                      const float* __restrict__ depth, const float* __restrict__ normal,
                                                      const float* __restrict__ draws, float* __restrict__ xyz) {
  const int v = blockIdx.y, N = VW.n[v];
  const int i = blockIdx.x * MB + threadIdx.x;
  if (i >= N) return;
  const int64_t off = VW.off[v];
  const int pix = valid_pixel(G, index[(size_t)v * G.P + i]);
  const PixelGeo pg = pixel_geo(G, RT + 12 * v, depth + (size_t)v * G.P, pix);
  float* out = xyz + 3 * (int64_t)G.m * off;
  if (G.mode == MODE_SURFACE) {
    float p[3];
    make_point(G.M, pg.c, pg.g.d, pg.z, p);
    const float* n = normal + 3 * ((size_t)v * G.P + pix);
    const float eta = draws[off + i];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float o = (G.M[0 * 3 + k] * n[0] + G.M[1 * 3 + k] * n[1] + G.M[2 * 3 + k] * n[2]) * eta;
      out[3 * (int64_t)i + k] = p[k] + o;
      out[3 * ((int64_t)N + i) + k] = p[k] - o;
    }
  } else {
    for (int k = 0; k < G.m; ++k) {
      float p[3];
      make_point(G.M, pg.c, pg.g.d, pg.z * draws[(int64_t)G.m * off + (int64_t)k * N + i], p);
      float* d = out + 3 * ((int64_t)k * N + i);
      d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
    }
  }
}

// SURFACE: out = [f(p + o) - eta | f(p - o) + eta] per view, in place on the decoder outputs
DISTR_GLOBAL void __launch_bounds__(MB) k_samp_epilogue(const Views VW, const float* __restrict__ eta, float* __restrict__ out) {
  const int v = blockIdx.y, N = VW.n[v];
  const int i = blockIdx.x * MB + threadIdx.x;
  if (i >= N) return;
  const int64_t off = VW.off[v];
  const float e = eta[off + i];
  float* o = out + 2 * off;
  o[i] = o[i] - e;
  o[(int64_t)N + i] = o[(int64_t)N + i] + e;
}

struct Cam12 { float a[12]; };     // gR (ray part) [9], g_c [3]
__device__ __forceinline__ Cam12 operator+(Cam12 x, Cam12 y) {
  Cam12 r;
#pragma unroll
  for (int k = 0; k < 12; ++k) r.a[k] = x.a[k] + y.a[k];
  return r;
}

// sum of one Cam12 per thread over the block: a fixed binary tree in LDS, component by component; every thread returns the total
__device__ __forceinline__ Cam12 block_sum12(Cam12 x, float* lds /*[MB]*/) {
  Cam12 r;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    lds[threadIdx.x] = x.a[k];
    __syncthreads();
    for (int s = MB / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) lds[threadIdx.x] = lds[threadIdx.x] + lds[threadIdx.x + s];
      __syncthreads();
    }
    r.a[k] = lds[0];
    __syncthreads();
  }
  return r;
}

// make_ray for the camera pull-back, in float64: h = K^-1 (x, y, 1), r = R^T h, |r|, calib = h_z / (|h| + 1e-12)
struct Ray64 { double h[3], r[3], rn, calib; };
__device__ __forceinline__ Ray64 make_ray64(const Geo& G, const float* RT, int pix) {
  Ray64 g;
  const double px = (double)(pix % G.W), py = (double)(pix / G.W);
#pragma unroll
  for (int a = 0; a < 3; ++a) g.h[a] = (double)G.Ki[a * 3 + 0] * px + (double)G.Ki[a * 3 + 1] * py + (double)G.Ki[a * 3 + 2];
  g.calib = g.h[2] / (sqrt(g.h[0] * g.h[0] + g.h[1] * g.h[1] + g.h[2] * g.h[2]) + 1e-12);
#pragma unroll
  for (int i = 0; i < 3; ++i) g.r[i] = (double)RT[0 * 4 + i] * g.h[0] + (double)RT[1 * 4 + i] * g.h[1] + (double)RT[2 * 4 + i] * g.h[2];
  g.rn = sqrt(g.r[0] * g.r[0] + g.r[1] * g.r[1] + g.r[2] * g.r[2]);
  return g;
}

// grid (blocks of MTILE valid pixels, views): part[v][block][12]. Point p = M^T q, q = d z + c: g_q = M g_p, g_d = sum_k z_k g_q_k,
// g_c = sum_k g_q_k (z_k = zdepth, or zdepth * ratio_k; the +-offset of SURFACE does not depend on the camera).
// A pixel's own twelve terms are formed in float64 and rounded once: g_r = g_d / e - (g_d . r) r / (rn e^2) takes the part of g_d along the
// ray away component by component, and g_d sums list entries whose upstream gradients differ in sign; in float32 the roundings of the
// parts are not small against what is left (a view with ONE valid pixel was up to 3e-4 off in an entry). The sums stay float32.
DISTR_GLOBAL void __launch_bounds__(MB) k_samp_cam_bwd(const Geo G, const Views VW, const int* __restrict__ index, const float* __restrict__ RT,
                                                       const float* __restrict__ depth, const float* __restrict__ draws,
                                                       const float* __restrict__ g_xyz, int nblk, float* __restrict__ part) {
  __shared__ float lds[MB];
  const int v = blockIdx.y, N = VW.n[v];
  const int64_t off = VW.off[v];
  const float* gx = g_xyz + 3 * (int64_t)G.m * off;
  const int base = blockIdx.x * MTILE + threadIdx.x * MPER;
  Cam12 acc;
#pragma unroll
  for (int k = 0; k < 12; ++k) acc.a[k] = 0.f;
  for (int q = 0; q < MPER && base + q < N; ++q) {
    const int i = base + q;
    const int pix = valid_pixel(G, index[(size_t)v * G.P + i]);
    const Ray64 g = make_ray64(G, RT + 12 * v, pix);
    const double z = (double)depth[(size_t)v * G.P + pix] / g.calib;
    double gd[3] = {0.0, 0.0, 0.0}, gc[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < G.m; ++k) {
      const float* gp = gx + 3 * ((int64_t)k * N + i);
      const double zk = G.mode == MODE_SURFACE ? z : z * (double)draws[(int64_t)G.m * off + (int64_t)k * N + i];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double gq = (double)G.M[j * 3 + 0] * gp[0] + (double)G.M[j * 3 + 1] * gp[1] + (double)G.M[j * 3 + 2] * gp[2];
        gd[j] += gq * zk;
        gc[j] += gq;
      }
    }
    const double e = g.rn + 1e-12;
    const double dot = gd[0] * g.r[0] + gd[1] * g.r[1] + gd[2] * g.r[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double gr = gd[c] / e - (g.rn > 0.0 ? dot * g.r[c] / (g.rn * e * e) : 0.0);
#pragma unroll
      for (int j = 0; j < 3; ++j) acc.a[j * 3 + c] += (float)(g.h[j] * gr);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) acc.a[9 + j] += (float)gc[j];
  }
  const Cam12 tot = block_sum12(acc, lds);
  if (threadIdx.x < 12) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 12; ++k) t = (int)threadIdx.x == k ? tot.a[k] : t;
    part[((size_t)v * nblk + blockIdx.x) * 12 + threadIdx.x] = t;
  }
}

// one block per view: the view's block sums added in block order (thread t: blocks t, t + MB, ...; then the tree), then
// c = -R^T T: g_R[j][i] = ray part - T[j] g_c[i], g_T[j] = -sum_i R[j][i] g_c[i] -> g_RT[v] (3, 4)
DISTR_GLOBAL void __launch_bounds__(MB) k_samp_cam_fin(const Views VW, const float* __restrict__ RT, const float* __restrict__ part, int nblk,
                                                       float* __restrict__ g_RT) {
  __shared__ float lds[MB];
  const int v = blockIdx.x;
  const int nb = (VW.n[v] + MTILE - 1) / MTILE;       // blocks of this view that hold pixels (<= nblk)
  Cam12 acc;
#pragma unroll
  for (int k = 0; k < 12; ++k) acc.a[k] = 0.f;
  for (int b = threadIdx.x; b < nb; b += MB) {
    const float* p = part + ((size_t)v * nblk + b) * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) acc.a[k] += p[k];
  }
  const Cam12 tot = block_sum12(acc, lds);
  if (threadIdx.x == 0) {
    const float* rt = RT + 12 * v;
    float* g = g_RT + 12 * v;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
      for (int i = 0; i < 3; ++i) g[j * 4 + i] = tot.a[j * 3 + i] - rt[j * 4 + 3] * tot.a[9 + i];
      g[j * 4 + 3] = -(rt[j * 4 + 0] * tot.a[9] + rt[j * 4 + 1] * tot.a[10] + rt[j * 4 + 2] * tot.a[11]);
    }
  }
}

}  // namespace samples
}  // namespace distr
