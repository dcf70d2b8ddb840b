// distr_normal_grad.hpp -- the decoder-path term of the autograd normals' backward (include/distr_normal_grad.h; reference:
// render_normal differentiates decode_sdf_gradient(create_graph=True) a second time, core/utils/decoder_utils.py:76-92,
// core/sdfrenderer/renderer.py:880-910): the kernels around ONE decoder backward over the valid pixels of every view.
//
// A ReLU decoder is piecewise linear in (code, x). With f = tanh(u) the raw normal of a pixel is h = 3 1[|f| <= clamp] (1 - f^2) grad_x u and
// grad_x u is locally constant, so a loss L(h) reaches code and camera through f alone: with g = dL/dh,
//     g_f = -2 f (g . h) / (1 - f^2)
// is the upstream gradient of f at the surface point x = M^T (c + d z) (z detached: has_zdepth_grad=False, renderer.py:895), and the rest
// is the ordinary first-order backward of the decoder at x. Unit normals (normalize_normal) are scale invariant: no term.
//
//   1 k_ng_count     per view, per block of MTILE pixels: number of valid pixels (the forward's final mask, View::mask_s)
//   2 k_samp_top_scan (distr_samples.hpp) per view: exclusive scan of the block counts, the view's total N_v behind them
//   3 k_ng_compact   the valid pixels of view v in row-major order -> index[v][0 .. N_v)
//   4 k_ng_gather    per valid pixel: x from camera, ray (recomputed) and Zdepth; g = M_normal^T R^T flip(g_normal) taken against the saved
//                    M_normal h (View::nrm_t): g . h = (R^T flip(g_normal)) . (M_normal h)
//   5 k_ng_consts64, k_ng_f64   f at the surface points in float64 (the term is proportional to f, which is nearly zero there), and g_f
//   6 k_ng_seg_table the tile table of the segmented point list from the DEVICE counts: segment v = N_v points at v * P
//     (decoder backward over the list: k_bwd<pointgrad+latent>, k_points_latent_grad -- distr_api.hip)
//   7 k_ng_cam_bwd   per valid pixel: g_x pulled back through M^T, the ray normalisation and R^T h; 12 sums per block
//   8 k_ng_cam_fin   per view: the block sums in block order, then c = -R^T T: g_R = ray part - T (x) g_c, g_T = -R g_c
//
// No atomics and no host read: list positions come from a scan in a fixed order, sums from fixed trees (thread-serial run -> LDS tree ->
// block order), counts stay on the device. Every kernel indexes (block, view): a view's blocks, tiles and trees are those of its own call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "distr_kernels.hpp"
#include "distr_samples.hpp"    // MB / MPER / MTILE, Cam12, block_sum12, k_samp_top_scan

namespace distr {
namespace ngrad {

using samples::MB;
using samples::MPER;
using samples::MTILE;
using samples::Cam12;

struct Lists {               // workspace arrays of one call; per-view arrays are [nviews][P]
  int32_t* index;            // compacted valid pixels
  const int* totals;         // [nviews] N_v
  float* xyz;                // [nviews * P][3] surface points, view v from v * P on
  float* gf;                 // [nviews * P]    g . h (k_ng_gather), then the upstream gradient of f (k_ng_f64)
  float* g_xyz;              // [nviews * P][3] decoder backward: d / d surface point
};

__device__ __forceinline__ const uint8_t* mask_of(const View& V0, int v) {
  return reinterpret_cast<const uint8_t*>(reinterpret_cast<const char*>(V0.mask_s) + (int64_t)v * V0.vstride);
}

DISTR_GLOBAL void __launch_bounds__(MB) k_ng_count(View V0, int nb, int* __restrict__ btot) {
  __shared__ int lds[MB];
  const int v = blockIdx.y, P = V0.P;
  const uint8_t* m = mask_of(V0, v);
  const int base = blockIdx.x * MTILE + threadIdx.x * MPER;
  int s = 0;
  for (int q = 0; q < MPER && base + q < P; ++q) s += m[base + q] ? 1 : 0;
  int tot;
  mesh::block_excl_scan(s, lds, &tot);
  if (threadIdx.x == 0) btot[(size_t)v * nb + blockIdx.x] = tot;
}

DISTR_GLOBAL void __launch_bounds__(MB) k_ng_compact(View V0, int nb, const int* __restrict__ boff, int32_t* __restrict__ index) {
  __shared__ int lds[MB];
  const int v = blockIdx.y, P = V0.P;
  const uint8_t* m = mask_of(V0, v);
  const int base = blockIdx.x * MTILE + threadIdx.x * MPER;
  int s = 0;
  for (int q = 0; q < MPER && base + q < P; ++q) s += m[base + q] ? 1 : 0;
  int tot;
  int at = boff[(size_t)v * nb + blockIdx.x] + mesh::block_excl_scan(s, lds, &tot);
  int32_t* out = index + (size_t)v * P;      // at < the view's count <= P
  for (int q = 0; q < MPER && base + q < P; ++q)
    if (m[base + q]) out[at++] = base + q;
}

// grid (blocks of MB valid pixels, views); g_normal [nviews][P][3]
DISTR_GLOBAL void __launch_bounds__(MB) k_ng_gather(View V0, Lists L, const float* __restrict__ g_normal) {
  const int v = blockIdx.y;
  const int i = blockIdx.x * MB + threadIdx.x;
  if (i >= L.totals[v]) return;
  const View V = view_at(V0, v);
  const size_t vo = (size_t)v * V.P;
  const int px = L.index[vo + i];
  const CamRegs cam = load_cam(V.C);
  float cx, cy;
  level_center(V.lv[0], px, cx, cy);
  const RayGeo g = make_ray(V.cfg.K_inv, cam.R, cx, cy);
  float p[3];
  make_point(V.cfg.M, cam.c, g.d, V.zdepth_s[px], p);
  float* x = L.xyz + 3 * (vo + i);
  x[0] = p[0]; x[1] = p[1]; x[2] = p[2];
  // g . h with h = the raw normal: nrm_t holds M_normal h (zero outside the clamp), so g . h = (R^T flip(g_normal)) . nrm_t
  const float* gn = g_normal + 3 * (vo + px);
  const float go[3] = {-gn[0], gn[1], gn[2]};
  const float* t = V.nrm_t + (size_t)px * 3;
  float gh = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) gh += (cam.R[0 * 3 + k] * go[0] + cam.R[1 * 3 + k] * go[1] + cam.R[2 * 3 + k] * go[2]) * t[k];
  L.gf[vo + i] = gh;        // k_ng_f64 turns it into g_f
}

// ---- f at the surface points in float64. The term is proportional to f, and a surface sample has |f| ~ 1e-6 to 1e-5: the float32 tile
// evaluates f to ~1e-7 absolute (activations of size 1), which is 1e-2 of the term per pixel. So f alone is evaluated again here -- the
// point formed in float64 from the float32 camera, ray constants and depth, the float32 weights promoted exactly, every sum in float64;
// h and the first-order backward stay in float32 (relative 1e-6, like every other gradient).
constexpr int FP = 8;        // points per block: activations [512][FP] doubles = 32 KiB of LDS

// c0 = b0 + W0[:, :C] code and c4 likewise, in float64: c64[view][1024]. grid (4, views), 256 threads (as k_latent_consts)
DISTR_GLOBAL void __launch_bounds__(256) k_ng_consts64(View V0, DecoderDev D, double* __restrict__ c64) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int o = gid & (HID - 1);
  const float* Wt = (gid < HID) ? D.W0lat_t : D.W4lat_t;
  const float* latent = view_at(V0, blockIdx.y).C->latent;
  double acc = (gid < HID) ? D.b0[o] : D.b4[o];
  for (int k = 0; k < D.nlat; ++k) acc = fma((double)Wt[k * HID + o], (double)latent[k], acc);
  c64[(size_t)blockIdx.y * (2 * HID) + gid] = acc;
}

// One layer on the block's FP points: X [K][FP] -> relu(init + W X) [O][FP], in place. Thread t owns rows t and t + 256 (O = 512) or row t
// (O = 256). W is read from the tile kernels' forward A-fragments (pack_fragments, distr_api.hip): float4 index
// g * (4 * NOB * 64) + (o / 32) * 64 + (o & 31) + 32 hh = { W[o][8g + 2s + hh] : s = 0..3 }, NOB = O / 128.
template <class Init>
__device__ __forceinline__ void layer64(const float* __restrict__ Wf, int K, int O, Init init, double* X) {
  const int tid = threadIdx.x;
  const bool two = O > 256;
  const size_t gstride = (size_t)4 * (O / 128) * 64;
  const int o1 = two ? tid + 256 : tid;
  const float4* w0p = reinterpret_cast<const float4*>(Wf) + (tid >> 5) * 64 + (tid & 31);
  const float4* w1p = reinterpret_cast<const float4*>(Wf) + (o1 >> 5) * 64 + (o1 & 31);
  double a0[FP], a1[FP];
  const double i0 = init(tid), i1 = init(o1);
#pragma unroll
  for (int p = 0; p < FP; ++p) { a0[p] = i0; a1[p] = i1; }
  for (int g = 0; g < K / 8; ++g) {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const float4 w0 = w0p[g * gstride + 32 * hh], w1 = w1p[g * gstride + 32 * hh];
      const float u0[4] = {w0.x, w0.y, w0.z, w0.w}, u1[4] = {w1.x, w1.y, w1.z, w1.w};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const double* x = X + (8 * g + 2 * s + hh) * FP;
#pragma unroll
        for (int p = 0; p < FP; ++p) {
          a0[p] = fma((double)u0[s], x[p], a0[p]);
          a1[p] = fma((double)u1[s], x[p], a1[p]);
        }
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < FP; ++p) {
    X[tid * FP + p] = fmax(a0[p], 0.0);
    if (two) X[o1 * FP + p] = fmax(a1[p], 0.0);
  }
  __syncthreads();
}

// grid (blocks of FP valid pixels, views), 256 threads: gf[i] = gh (k_ng_gather) -> g_f = -2 f gh / (1 - f^2), zero outside the clamp
DISTR_GLOBAL void __launch_bounds__(256) k_ng_f64(View V0, Lists L, DecoderDev D, const double* __restrict__ c64, int wide) {
  __shared__ double X[HID * FP];
  __shared__ double xs[3 * FP];
  const int v = blockIdx.y, N = L.totals[v], tid = threadIdx.x;
  if ((int64_t)blockIdx.x * FP >= N) return;       // (block-uniform)
  const View V = view_at(V0, v);
  const size_t vo = (size_t)v * V.P;
  const double* c0 = c64 + (size_t)v * (2 * HID);
  const double* c4 = c0 + HID;
  if (tid < FP) {      // the surface point (points past the list's end repeat its last one; nothing is written for them)
    const int px = L.index[vo + min((int)blockIdx.x * FP + tid, N - 1)];
    float cx, cy;
    level_center(V.lv[0], px, cx, cy);
    const float* Ki = V.cfg.K_inv;
    const Consts* C = V.C;
    double h[3], r[3], c[3], q[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) h[j] = (double)Ki[3 * j] * cx + (double)Ki[3 * j + 1] * cy + (double)Ki[3 * j + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      r[i] = (double)C->R[i] * h[0] + (double)C->R[3 + i] * h[1] + (double)C->R[6 + i] * h[2];
      c[i] = -((double)C->R[i] * C->T[0] + (double)C->R[3 + i] * C->T[1] + (double)C->R[6 + i] * C->T[2]);
    }
    const double rn = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) + 1e-12, z = V.zdepth_s[px];
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = r[i] / rn * z + c[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) xs[i * FP + tid] = (double)V.cfg.M[i] * q[0] + (double)V.cfg.M[3 + i] * q[1] + (double)V.cfg.M[6 + i] * q[2];
  }
  __syncthreads();
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {      // lin0: the code is folded into c0
    const int o = tid + 256 * rr;
    const double w[3] = {D.W0x[o], D.W0x[HID + o], D.W0x[2 * HID + o]};
#pragma unroll
    for (int p = 0; p < FP; ++p) X[o * FP + p] = fmax(fma(w[0], xs[p], fma(w[1], xs[FP + p], fma(w[2], xs[2 * FP + p], c0[o]))), 0.0);
  }
  __syncthreads();
  const int O3 = wide ? HID : HID / 2;      // lin3's rows in the tile layout; its last three carry the point into lin4
  layer64(D.Wf[1], HID, HID, [&](int o) { return (double)D.bias[1][o]; }, X);
  layer64(D.Wf[2], HID, HID, [&](int o) { return (double)D.bias[2][o]; }, X);
  layer64(D.Wf[3], HID, O3, [&](int o) { return (double)D.bias[3][o]; }, X);
  if (tid < 3 * FP) X[(O3 - 3 + tid / FP) * FP + tid % FP] = xs[tid];
  __syncthreads();
  layer64(D.Wf[4], O3, HID, [&](int o) { return c4[o]; }, X);
  layer64(D.Wf[5], HID, HID, [&](int o) { return (double)D.bias[5][o]; }, X);
  layer64(D.Wf[6], HID, HID, [&](int o) { return (double)D.bias[6][o]; }, X);
  layer64(D.Wf[7], HID, HID, [&](int o) { return (double)D.bias[7][o]; }, X);
  // lin8: thread t's two rows, then the 256 partial sums of a point in thread order
  double part[FP];
  {
    const double w0 = D.w8[tid], w1 = D.w8[tid + 256];
#pragma unroll
    for (int p = 0; p < FP; ++p) part[p] = fma(w0, X[tid * FP + p], w1 * X[(tid + 256) * FP + p]);
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < FP; ++p) X[tid * FP + p] = part[p];
  __syncthreads();
  const int i = blockIdx.x * FP + tid;
  if (tid < FP && i < N) {
    double u = D.b8;
    for (int t = 0; t < 256; ++t) u += X[t * FP + tid];
    const double f = tanh(u), gh = L.gf[vo + i];
    const double den = 1.0 - f * f;
    L.gf[vo + i] = (fabs(f) <= (double)V.cfg.clamp_dist && den > 0.0) ? (float)(-2.0 * f * gh / den) : 0.f;
  }
}

// one wavefront: segment v = N_v points from point v * P on, on ceil(N_v / 64) tiles of its own (SegTable, distr_kernels.hpp)
DISTR_GLOBAL void __launch_bounds__(64) k_ng_seg_table(const int* __restrict__ totals, int nviews, int P, SegTable* __restrict__ tab) {
  if (threadIdx.x != 0) return;
  int32_t tiles = 0;
  for (int s = 0; s < DISTR_MAX_VIEWS; ++s) {
    const int32_t n = s < nviews ? min(max(totals[s], 0), P) : 0;
    tab->off[s] = s < nviews ? s * P : 0;
    tab->n[s] = n;
    tiles += (n + SEG_TILE - 1) / SEG_TILE;
    tab->tend[s] = tiles;
  }
}

// grid (blocks of MTILE valid pixels, views): part[v][block][12]. x = M^T q, q = d z + c: g_q = M g_x, g_d = z g_q, g_c = g_q
DISTR_GLOBAL void __launch_bounds__(MB) k_ng_cam_bwd(View V0, Lists L, int nblk, float* __restrict__ part) {
  __shared__ float lds[MB];
  const int v = blockIdx.y, N = L.totals[v];
  if ((int64_t)blockIdx.x * MTILE >= N) return;       // (block-uniform; k_ng_cam_fin reads the blocks that hold pixels only)
  const View V = view_at(V0, v);
  const size_t vo = (size_t)v * V.P;
  const CamRegs cam = load_cam(V.C);
  const int base = blockIdx.x * MTILE + threadIdx.x * MPER;
  Cam12 acc;
#pragma unroll
  for (int k = 0; k < 12; ++k) acc.a[k] = 0.f;
  for (int q = 0; q < MPER && base + q < N; ++q) {
    const int i = base + q;
    const int px = L.index[vo + i];
    float cx, cy;
    level_center(V.lv[0], px, cx, cy);
    const RayGeo g = make_ray(V.cfg.K_inv, cam.R, cx, cy);
    const float z = V.zdepth_s[px];
    const float* gp = L.g_xyz + 3 * (vo + i);
    float gd[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float gq = V.cfg.M[j * 3 + 0] * gp[0] + V.cfg.M[j * 3 + 1] * gp[1] + V.cfg.M[j * 3 + 2] * gp[2];
      gd[j] = gq * z;
      acc.a[9 + j] += gq;
    }
    ray_backward_acc(g, gd, acc.a);
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
DISTR_GLOBAL void __launch_bounds__(MB) k_ng_cam_fin(View V0, const int* __restrict__ totals, const float* __restrict__ part, int nblk,
                                                     float* __restrict__ g_R, float* __restrict__ g_T) {
  __shared__ float lds[MB];
  const int v = blockIdx.x;
  const Consts* C = view_at(V0, v).C;
  const int nb = min((totals[v] + MTILE - 1) / MTILE, nblk);
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
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (g_R) g_R[9 * v + j * 3 + i] = tot.a[j * 3 + i] - C->T[j] * tot.a[9 + i];
      if (g_T) g_T[3 * v + j] = -(C->R[j * 3 + 0] * tot.a[9] + C->R[j * 3 + 1] * tot.a[10] + C->R[j * 3 + 2] * tot.a[11]);
    }
  }
}

}  // namespace ngrad
}  // namespace distr
