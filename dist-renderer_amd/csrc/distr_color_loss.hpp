// distr_color_loss.hpp -- the photometric loss of a batch of colour images (include/distr_color_train.h; reference:
// compute_loss_color(use_ssim=True), core/utils/loss_utils.py:188-209, and loss_ssim / SSIM, core/utils/pytorch_ssim/ssim.py:4-35, which
// run once per view): the masked L1 and the SSIM term, forward and backward, for up to DISTR_MAX_VIEWS views in one launch sequence.
//
//   overlap = mask & gt_mask; l1 = mean |rgb - gt| over the overlap's 3 N entries. For SSIM both images are zeroed off the overlap
//   (x = gt, y = rgb); mu_x, mu_y, E[x^2], E[y^2], E[xy] are 3 x 3 zero-padded box sums, always divided by 9 (AvgPool2d(3, 1, padding=1));
//   A1 = 2 mu_x mu_y + C1, A2 = 2 (E[xy] - mu_x mu_y) + C2, B1 = mu_x^2 + mu_y^2 + C1, B2 = (E[x^2] - mu_x^2) + (E[y^2] - mu_y^2) + C2,
//   ssim = A1 A2 / (B1 B2 + 1e-12); the loss is the mean over 3 H W of clamp((1 - ssim) / 2, 0, 1).
//
//   forward
//   1 k_cl_fwd       a thread per pixel: its nine neighbours straight from global memory (nine pixels x 2 mask bytes + 6 floats, all of them
//                    in L2 after the first touch: an LDS tile with a halo would save reads the cache already absorbs, for more code), the three
//                    channels' loss terms, |rgb - gt| on the overlap; per block the sums by a fixed LDS tree -> part[v][block][3]
//   2 k_cl_fin       a block per view: the block sums in block order (thread t: blocks t, t + 256, ...; then the tree) -> l1, ssim, overlap
//   backward
//   3 k_cl_bwd_part  a thread per pixel: g_s = g_ssim (-1/2 inside the clamp, 0 outside) / (3 H W) times d ssim / d(mu_y, E[y^2], E[xy])
//                    per channel -> dpart[v][pixel][9]
//   4 k_cl_bwd       a thread per pixel: the 3 x 3 gather of the partials (the box mean is its own adjoint), g = (sum g_mu + 2 y sum g_eyy +
//                    x sum g_exy) / 9 + g_l1 sign(rgb - gt) / (3 N); zero off the overlap (the zeroing passes nothing)
//
// No atomics: every sum has a fixed order, so every run gives the same bytes, and every kernel indexes (block, view): a view's blocks and
// trees are those of its own nviews = 1 call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "distr_kernels.hpp"    // DISTR_GLOBAL

namespace distr {
namespace closs {

constexpr int CB = 256;                       // pixels per block
constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f, EPS = 1e-12f;

struct Imgs {                // per call: [v][P][3] images, [v][P] masks
  int H, W, P;
  const float* rgb;
  const float* gt;
  const uint8_t* mask;
  const uint8_t* gt_mask;
};

struct Win { float mx, my, exx, eyy, exy; };

// the five box means of channel c around pixel (py, px) of view offset vo; pixels outside the image or off the overlap count as zero
__device__ __forceinline__ void windows(const Imgs& I, size_t vo, int py, int px, Win w[3]) {
  float sx[3] = {0.f, 0.f, 0.f}, sy[3] = {0.f, 0.f, 0.f}, sxx[3] = {0.f, 0.f, 0.f}, syy[3] = {0.f, 0.f, 0.f}, sxy[3] = {0.f, 0.f, 0.f};
  for (int dy = -1; dy <= 1; ++dy) {
    for (int dx = -1; dx <= 1; ++dx) {
      const int qy = py + dy, qx = px + dx;
      if (qy < 0 || qy >= I.H || qx < 0 || qx >= I.W) continue;
      const size_t q = vo + (size_t)qy * I.W + qx;
      if (!(I.mask[q] && I.gt_mask[q])) continue;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float x = I.gt[3 * q + c], y = I.rgb[3 * q + c];
        sx[c] += x; sy[c] += y; sxx[c] += x * x; syy[c] += y * y; sxy[c] += x * y;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    w[c].mx = sx[c] / 9.0f; w[c].my = sy[c] / 9.0f; w[c].exx = sxx[c] / 9.0f; w[c].eyy = syy[c] / 9.0f; w[c].exy = sxy[c] / 9.0f;
  }
}

struct Terms { float A1, A2, B1, B2, n, D; };
__device__ __forceinline__ Terms ssim_terms(const Win& w) {
  Terms t;
  const float sx = w.exx - w.mx * w.mx, sy = w.eyy - w.my * w.my, sxy = w.exy - w.mx * w.my;
  t.A1 = 2.0f * w.mx * w.my + C1;
  t.A2 = 2.0f * sxy + C2;
  t.B1 = w.mx * w.mx + w.my * w.my + C1;
  t.B2 = sx + sy + C2;
  t.n = t.A1 * t.A2;
  t.D = t.B1 * t.B2 + EPS;
  return t;
}

// sum of one float per thread over the block by a fixed binary tree in LDS; every thread returns the total
__device__ __forceinline__ float block_sum(float x, float* lds /*[CB]*/) {
  lds[threadIdx.x] = x;
  __syncthreads();
  for (int s = CB / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] = lds[threadIdx.x] + lds[threadIdx.x + s];
    __syncthreads();
  }
  const float r = lds[0];
  __syncthreads();
  return r;
}

// grid (blocks of CB pixels, views): part[v][block] = (sum |rgb - gt| on the overlap, sum of the clamped ssim terms, overlap pixels)
DISTR_GLOBAL void __launch_bounds__(CB) k_cl_fwd(const Imgs I, int want_ssim, int nblk, float* __restrict__ part) {
  __shared__ float lds[CB];
  const int v = blockIdx.y;
  const int pix = blockIdx.x * CB + threadIdx.x;
  const size_t vo = (size_t)v * I.P;
  float a = 0.f, t = 0.f, n = 0.f;
  if (pix < I.P) {
    const size_t q = vo + pix;
    if (I.mask[q] && I.gt_mask[q]) {
      n = 1.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) a += fabsf(I.rgb[3 * q + c] - I.gt[3 * q + c]);
    }
    if (want_ssim) {
      Win w[3];
      windows(I, vo, pix / I.W, pix % I.W, w);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const Terms m = ssim_terms(w[c]);
        t += fminf(fmaxf((1.0f - m.n / m.D) / 2.0f, 0.0f), 1.0f);
      }
    }
  }
  const float sa = block_sum(a, lds), st = block_sum(t, lds), sn = block_sum(n, lds);      // (n <= 256 per block, <= 2^24 per view: exact)
  if (threadIdx.x == 0) {
    float* o = part + ((size_t)v * nblk + blockIdx.x) * 3;
    o[0] = sa; o[1] = st; o[2] = sn;
  }
}

// one block per view: the view's block sums in block order -> l1[v] (0 for an empty overlap), ssim[v] (null: not wanted), overlap[v]
DISTR_GLOBAL void __launch_bounds__(CB) k_cl_fin(int P, int nblk, const float* __restrict__ part, float* __restrict__ l1, float* __restrict__ ssim,
                                                 int32_t* __restrict__ overlap) {
  __shared__ float lds[CB];
  const int v = blockIdx.x;
  float a = 0.f, t = 0.f, n = 0.f;
  for (int b = threadIdx.x; b < nblk; b += CB) {
    const float* p = part + ((size_t)v * nblk + b) * 3;
    a += p[0]; t += p[1]; n += p[2];
  }
  const float sa = block_sum(a, lds), st = block_sum(t, lds), sn = block_sum(n, lds);
  if (threadIdx.x == 0) {
    l1[v] = sn > 0.f ? sa / (3.0f * sn) : 0.f;
    if (ssim) ssim[v] = st / (3.0f * (float)P);
    overlap[v] = (int32_t)sn;
  }
}

// grid (blocks of CB pixels, views): dpart[v][pixel][c][0..2] = g_s d ssim / d(mu_y, E[y^2], E[xy]) of channel c
DISTR_GLOBAL void __launch_bounds__(CB) k_cl_bwd_part(const Imgs I, const float* __restrict__ g_ssim, float* __restrict__ dpart) {
  const int v = blockIdx.y;
  const int pix = blockIdx.x * CB + threadIdx.x;
  if (pix >= I.P) return;
  const size_t vo = (size_t)v * I.P;
  Win w[3];
  windows(I, vo, pix / I.W, pix % I.W, w);
  const float scale = g_ssim[v] * -0.5f / (3.0f * (float)I.P);
  float* o = dpart + 9 * (vo + pix);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const Terms m = ssim_terms(w[c]);
    const float tt = (1.0f - m.n / m.D) / 2.0f;
    const float gs = (tt >= 0.0f && tt <= 1.0f) ? scale : 0.0f;             // torch.clamp passes the gradient on [min, max]
    const float dA1 = m.A2 / m.D, dA2 = m.A1 / m.D, dB1 = -m.n * m.B2 / (m.D * m.D), dB2 = -m.n * m.B1 / (m.D * m.D);
    o[3 * c + 0] = gs * (dA1 * 2.0f * w[c].mx - dA2 * 2.0f * w[c].mx + dB1 * 2.0f * w[c].my - dB2 * 2.0f * w[c].my);
    o[3 * c + 1] = gs * dB2;
    o[3 * c + 2] = gs * dA2 * 2.0f;
  }
}

// grid (blocks of CB pixels, views): g_rgb[v][pixel][3]; dpart null: the L1 term alone. overlap[v]: the forward's count
DISTR_GLOBAL void __launch_bounds__(CB) k_cl_bwd(const Imgs I, const float* __restrict__ g_l1, const int32_t* __restrict__ overlap,
                                                 const float* __restrict__ dpart, float* __restrict__ g_rgb) {
  const int v = blockIdx.y;
  const int pix = blockIdx.x * CB + threadIdx.x;
  if (pix >= I.P) return;
  const size_t vo = (size_t)v * I.P, q = vo + pix;
  float* o = g_rgb + 3 * q;
  if (!(I.mask[q] && I.gt_mask[q])) { o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; return; }
  float s[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (dpart) {
    const int py = pix / I.W, px = pix % I.W;
    for (int dy = -1; dy <= 1; ++dy) {
      for (int dx = -1; dx <= 1; ++dx) {
        const int qy = py + dy, qx = px + dx;
        if (qy < 0 || qy >= I.H || qx < 0 || qx >= I.W) continue;
        const float* d = dpart + 9 * (vo + (size_t)qy * I.W + qx);
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] += d[k];
      }
    }
  }
  const int N = overlap[v];                                               // (>= 1: this pixel is on the overlap)
  const float gl = g_l1 ? g_l1[v] / (3.0f * (float)N) : 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float x = I.gt[3 * q + c], y = I.rgb[3 * q + c], d = y - x;
    const float sgn = d > 0.f ? 1.0f : (d < 0.f ? -1.0f : 0.0f);
    o[c] = (s[3 * c] + 2.0f * y * s[3 * c + 1] + x * s[3 * c + 2]) / 9.0f + gl * sgn;
  }
}

}  // namespace closs
}  // namespace distr
