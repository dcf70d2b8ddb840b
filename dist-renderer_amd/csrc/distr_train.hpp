// distr_train.hpp -- the LAYER-WISE decoder path (include/distr_train.h): decode_sdf with gradients to the decoder's
// weights. The fused tiles keep activations in LDS only; a weight gradient needs every point's activations and deltas of a layer at once
// (they are the K dimension of g_W = Delta^T X), so this path runs one GEMM per layer over the whole point list and keeps the layer
// inputs in HBM. Weights are read as plain row-major (out, in) arrays, straight from the caller's tensors: no pack.
//
//   rows      every segment padded to a multiple of 64 rows (TROW): a 64-row block never holds two segments. A padded row has xyz = 0
//             and an upstream gradient of 0 -> its deltas are exactly 0 and it adds exactly nothing to any sum.
//   forward   k_train_rows (row -> point table), k_train_consts (c0 / c4 per segment), k_train_lin0, k_train_gemm<FWD> x 8 (lin1..lin8;
//             lin8 as a GEMM with one or three output columns), k_train_out (tanh, clamp, scatter to the caller's order)
//   network   the host describes it (section 8i): code length L, lin3's rows n3, W4's row stride ld4 = n3 + L + 3 with the columns
//             [lin3 outputs | code | xyz], nout = 1 or 3 output channels. The SDF decoder is L = C, n3 = 509 - C, ld4 = 512, nout = 1.
//   backward  k_train_dz, then per layer 8..1: k_train_gemm<DW> over K slabs + k_train_slab_sum (g_W), k_train_colsum +
//             k_train_colsum_seg + k_train_bias (g_b and, for lin0 / lin4, the xyz and latent columns of g_W), k_train_gemm<DX> (the
//             delta of the layer below, gated by the saved activation); k_train_glatent last.
//   grad_x f  section 8m, at the end of this file: the unit-delta chain, k_train_gx, and the backward for losses on (f, grad_x f):
//             k_train_tan0, k_train_gemm<TAN> x 8, k_train_rowscal, then the walk 8..1 on k_train_combine + k_train_colsum_w.
//
// One LDS-staged tile kernel serves the three GEMM forms; its template arguments are the orientation of the two operands in memory.
// Every sum has a fixed order (k natural inside an MFMA chain, slabs in slab order, 64-row blocks in block order, segments in segment
// order): no atomics, the same bytes on every run and on every machine. HIP C++ and the f32 MFMA builtin only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "distr_mlp.hpp"        // HID, tanh_spec, DISTR_GLOBAL
#include "distr_philox.hpp"     // the dropout mask (section 8g)

namespace distr {
namespace train {

constexpr int TROW = 64;             // rows per block of the padded list (= SEG_TILE)
constexpr int TBM = 128, TBN = 128;  // GEMM block tile: 4 waves as 2 x 2, each 64 x 64 = 2 x 2 MFMA tiles of 32 x 32
constexpr int TBK = 16;              // k per LDS stage
constexpr int TLD = TBM + 4;         // LDS row stride (floats): the transposing stores of a k-contiguous operand hit 64 different banks
constexpr int SLAB_MIN = 256;        // smallest K slab of a weight-gradient GEMM (rows); DISTR_TRAIN_MAX_SLABS slabs at most
constexpr int MAX_SLABS = 64;

struct Segs { int32_t n[DISTR_MAX_VIEWS]; };     // points per segment (0 behind nseg)

typedef float f32x16 __attribute__((ext_vector_type(16)));

// rowpt[row] = index of the row's point in the caller's list, -1 for a padded row; blkseg[row / 64] = the block's segment;
// blkpt0[row / 64] = the index, inside that segment, of the block's first row (a multiple of 64: what the dropout mask counts by)
DISTR_GLOBAL void __launch_bounds__(256) k_train_rows(Segs sg, int nseg, int rows, int32_t* __restrict__ rowpt, int32_t* __restrict__ blkseg,
                                                    int32_t* __restrict__ blkpt0) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  int r0 = 0, p0 = 0, pt = -1, seg = 0, in_seg = 0;
  for (int s = 0; s < nseg; ++s) {
    const int n = sg.n[s], pad = (n + TROW - 1) / TROW * TROW;
    if (row >= r0 && row < r0 + pad) { seg = s; in_seg = row - r0; pt = (row - r0 < n) ? p0 + (row - r0) : -1; }
    r0 += pad; p0 += n;
  }
  rowpt[row] = pt;
  if ((row & (TROW - 1)) == 0) { blkseg[row / TROW] = seg; blkpt0[row / TROW] = in_seg; }
}

// Dropout of one launch (section 8g): keep(row, n) = draw >= thr, the draws of dropout_draws(key, layer, seg_base + blkseg[block],
// (blkpt0[block] + row in block) >> 2, n); a kept value is multiplied by scale, a dropped one stored as +0. The delta GEMM reads scale only.
struct DropArgs {
  uint32_t key0, key1, thr;
  float scale;
  uint32_t seg_base, layer;
  const int32_t* blkseg; const int32_t* blkpt0;
};

// c0[s] = b0 + W0[:, :C] code_s, c4[s] = b4 + W4[:, col4 : col4 + C] code_s, one k-ordered fmaf chain each (the arithmetic of
// k_latent_consts, on row-major weights). C = the code length L of the net, ld4 = W4's row stride, col4 = its first code column (the
// SDF decoder: 512 and 509 - C). grid (4, segments), 256 threads; c0c4[s][1024]
DISTR_GLOBAL void __launch_bounds__(256) k_train_consts(float* __restrict__ c0c4, const float* __restrict__ W0, const float* __restrict__ b0,
                                                      const float* __restrict__ W4, const float* __restrict__ b4, int C, int ld4, int col4,
                                                      const float* __restrict__ latent, int64_t lat_stride) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int o = gid & (HID - 1);
  const float* w = (gid < HID) ? W0 + (size_t)o * (C + 3) : W4 + (size_t)o * ld4 + col4;
  float acc = (gid < HID) ? b0[o] : b4[o];
  latent += (int64_t)blockIdx.y * lat_stride;
  for (int k = 0; k < C; ++k) acc = __builtin_fmaf(w[k], latent[k], acc);
  c0c4[(size_t)blockIdx.y * (2 * HID) + gid] = acc;
}

// lin0: X1[row] = relu(c0[seg] + W0[:, C:] xyz), and the padded point list xyz4[row] = (x, y, z, 0). One row per thread-column pass:
// block = one 64-row block, 256 threads; thread t owns outputs t and t + 256 of every row.
// DROP: dropout behind the relu, one Philox call per four rows.
template <bool DROP>
__device__ __forceinline__ void lin0_block(const float* __restrict__ xyz, const int32_t* __restrict__ rowpt, const int32_t* __restrict__ blkseg,
                                           const float* __restrict__ c0c4, const float* __restrict__ W0, int C,
                                           float* __restrict__ X1, float* __restrict__ xyz4, const DropArgs& d) {
  __shared__ float p[TROW][4];
  const int blk = blockIdx.x, t = threadIdx.x;
  if (t < TROW) {
    const int pt = rowpt[blk * TROW + t];
    float x = 0.f, y = 0.f, z = 0.f;
    if (pt >= 0) { x = xyz[(size_t)pt * 3]; y = xyz[(size_t)pt * 3 + 1]; z = xyz[(size_t)pt * 3 + 2]; }
    p[t][0] = x; p[t][1] = y; p[t][2] = z; p[t][3] = 0.f;
    float* q = xyz4 + ((size_t)blk * TROW + t) * 4;
    q[0] = x; q[1] = y; q[2] = z; q[3] = 0.f;
  }
  __syncthreads();
  const float* c0 = c0c4 + (size_t)blkseg[blk] * (2 * HID);
  for (int h = 0; h < 2; ++h) {
    const int o = t + h * 256;
    const float* w = W0 + (size_t)o * (C + 3) + C;
    const float wx = w[0], wy = w[1], wz = w[2], c = c0[o];
    if (DROP) {
      const uint32_t gs = d.seg_base + (uint32_t)d.blkseg[blk], q0 = (uint32_t)d.blkpt0[blk] >> 2;
      for (int r4 = 0; r4 < TROW; r4 += 4) {
        const Philox4 u = dropout_draws(d.key0, d.key1, d.layer, gs, q0 + (uint32_t)(r4 >> 2), (uint32_t)o);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = r4 + e;
          float a = __builtin_fmaf(wx, p[r][0], c);
          a = __builtin_fmaf(wy, p[r][1], a);
          a = __builtin_fmaf(wz, p[r][2], a);
          a = a > 0.f ? a : 0.f;
          X1[((size_t)blk * TROW + r) * HID + o] = u.v[e] >= d.thr ? a * d.scale : 0.f;
        }
      }
    } else {
      for (int r = 0; r < TROW; ++r) {
        float a = __builtin_fmaf(wx, p[r][0], c);
        a = __builtin_fmaf(wy, p[r][1], a);
        a = __builtin_fmaf(wz, p[r][2], a);
        X1[((size_t)blk * TROW + r) * HID + o] = a > 0.f ? a : 0.f;
      }
    }
  }
}

DISTR_GLOBAL void __launch_bounds__(256) k_train_lin0(const float* __restrict__ xyz, const int32_t* __restrict__ rowpt, const int32_t* __restrict__ blkseg,
                                                    const float* __restrict__ c0c4, const float* __restrict__ W0, int C,
                                                    float* __restrict__ X1, float* __restrict__ xyz4) {
  lin0_block<false>(xyz, rowpt, blkseg, c0c4, W0, C, X1, xyz4, DropArgs());
}

DISTR_GLOBAL void __launch_bounds__(256) k_train_lin0_drop(const float* __restrict__ xyz, const int32_t* __restrict__ rowpt, const int32_t* __restrict__ blkseg,
                                                         const float* __restrict__ c0c4, const float* __restrict__ W0, int C,
                                                         float* __restrict__ X1, float* __restrict__ xyz4, DropArgs d) {
  lin0_block<true>(xyz, rowpt, blkseg, c0c4, W0, C, X1, xyz4, d);
}

// ---- the GEMM tile: C[m][n] = init + sum_k A(m, k) B(k, n), k in natural order.
//   A_K: A is stored [m][k] (k contiguous, row stride lda), else [k][m];  B_K: B is stored [n][k], else [k][n].
//   forward  X W^T     A = X [row][k] (A_K)      B = W [out][in] (B_K)     EPI_FWD: init = bias[n] or ctab[seg(row)][n]; (+ xyz tail); relu
//   delta    Delta W   A = Delta [row][out] (A_K) B = W [out][in] (!B_K)    EPI_GATE: init 0; times [gate[row][n] > 0]
//   weights  Delta^T X A = Delta [row][out] (!A_K) B = X [row][in] (!B_K)   EPI_PART: init 0; blockIdx.z = K slab, its own output
//   tangent  T W^T     A = T [row][k] (A_K)      B = W [out][in] (B_K)     EPI_TAN: init 0, no bias; (+ tail on u4); times [gate > 0]
//                                                                          (section 8m: the forward form, linearised along u)
// Elements outside M, N or K are read as zero and never stored, so no dimension needs to be a multiple of the tile.
constexpr int EPI_FWD = 0, EPI_GATE = 1, EPI_PART = 2, EPI_TAN = 3;

struct GemmArgs {
  const float* A; const float* B; float* Cout;
  int M, N, K;
  int lda, ldb, ldc;
  int vecA, vecB;                 // operand base and row stride are 16-byte aligned: float4 loads where a quad lies inside the matrix
  // EPI_FWD
  const float* bias;              // [N], or null with ctab
  const float* ctab; int ctab_stride; const int32_t* blkseg;    // init of row m = ctab[blkseg[m / 64] * ctab_stride + n]
  const float* tailW; int tail_ld; const float* xyz4;           // three more k behind K: B = tailW[n * tail_ld + d], A = xyz4[m][d]
  int relu;                                                     // (EPI_TAN: the same tail, xyz4 = the padded upstream u4)
  // EPI_GATE, EPI_TAN (null gate: none, lin8's tangent)
  const float* gate; int ldg;
  // EPI_PART
  int slab_len; size_t slab_stride;   // slab z covers k in [z * slab_len, min(K, (z + 1) * slab_len)); output at Cout + z * slab_stride
};

// a 128 x 16 stage of an operand into LDS as S[k][mn]; KC = the operand is k-contiguous in memory. 256 threads, two quads each.
template <bool KC>
__device__ __forceinline__ void stage_load(const float* __restrict__ P, int ld, int mn0, int mn_lim, int k0, int k_lim, int vec, float4 (&r)[2]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int idx = t + p * 256;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (KC) {
      const int mn = mn0 + (idx >> 2), k = k0 + (idx & 3) * 4;
      if (mn < mn_lim && k < k_lim) {
        const float* g = P + (size_t)mn * ld + k;
        if (vec && k + 3 < k_lim) v = *(const float4*)g;
        else {
          v.x = g[0];
          if (k + 1 < k_lim) v.y = g[1];
          if (k + 2 < k_lim) v.z = g[2];
          if (k + 3 < k_lim) v.w = g[3];
        }
      }
    } else {
      const int k = k0 + (idx >> 5), mn = mn0 + (idx & 31) * 4;
      if (k < k_lim && mn < mn_lim) {
        const float* g = P + (size_t)k * ld + mn;
        if (vec && mn + 3 < mn_lim) v = *(const float4*)g;
        else {
          v.x = g[0];
          if (mn + 1 < mn_lim) v.y = g[1];
          if (mn + 2 < mn_lim) v.z = g[2];
          if (mn + 3 < mn_lim) v.w = g[3];
        }
      }
    }
    r[p] = v;
  }
}

template <bool KC>
__device__ __forceinline__ void stage_store(float (*S)[TLD], const float4 (&r)[2]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int idx = t + p * 256;
    if (KC) {
      const int mn = idx >> 2, k = (idx & 3) * 4;
      S[k][mn] = r[p].x; S[k + 1][mn] = r[p].y; S[k + 2][mn] = r[p].z; S[k + 3][mn] = r[p].w;
    } else {
      const int k = idx >> 5, mn = (idx & 31) * 4;
      *(float4*)&S[k][mn] = r[p];
    }
  }
}

// DROP (section 8g): EPI_FWD drops behind the relu -- a lane's four consecutive rows (r & 3) are the points 4q .. 4q + 3 of one segment, one
// Philox call serves them; EPI_GATE and EPI_TAN multiply the gated value by d.scale (the saved activation of a dropped unit is an exact zero).
template <bool A_K, bool B_K, int EPI, bool DROP>
__device__ __forceinline__ void gemm_tile(const GemmArgs& g, const DropArgs& d) {
  __shared__ __attribute__((aligned(16))) float As[TBK][TLD];
  __shared__ __attribute__((aligned(16))) float Bs[TBK][TLD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int m0 = blockIdx.x * TBM, n0 = blockIdx.y * TBN;      // (x: the dimension that can be long, the rows of the list)
  const int l31 = lane & 31, lh = lane >> 5;

  int kbeg = 0, kend = g.K;
  if (EPI == EPI_PART) {
    kbeg = blockIdx.z * g.slab_len;
    kend = min(g.K, kbeg + g.slab_len);
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float c = 0.f;
      if (EPI == EPI_FWD) {
        const int n = n0 + wn + j * 32 + l31;
        if (n < g.N) {
          if (g.ctab) {
            const int m = m0 + wm;                        // a wave's 64 rows are one 64-row block: one segment
            c = (m < g.M) ? g.ctab[(size_t)g.blkseg[m / TROW] * g.ctab_stride + n] : 0.f;
          } else c = g.bias[n];
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = c;
    }

  float4 ra[2], rb[2];
  stage_load<A_K>(g.A, g.lda, m0, g.M, kbeg, kend, g.vecA, ra);
  stage_load<B_K>(g.B, g.ldb, n0, g.N, kbeg, kend, g.vecB, rb);
  for (int k0 = kbeg; k0 < kend; k0 += TBK) {
    stage_store<A_K>(As, ra);
    stage_store<B_K>(Bs, rb);
    __syncthreads();
    if (k0 + TBK < kend) {
      stage_load<A_K>(g.A, g.lda, m0, g.M, k0 + TBK, kend, g.vecA, ra);
      stage_load<B_K>(g.B, g.ldb, n0, g.N, k0 + TBK, kend, g.vecB, rb);
    }
#pragma unroll
    for (int kk = 0; kk < TBK; kk += 2) {
      const float a0 = As[kk + lh][wm + l31], a1 = As[kk + lh][wm + 32 + l31];
      const float b0 = Bs[kk + lh][wn + l31], b1 = Bs[kk + lh][wn + 32 + l31];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }

  float* out = g.Cout;
  if (EPI == EPI_PART) out += (size_t)blockIdx.z * g.slab_stride;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn + j * 32 + l31;
      if (n >= g.N) continue;
      float tw0 = 0.f, tw1 = 0.f, tw2 = 0.f;
      if ((EPI == EPI_FWD || EPI == EPI_TAN) && g.tailW) {
        const float* w = g.tailW + (size_t)n * g.tail_ld;
        tw0 = w[0]; tw1 = w[1]; tw2 = w[2];
      }
      uint32_t gs = 0, q0 = 0;
      Philox4 u = {{0u, 0u, 0u, 0u}};
      if (EPI == EPI_FWD && DROP) {
        if (m0 + wm >= g.M) continue;                    // (a wave's 64 rows are one 64-row block)
        const int blk = (m0 + wm) / TROW;
        gs = d.seg_base + (uint32_t)d.blkseg[blk];
        q0 = ((uint32_t)d.blkpt0[blk] >> 2) + (uint32_t)(i * 8 + lh);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (EPI == EPI_FWD && DROP && (r & 3) == 0) u = dropout_draws(d.key0, d.key1, d.layer, gs, q0 + (uint32_t)(2 * (r >> 2)), (uint32_t)n);
        const int m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;      // C/D map of the 32 x 32 MFMA: col = lane & 31
        if (m >= g.M) continue;
        float v = acc[i][j][r];
        if (EPI == EPI_FWD) {
          if (g.tailW) {
            const float* q = g.xyz4 + (size_t)m * 4;
            v = __builtin_fmaf(tw0, q[0], v);
            v = __builtin_fmaf(tw1, q[1], v);
            v = __builtin_fmaf(tw2, q[2], v);
          }
          if (g.relu) v = v > 0.f ? v : 0.f;
          if (DROP) v = u.v[r & 3] >= d.thr ? v * d.scale : 0.f;
        }
        if (EPI == EPI_GATE) {
          if (DROP) v = g.gate[(size_t)m * g.ldg + n] > 0.f ? v * d.scale : 0.f;
          else v = g.gate[(size_t)m * g.ldg + n] > 0.f ? v : 0.f;
        }
        if (EPI == EPI_TAN) {
          if (g.tailW) {
            const float* q = g.xyz4 + (size_t)m * 4;
            v = __builtin_fmaf(tw0, q[0], v);
            v = __builtin_fmaf(tw1, q[1], v);
            v = __builtin_fmaf(tw2, q[2], v);
          }
          if (g.gate) {
            if (DROP) v = g.gate[(size_t)m * g.ldg + n] > 0.f ? v * d.scale : 0.f;
            else v = g.gate[(size_t)m * g.ldg + n] > 0.f ? v : 0.f;
          }
        }
        out[(size_t)m * g.ldc + n] = v;
      }
    }
}

template <bool A_K, bool B_K, int EPI>
DISTR_GLOBAL void __launch_bounds__(256, 2) k_train_gemm(GemmArgs g) {      // (2 waves per SIMD: at most 256 registers)
  gemm_tile<A_K, B_K, EPI, false>(g, DropArgs());
}

template <bool A_K, bool B_K, int EPI>
DISTR_GLOBAL void __launch_bounds__(256, 2) k_train_gemm_drop(GemmArgs g, DropArgs d) {
  gemm_tile<A_K, B_K, EPI, true>(g, d);
}

// out = tanh(z), clamped, into the caller's order as out[pt][ch]; th[row][ch] = tanh(z) (unclamped) for the backward. One thread per
// (row, channel) of the nout channels (the host passes clamp < 0 for nout == 3).
DISTR_GLOBAL void __launch_bounds__(256) k_train_out(const float* __restrict__ z, const int32_t* __restrict__ rowpt, int rows, int nout, float clamp,
                                                   float* __restrict__ th, float* __restrict__ sdf) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)rows * nout) return;
  const int row = (int)(i / nout), ch = (int)(i - (int64_t)row * nout);
  const float s = tanh_spec(z[i]);
  th[i] = s;
  const int pt = rowpt[row];
  if (pt >= 0) sdf[(size_t)pt * nout + ch] = clamp >= 0.f ? fminf(fmaxf(s, -clamp), clamp) : s;
}

// delta at the output: dz[row][ch] = g_out[pt][ch] (1 - tanh^2), 0 where the clamp cut and for a padded row
DISTR_GLOBAL void __launch_bounds__(256) k_train_dz(const float* __restrict__ g_sdf, const float* __restrict__ th, const int32_t* __restrict__ rowpt,
                                                  int rows, int nout, float clamp, float* __restrict__ dz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)rows * nout) return;
  const int row = (int)(i / nout), ch = (int)(i - (int64_t)row * nout);
  const int pt = rowpt[row];
  float d = 0.f;
  if (pt >= 0) {
    const float s = th[i];
    if (!(clamp >= 0.f && fabsf(s) > clamp)) d = g_sdf[(size_t)pt * nout + ch] * (1.f - s * s);
  }
  dz[i] = d;
}

// g_W = the slab partials in slab order. out[m * ldo + n] for m < M, n < N; part[slab][M * N]
DISTR_GLOBAL void __launch_bounds__(256) k_train_slab_sum(const float* __restrict__ part, int nslab, int M, int N, float* __restrict__ out, int ldo) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, MN = (size_t)M * N;
  if (i >= MN) return;
  float s = part[i];
  for (int z = 1; z < nslab; ++z) s += part[(size_t)z * MN + i];
  out[(i / N) * (size_t)ldo + (i % N)] = s;
}

// Column sums of a delta per 64-row block: part[blk][q][col], q = 0: sum Delta; with xyz4 also q = 1..3: sum Delta x / y / z. Rows in
// row order. grid = 64-row blocks, 256 threads: thread t owns columns t and t + 256.
DISTR_GLOBAL void __launch_bounds__(256) k_train_colsum(const float* __restrict__ D, int ldd, int ncols, const float* __restrict__ xyz4,
                                                      float* __restrict__ part) {
  __shared__ float p[TROW][4];
  const int blk = blockIdx.x, t = threadIdx.x;
  if (xyz4) {
    if (t < TROW) *(float4*)p[t] = *(const float4*)(xyz4 + ((size_t)blk * TROW + t) * 4);
    __syncthreads();
  }
  for (int h = 0; h < 2; ++h) {
    const int c = t + h * 256;
    if (c >= ncols) continue;
    float s = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
    const float* d = D + (size_t)blk * TROW * ldd + c;
    for (int r = 0; r < TROW; ++r) {
      const float v = d[(size_t)r * ldd];
      s += v;
      if (xyz4) { sx = __builtin_fmaf(v, p[r][0], sx); sy = __builtin_fmaf(v, p[r][1], sy); sz = __builtin_fmaf(v, p[r][2], sz); }
    }
    float* o = part + (size_t)blk * 4 * HID + c;
    o[0] = s;
    if (xyz4) { o[HID] = sx; o[2 * HID] = sy; o[3 * HID] = sz; }
  }
}

// Per segment: the block sums of its blocks. 8 lanes per column take every 8th block in block order, then an ordered tree over the 8.
// grid (segments, 16 column groups of 32, nq), 256 threads; seg[s][q][col]. blk0[s] / nblk from the counts.
DISTR_GLOBAL void __launch_bounds__(256) k_train_colsum_seg(const float* __restrict__ part, Segs sg, int ncols, float* __restrict__ seg) {
  __shared__ float lds[8][32];
  const int s = blockIdx.x, q = blockIdx.z;
  const int c = blockIdx.y * 32 + (threadIdx.x & 31), j = threadIdx.x >> 5;
  int b0 = 0;
  for (int i = 0; i < s; ++i) b0 += (sg.n[i] + TROW - 1) / TROW;
  const int nb = (sg.n[s] + TROW - 1) / TROW;
  float a = 0.f;
  if (c < ncols)
    for (int b = j; b < nb; b += 8) a += part[((size_t)(b0 + b) * 4 + q) * HID + c];
  lds[j][threadIdx.x & 31] = a;
  __syncthreads();
  if (j == 0 && c < ncols) {
    const int x = threadIdx.x;
    const float r = ((lds[0][x] + lds[1][x]) + (lds[2][x] + lds[3][x])) + ((lds[4][x] + lds[5][x]) + (lds[6][x] + lds[7][x]));
    seg[((size_t)s * 4 + q) * HID + c] = r;
  }
}

// From the per-segment sums seg[s][q][col] of layer l's delta, segments in order:
//   g_b[o] = sum_s seg[s][0][o]
//   with g_W (lin0 / lin4): g_W[o][xyz_col + d] = sum_s seg[s][1 + d][o], g_W[o][lat_col + c] = sum_s seg[s][0][o] code_s[c]
// grid = ncols outputs o, 256 threads over the C + 3 + 1 entries of the row.
DISTR_GLOBAL void __launch_bounds__(256) k_train_bias(const float* __restrict__ seg, int nseg, float* __restrict__ g_b, float* __restrict__ g_W, int ldw,
                                                    int lat_col, int xyz_col, int C, const float* __restrict__ latent, int64_t lat_stride) {
  const int o = blockIdx.x;
  const int nW = g_W ? C + 3 : 0;          // g_W == null: the bias only
  for (int e = threadIdx.x; e < nW + 1; e += 256) {
    float a = 0.f;
    if (e < nW - 3) {
      for (int s = 0; s < nseg; ++s) a = __builtin_fmaf(seg[((size_t)s * 4) * HID + o], latent[(int64_t)s * lat_stride + e], a);
      g_W[(size_t)o * ldw + lat_col + e] = a;
    } else if (e < nW) {
      const int d = e - C;
      for (int s = 0; s < nseg; ++s) a += seg[((size_t)s * 4 + 1 + d) * HID + o];
      g_W[(size_t)o * ldw + xyz_col + d] = a;
    } else {
      for (int s = 0; s < nseg; ++s) a += seg[((size_t)s * 4) * HID + o];
      g_b[o] = a;
    }
  }
}

// g_latent[s][c] = sum_o W0[o][c] seg0[s][0][o] + sum_o W4[o][col4 + c] seg4[s][0][o], o in order, lin0's chain then lin4's. W0's row
// stride is C + 3, W4's is ld4 (the SDF decoder: ld4 = 512, col4 = 509 - C). grid (ceil(C / 256), segments)
DISTR_GLOBAL void __launch_bounds__(256) k_train_glatent(const float* __restrict__ seg0, const float* __restrict__ seg4, const float* __restrict__ W0,
                                                       const float* __restrict__ W4, int C, int ld4, int col4, float* __restrict__ g_latent) {
  const int c = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (c >= C) return;
  const float* s0 = seg0 + (size_t)s * 4 * HID;
  const float* s4 = seg4 + (size_t)s * 4 * HID;
  float a = 0.f;
  for (int o = 0; o < HID; ++o) a = __builtin_fmaf(W0[(size_t)o * (C + 3) + c], s0[o], a);
  for (int o = 0; o < HID; ++o) a = __builtin_fmaf(W4[(size_t)o * ld4 + col4 + c], s4[o], a);
  g_latent[(size_t)s * C + c] = a;
}

// ---- the spatial gradient g = grad_x f and its weight gradients (include/distr_train.h).
// Unit deltas Delta_l = d z / d (lin_l's output): the EPI_GATE chain from Delta_8 = 1 (0 on a padded row). Tangents tau_l = d in_l along
// the upstream u = dL/dg: the EPI_TAN chain from tau_0 = [0 | u].

// Delta_8: one[row] = 1 for a real row, 0 for a padded one
DISTR_GLOBAL void __launch_bounds__(256) k_train_unit(const int32_t* __restrict__ rowpt, int rows, float* __restrict__ one) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row < rows) one[row] = rowpt[row] >= 0 ? 1.f : 0.f;
}

// g[pt][d] = (1 - f^2) (sum_o W0[o][C + d] Delta_0[row][o] + sum_o W4[o][ld4 - 3 + d] Delta_4[row][o]): one fmaf chain per (row, d), o in
// natural order, lin0's chain then lin4's (the order of k_train_glatent). block = one 64-row block, 256 threads: thread t owns row
// t & 63 and component t >> 6 (the fourth wave only stages); the deltas pass through LDS in tiles of 64 rows x 64 units.
DISTR_GLOBAL void __launch_bounds__(256) k_train_gx(const float* __restrict__ D0, const float* __restrict__ D4, const float* __restrict__ W0,
                                                  const float* __restrict__ W4, int C, int ld4, const float* __restrict__ th,
                                                  const int32_t* __restrict__ rowpt, float* __restrict__ grad) {
  __shared__ float ds[TROW][TROW + 1];
  __shared__ float ws[TROW][4];
  const int blk = blockIdx.x, t = threadIdx.x, r = t & (TROW - 1), d = t >> 6;
  float acc = 0.f;
  for (int half = 0; half < 2; ++half) {
    const float* D = half ? D4 : D0;
    const float* W = half ? W4 + (ld4 - 3) : W0 + C;
    const int ldw = half ? ld4 : C + 3;
    for (int o0 = 0; o0 < HID; o0 += TROW) {
      for (int e = t; e < TROW * TROW; e += 256) ds[e >> 6][e & 63] = D[((size_t)blk * TROW + (e >> 6)) * HID + o0 + (e & 63)];
      if (t < TROW * 3) ws[t / 3][t % 3] = W[(size_t)(o0 + t / 3) * ldw + t % 3];
      __syncthreads();
      if (d < 3)
        for (int o = 0; o < TROW; ++o) acc = __builtin_fmaf(ws[o][d], ds[r][o], acc);
      __syncthreads();
    }
  }
  if (d < 3) {
    const int row = blk * TROW + r, pt = rowpt[row];
    if (pt >= 0) {
      const float f = th[row];
      grad[(size_t)pt * 3 + d] = (1.f - f * f) * acc;
    }
  }
}

// lin0's tangent: T1[row] = G_0 (W0[:, C:] u[row]) with G_0 = scale [X1 > 0] (scale = 1 without dropout), and the padded upstream
// u4[row] = (u, 0), zero for a padded row and for g_grad == null. The thread layout of lin0_block.
DISTR_GLOBAL void __launch_bounds__(256) k_train_tan0(const float* __restrict__ g_grad, const int32_t* __restrict__ rowpt, const float* __restrict__ W0, int C,
                                                    const float* __restrict__ X1, float scale, float* __restrict__ T1, float* __restrict__ u4) {
  __shared__ float p[TROW][4];
  const int blk = blockIdx.x, t = threadIdx.x;
  if (t < TROW) {
    const int pt = rowpt[blk * TROW + t];
    float x = 0.f, y = 0.f, z = 0.f;
    if (pt >= 0 && g_grad) { x = g_grad[(size_t)pt * 3]; y = g_grad[(size_t)pt * 3 + 1]; z = g_grad[(size_t)pt * 3 + 2]; }
    p[t][0] = x; p[t][1] = y; p[t][2] = z; p[t][3] = 0.f;
    float* q = u4 + ((size_t)blk * TROW + t) * 4;
    q[0] = x; q[1] = y; q[2] = z; q[3] = 0.f;
  }
  __syncthreads();
  for (int h = 0; h < 2; ++h) {
    const int o = t + h * 256;
    const float* w = W0 + (size_t)o * (C + 3) + C;
    const float wx = w[0], wy = w[1], wz = w[2];
    for (int r = 0; r < TROW; ++r) {
      const size_t i = ((size_t)blk * TROW + r) * HID + o;
      float a = wx * p[r][0];
      a = __builtin_fmaf(wy, p[r][1], a);
      a = __builtin_fmaf(wz, p[r][2], a);
      T1[i] = X1[i] > 0.f ? a * scale : 0.f;
    }
  }
}

// The row scalars of the backward: f = th, t' = 1 - f^2, c1 = t', c2 = t' (phi - 2 f Q) with phi = g_sdf[pt] (null: 0) and Q = W8 tau_8;
// rw[row] = (c2 x + c1 u_x, c2 y + c1 u_y, c2 z + c1 u_z, c2), the weights of k_train_colsum_w; one[row] = Delta_8. All 0 on a padded row.
DISTR_GLOBAL void __launch_bounds__(256) k_train_rowscal(const float* __restrict__ g_sdf, const float* __restrict__ th, const float* __restrict__ Q,
                                                       const int32_t* __restrict__ rowpt, const float* __restrict__ xyz4, const float* __restrict__ u4, int rows,
                                                       float* __restrict__ c1, float* __restrict__ c2, float* __restrict__ rw, float* __restrict__ one) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const int pt = rowpt[row];
  float a1 = 0.f, a2 = 0.f;
  if (pt >= 0) {
    const float f = th[row], phi = g_sdf ? g_sdf[pt] : 0.f;
    a1 = 1.f - f * f;
    a2 = a1 * (phi - 2.f * f * Q[row]);
  }
  c1[row] = a1; c2[row] = a2; one[row] = pt >= 0 ? 1.f : 0.f;
  const float4 x = *(const float4*)(xyz4 + (size_t)row * 4), u = *(const float4*)(u4 + (size_t)row * 4);
  *(float4*)(rw + (size_t)row * 4) = make_float4(__builtin_fmaf(a2, x.x, a1 * u.x), __builtin_fmaf(a2, x.y, a1 * u.y), __builtin_fmaf(a2, x.z, a1 * u.z), a2);
}

// The combined operand of a weight gradient, in place: T[row][c] = c2[row] X[row][c] + c1[row] T[row][c] for c < ncols (rows of 512
// floats; ncols = lin3's rows for X_4, whose other columns are not written). One thread per quad of columns.
DISTR_GLOBAL void __launch_bounds__(256) k_train_combine(const float* __restrict__ X, const float* __restrict__ c1, const float* __restrict__ c2, int rows, int ncols,
                                                       float* __restrict__ T) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)rows * (HID / 4)) return;
  const int row = (int)(i / (HID / 4)), c = (int)(i % (HID / 4)) * 4;
  if (c >= ncols) return;
  const float a1 = c1[row], a2 = c2[row];
  const size_t at = (size_t)row * HID + c;
  const float4 x = *(const float4*)(X + at);
  float4 v = *(const float4*)(T + at);
  v.x = __builtin_fmaf(a2, x.x, a1 * v.x); v.y = __builtin_fmaf(a2, x.y, a1 * v.y);
  v.z = __builtin_fmaf(a2, x.z, a1 * v.z); v.w = __builtin_fmaf(a2, x.w, a1 * v.w);
  if (c + 3 < ncols) *(float4*)(T + at) = v;
  else {
    T[at] = v.x;
    if (c + 1 < ncols) T[at + 1] = v.y;
    if (c + 2 < ncols) T[at + 2] = v.z;
  }
}

// k_train_colsum with a weight per row: part[blk][q][col] = sum_r D[r][col] rw[r][q == 0 ? 3 : q - 1], rows in row order; q = 0 (sum
// c2 Delta: the bias, the latent columns, the code gradient) always, q = 1..3 (the xyz columns of g_W0 / g_W4) with `moments`.
DISTR_GLOBAL void __launch_bounds__(256) k_train_colsum_w(const float* __restrict__ D, int ldd, int ncols, const float* __restrict__ rw, int moments,
                                                        float* __restrict__ part) {
  __shared__ float p[TROW][4];
  const int blk = blockIdx.x, t = threadIdx.x;
  if (t < TROW) *(float4*)p[t] = *(const float4*)(rw + ((size_t)blk * TROW + t) * 4);
  __syncthreads();
  for (int h = 0; h < 2; ++h) {
    const int c = t + h * 256;
    if (c >= ncols) continue;
    float s = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
    const float* d = D + (size_t)blk * TROW * ldd + c;
    for (int r = 0; r < TROW; ++r) {
      const float v = d[(size_t)r * ldd];
      s = __builtin_fmaf(v, p[r][3], s);
      if (moments) { sx = __builtin_fmaf(v, p[r][0], sx); sy = __builtin_fmaf(v, p[r][1], sy); sz = __builtin_fmaf(v, p[r][2], sz); }
    }
    float* o = part + (size_t)blk * 4 * HID + c;
    o[0] = s;
    if (moments) { o[HID] = sx; o[2 * HID] = sy; o[3 * HID] = sz; }
  }
}

}  // namespace train
}  // namespace distr
