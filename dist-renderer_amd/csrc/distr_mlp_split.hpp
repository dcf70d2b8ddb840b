// distr_mlp_split.hpp -- the DeepSDF 8x512 decoder tile in SPLIT arithmetic (opt-in), forward and backward: ONE chain, two number formats.
//
// The default decoder tile (distr_mlp.hpp) computes every dense layer with f32-input MFMAs: exact f32, bit-identical to the
// oracle's k-ordered fmaf chains, at 1/16 of the 16-bit MFMA rate. This tile evaluates the same network (Decoder.inference,
// core/graph/deep_sdf_decoder.py:80-111) with every f32 product W x replaced by a few products of 16-bit PLANES, accumulated in f32.
// What a plane is, how many there are and which products are formed is a FORMAT (FmtB6, FmtH3 below); everything else -- tile
// geometry, k-loop, layer sequence, mask format, backward walk -- is written once and parameterised by the format type.
// Neither format is bit-identical to the oracle (different summation order inside the MFMA), so they never replace the exact path
// silently: callers ask for them (distr_render_cfg.arith, distr_mlp_eval_bf16x6 / _f16x3; bulk SDF grids for meshing,
// core/evaluation/create_mesh.py, where marching cubes is indifferent to 1e-6). Measured: see profiles/.
//
// Data flow of a 64-ray tile (one workgroup = 4 waves):
//   * activations live in LDS (128 KiB in either format), k-MINOR: [k >> 3][ray][k & 7], so the 8 k-values a lane feeds to one
//     16-bit MFMA are contiguous; the format decides whether they are f32 values split by every consumer or planes split once by
//     the producer (Fmt::Act);
//   * weights: pre-split planes per layer, pre-packed on the host as A fragments of v_mfma_f32_32x32x16_{bf16,f16}
//     (fragment index (((kb * 4 + wave) * NOB + ob) * NP + plane) * 64 + lane = 8 values W_plane[o][16 kb + 8 h + 0..7]);
//   * wave w owns output rows [w O/4, (w+1) O/4) as NOB x 2 accumulator tiles of 32 x 32, started from the bias (exact f32);
//   * lin0 (K = 3) and lin8 (one row) are plain f32 VALU work, as in the exact tile;
//   * march tiles: the same forward inside k_march / k_step when distr_render_cfg.arith asks for it, on 64- and 32-ray tiles only
//     (no 16-ray / cluster tiles: they are built on the f32 16x16x4 MFMA and would not be bit-identical to these);
//   * backward (split_backward): the dX chain on the saved ReLU masks with the transposed weight planes, same loop.
#pragma once
#include "distr_mlp.hpp"

namespace distr {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

struct DecoderSplit {
  const uint32_t* Wp[8];   // A-fragment planes of lin1..lin7 in one format ([0] unused); lin3: O padded to 256; lin4: K = 256
  const uint32_t* Wb[8];   // the same for the TRANSPOSED matrices (backward dX chain), index = layer whose weights are used (1..7)
};

template <int TILE>
__device__ __forceinline__ int xk(int k, int ray) { return ((k >> 3) * TILE + ray) * 8 + (k & 7); }

// ---------------------------------------------------------------------------------------- format: six bf16 products
//     W = w0 + w1 + w2,  x = a0 + a1 + a2   (bf16 planes, round to nearest even of the running remainder)
//     W x ~ w0 a0 + w1 a0 + w0 a1 + w1 a1 + w2 a0 + w0 a2
// on v_mfma_f32_32x32x16_bf16: both operands keep 24 significant bits, the dropped terms are below 2^-24 relative, and one layer's
// error against a float64 product is no larger than the f32 chain's own (profiles/r03_split_bf16_layer.md: 1.4e-7 vs 2.0e-7).
// Activations stay f32 in LDS (three bf16 planes of 512 x 64 would need 192 KiB); they are split into the three planes in registers
// while the next block's fragments load (VALU that hides in the gaps of bf16 MFMAs, unlike next to f32 MFMAs). No scales, no range
// to watch: bf16 has the exponent of f32.
__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {   // {bf16(a) low half, bf16(b) high half}, round to nearest even
  typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
  const f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf2));      // v_cvt_pk_bf16_f32
}
__device__ __forceinline__ void split_pair(float a, float b, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
  p0 = pk_bf16(a, b);
  const float ra = a - __uint_as_float(p0 << 16), rb = b - __uint_as_float(p0 & 0xffff0000u);
  p1 = pk_bf16(ra, rb);
  const float sa = ra - __uint_as_float(p1 << 16), sb = rb - __uint_as_float(p1 & 0xffff0000u);
  p2 = pk_bf16(sa, sb);
}

struct FmtB6 {
  static constexpr int NP = 3, NQ = 6;
  static constexpr int PW[6] = {0, 1, 0, 1, 2, 0}, PA[6] = {0, 0, 1, 1, 0, 2};     // (weight plane, activation plane) of the six products
  static constexpr bool SCALED = false, RANGE = false, NORMALISED = false;
  static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
  template <int RB> struct Ahead { f32x4 x[RB][2]; };       // the next block's f32 activations, split between this block's MFMAs
  template <int RB> struct Carry { u32x4 a[4][3]; };        // registers that travel through the forward chain: the next weight block
  template <int RB>
  struct Act {
    static constexpr int TILE = 32 * RB;
    float X[HID * TILE];
    __device__ __forceinline__ void load_ahead(int kb, int lane, Ahead<RB>& n, u32x4 (&)[RB][3]) const {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const f32x4* xp = reinterpret_cast<const f32x4*>(&X[xk<TILE>(16 * kb + 8 * (lane >> 5), 32 * rb + (lane & 31))]);
        n.x[rb][0] = xp[0]; n.x[rb][1] = xp[1];
      }
    }
    __device__ __forceinline__ void store4(int row, int ray, f32x4 v) { *reinterpret_cast<f32x4*>(&X[xk<TILE>(row, ray)]) = v; }
    __device__ __forceinline__ void store1(int row, int ray, float v) { X[xk<TILE>(row, ray)] = v; }
    __device__ __forceinline__ float read(int row, int ray) const { return X[xk<TILE>(row, ray)]; }
  };
  template <int RB>
  static __device__ __forceinline__ void split_ahead(const Ahead<RB>& n, u32x4 (&dst)[RB][3]) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      uint32_t q0[4], q1[4], q2[4];
      split_pair(n.x[rb][0][0], n.x[rb][0][1], q0[0], q1[0], q2[0]);
      split_pair(n.x[rb][0][2], n.x[rb][0][3], q0[1], q1[1], q2[1]);
      split_pair(n.x[rb][1][0], n.x[rb][1][1], q0[2], q1[2], q2[2]);
      split_pair(n.x[rb][1][2], n.x[rb][1][3], q0[3], q1[3], q2[3]);
#pragma unroll
      for (int i = 0; i < 4; ++i) { dst[rb][0][i] = q0[i]; dst[rb][1][i] = q1[i]; dst[rb][2][i] = q2[i]; }
    }
  }
};

// ---------------------------------------------------------------------------------------- format: three f16 products
//     SW W = w0 + w1,  SX x = a0 + a1   (f16 planes of the SCALED operands, round to nearest even of the running remainder)
//     W x ~ (w0 a0 + w1 a0 + w0 a1) / (SW SX)             on v_mfma_f32_32x32x16_f16, f32 accumulation
// An f16 plane carries 11 significant bits, two planes 22, and the dropped product w1 a1 is 2^-22 of w0 a0 -- the size of the f32
// chain's own rounding. Measured on both fixture decoders (oracle/study_split_bf16.py, CPU restatement, 20 000 points against a
// float64 decoder): max |sdf - sdf_f64| 3.5e-7 for this form, 3.0e-7 for the exact f32 chain, 3.0e-7 for six bf16 products, 7.9e-6
// for three bf16 products. Three MFMAs per f32 product instead of six, and -- because two f16 planes of a 512 x 64 activation tile
// are 128 KiB, the size of the f32 tile -- the planes themselves live in LDS: the split is done ONCE by the wave that produces a
// value (write-back), not by each of the four waves that consume it, and the k-loop has no VALU work at all. The weight stream is
// two f16 planes = the bytes of f32 (the bf16 form streams 1.5 x). profiles/ubench/split_f16_layer.hip: 34.3 k cycles per
// 512 x 512 layer on a 64-ray tile (bf16x6 66.4 k, exact f32 133.7 k).
//
// What f16 costs is RANGE (5 exponent bits), on both sides. Above: a scaled operand beyond 65504 becomes inf. SX = SW = 64 allows
// |x|, |W| < 1023.5 (H3_WMAX); an activation that overflows turns the evaluation's result non-finite, which the tiles COUNT
// (Consts.f16_overflow -> distr_render_stats.f16_overflows; distr_mlp_eval_f16x3 writes NaN for the point) instead of hiding it
// behind the clamps of the march. Below: the second plane of a value x holds SX x's bits 12..22; once it falls under 2^-14 it is an
// f16 denormal (the conversions and the MFMA keep them: measured, tests/test_gpu_split_arith.py) with a fixed spacing of 2^-24,
// so a layer whose activations are small loses accuracy and NOTHING is counted. SX = 64 keeps the second planes of this network's
// magnitudes (activations 1e-3 .. 1, weights ~ 0.05) above that. Measured on function-preserving rescales of fixture F1 (one
// layer's weights times 2^-k, the next layer's times 2^k; or lin1 times 2^-k and lin7 times 2^k), max |sdf - sdf_f64| relative
// to the exact f32 kernel's on the same 8 193 points: 1.3 at k = 6 (smallest layer maximum 4.5e-3), 2.5 at k = 7 (2.3e-3),
// 3.2 at k = 8, 13.5 at k = 10. distr_set_decoder therefore accepts the mode only when every layer's
// largest |weight| lies in [H3_WMIN, H3_WMAX); otherwise the calls that ask for the mode fail and name the layer. This is a rule on
// WEIGHTS: it cannot prove that activations stay large enough (a decoder whose small activations come from its inputs or biases
// passes it); it was checked on the two rescale families above and on both fixtures.
// The backward of a render in this mode is the dX chain on the ReLU masks the forward saved, in the same arithmetic, on deltas
// NORMALISED per ray by the loss gradient (whose range has no bound; see split_backward), with transposed weight planes.

// {f16(a) low half, f16(b) high half} of the value and of its remainder (v_cvt_pk_f16_f32, v_cvt_f32_f16, v_sub_f32)
__device__ __forceinline__ void split2_f16(float a, float b, uint32_t& p0, uint32_t& p1) {
  const f32x2 v = {a, b};
  const f16x2 h0 = __builtin_convertvector(v, f16x2);
  const f32x2 r = v - __builtin_convertvector(h0, f32x2);
  const f16x2 h1 = __builtin_convertvector(r, f16x2);
  p0 = __builtin_bit_cast(uint32_t, h0);
  p1 = __builtin_bit_cast(uint32_t, h1);
}
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

struct FmtH3 {
  static constexpr int NP = 2, NQ = 3;
  static constexpr int PW[3] = {0, 1, 0}, PA[3] = {0, 0, 1};     // (weight plane, activation plane) of the three products
  static constexpr bool SCALED = true, RANGE = true, NORMALISED = true;
  static constexpr float SX = 64.f, SW = 64.f;      // powers of two: every rescale is exact
  static constexpr float BIAS = SW * SX;            // the accumulators are in units of SW SX ...
  static constexpr float BACK = 1.0f / SW;          // ... and go back to LDS in units of SX (forward) or SD (backward)
  static constexpr float SD = 1024.f;               // scale of the backward's per-ray normalised deltas (|delta / d8| < 64)
  static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  template <int RB> struct Ahead {};                // nothing to split in the k-loop: the planes themselves are loaded ahead
  // Range check of the forward: every lane keeps, per block of 32 rays, the largest leading-plane bit pattern it wrote (v_pk_max_u16;
  // non-negative f16 order like unsigned integers, inf = 0x7c00 and NaN above it): one instruction per pair of values.
  template <int RB> struct Carry { u32x4 a[4][2]; uint32_t top[RB]; };
  static __device__ __forceinline__ bool top_overflowed(uint32_t top) { return (top & 0xffffu) >= 0x7c00u || (top >> 16) >= 0x7c00u; }
  template <int RB>
  struct Act {
    static constexpr int TILE = 32 * RB;
    uint16_t P[2][HID * TILE];   // the two f16 planes of the scaled value
    __device__ __forceinline__ void load_ahead(int kb, int lane, Ahead<RB>&, u32x4 (&b)[RB][2]) const {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int p = 0; p < 2; ++p) b[rb][p] = *reinterpret_cast<const u32x4*>(&P[p][xk<TILE>(16 * kb + 8 * (lane >> 5), 32 * rb + (lane & 31))]);
    }
    // four consecutive features of one ray -> one 8-byte store per plane; top (ReLU outputs only, >= 0): the range check above
    __device__ __forceinline__ void store4(int row, int ray, f32x4 v, uint32_t* top = nullptr) {
      u32x2 p0, p1;
      uint32_t t0, t1;
      split2_f16(v[0], v[1], t0, t1); p0[0] = t0; p1[0] = t1; if (top) *top = pk_max_u16(*top, t0);
      split2_f16(v[2], v[3], t0, t1); p0[1] = t0; p1[1] = t1; if (top) *top = pk_max_u16(*top, t0);
      *reinterpret_cast<u32x2*>(&P[0][xk<TILE>(row, ray)]) = p0;
      *reinterpret_cast<u32x2*>(&P[1][xk<TILE>(row, ray)]) = p1;
    }
    __device__ __forceinline__ void store1(int row, int ray, float v) {     // (scalar conversions, not the packed pair)
      const _Float16 h0 = (_Float16)v;
      const _Float16 h1 = (_Float16)(v - (float)h0);
      P[0][xk<TILE>(row, ray)] = __builtin_bit_cast(uint16_t, h0);
      P[1][xk<TILE>(row, ray)] = __builtin_bit_cast(uint16_t, h1);
    }
    __device__ __forceinline__ float read(int row, int ray) const {         // (the sum of the planes is exact in f32)
      const int i = xk<TILE>(row, ray);
      return (float)__builtin_bit_cast(_Float16, P[0][i]) + (float)__builtin_bit_cast(_Float16, P[1][i]);
    }
  };
  template <int RB>
  static __device__ __forceinline__ void split_ahead(const Ahead<RB>&, u32x4 (&)[RB][2]) {}
};

constexpr float H3_WMAX = 65504.f / FmtH3::SW;   // a layer's largest |weight| must stay below this (1023 passes, 1024 does not) ...
constexpr float H3_WMIN = 0.00390625f;           // ... and reach this (2^-8: between the measured 4.5e-3, inside 2 x the f32 error, and 2.3e-3, outside)

template <int ARITH> struct SplitFmtOf;           // ARITH = DISTR_ARITH_* of distr_render_cfg.arith
template <> struct SplitFmtOf<1> { using type = FmtB6; };
template <> struct SplitFmtOf<2> { using type = FmtH3; };
template <int ARITH> using SplitFmt = typename SplitFmtOf<ARITH>::type;

// A tile = RB blocks of 32 rays (RB = 2: 64 rays, RB = 1: 32 rays). Every output column of v_mfma_f32_32x32x16_* depends only
// on its own B column, so a ray's value does not depend on RB or on which other rays share its tile: the two tile sizes are
// bit-identical (within one arithmetic), like the tile sizes of the exact path are among themselves.
template <class Fmt, int RB>
struct alignas(16) SmemSplit {
  static constexpr int TILE = 32 * RB;
  typename Fmt::template Act<RB> act;   // k-minor activations
  float xyz[4 * TILE];     // (normalised backward: row 0 = d8 / SD)
  float part[12 * TILE];   // lin8 partial chains [4][TILE], range flags [TILE] behind them; backward: xyz-gradient partials [3][4][TILE], mask-block indices
  float aux[4 * TILE];     // march tiles (KEEP): the rays' mask-block indices (8 bytes each); backward: row 0 = d8, rows 1..3 = d/dxyz
};
static_assert(sizeof(SmemSplit<FmtH3, 2>) == sizeof(SmemSplit<FmtB6, 2>) && sizeof(SmemSplit<FmtH3, 1>) == sizeof(SmemSplit<FmtB6, 1>), "the tiles share k_step's role buffer");

// weight fragments of one 16-feature block: NP planes x NOB row blocks, one 16-byte load each (buffers are sized for NOB = 4)
template <class Fmt, int NOB>
__device__ __forceinline__ void split_load_a(const uint32_t* __restrict__ Wp, int kb, int wave, int lane, u32x4 (&dst)[4][Fmt::NP]) {
  constexpr int NP = Fmt::NP;
  const u32x4* wp = reinterpret_cast<const u32x4*>(Wp) + (size_t)wave * NOB * NP * 64 + lane;
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
    for (int p = 0; p < NP; ++p) dst[ob][p] = wp[(((size_t)kb * 4 * NOB + ob) * NP + p) * 64];
}

// acc[ob][rb] (started by the caller, in the format's units) += W[rows of this wave][0..K) x X[0..K)[rays], NQ products of planes per
// f32 product. Register double buffer: block kb + 1 (weights from L2, activations from LDS) is requested before the MFMAs of block
// kb; a format that splits in registers does so right after the first group of those MFMAs (one wave per SIMD: nothing else hides
// the L2 round trip), the other has nothing but loads and MFMAs in the loop.
// On entry `a` holds this layer's block 0 -- requested by the previous layer during ITS last block -- and the look-ahead slot of
// the last block requests block 0 of the NEXT layer (WpNext, NOBN row blocks per wave; null: nothing), returned in `a`: no layer
// begins with an exposed round trip (the same arrangement as dense_pf of the exact tile). (A three-deep ring, two blocks ahead,
// was tried. bf16x6: the compiler needs > 512 registers for it and spills inside the loop. f16x3: worth 13 % in the microbenchmark
// and 4.5 % in distr_mlp_eval_f16x3, but puts 380 bytes of k_step's state into scratch and leaves the march unchanged: not used.)
template <class Fmt, int K, int NOB, int RB, int NOBN>
__device__ __forceinline__ void split_dense(const uint32_t* __restrict__ Wp, const uint32_t* __restrict__ WpNext, const typename Fmt::template Act<RB>& X,
                                            f32x16 (&acc)[NOB][RB], int wave, int lane, u32x4 (&a)[4][Fmt::NP]) {
  constexpr int NKB = K / 16, NP = Fmt::NP;
  u32x4 b[RB][NP];
  {
    typename Fmt::template Ahead<RB> x0;
    X.load_ahead(0, lane, x0, b);
    Fmt::split_ahead(x0, b);
  }
#pragma unroll 2
  for (int kb = 0; kb < NKB; ++kb) {
    u32x4 an[4][NP], bn[RB][NP];
    typename Fmt::template Ahead<RB> xn;
    const bool last = (kb + 1 == NKB);
    if (!last) split_load_a<Fmt, NOB>(Wp, kb + 1, wave, lane, an);
    else if (WpNext) split_load_a<Fmt, NOBN>(WpNext, 0, wave, lane, an);
    X.load_ahead(last ? kb : kb + 1, lane, xn, bn);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < Fmt::NQ; ++q) {
#pragma unroll
      for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) acc[ob][rb] = Fmt::mfma(a[ob][Fmt::PW[q]], b[rb][Fmt::PA[q]], acc[ob][rb]);
      if (q == 0) Fmt::split_ahead(xn, bn);
    }
#pragma unroll
    for (int ob = 0; ob < 4; ++ob)
#pragma unroll
      for (int p = 0; p < NP; ++p) a[ob][p] = an[ob][p];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int p = 0; p < NP; ++p) b[rb][p] = bn[rb][p];
  }
}

// Four consecutive ReLU outputs of ray 32 rb + j, with the format's range tracking
template <class Fmt, int RB>
__device__ __forceinline__ void split_store_relu(typename Fmt::template Act<RB>& X, int row, int rb, int j, f32x4 v, typename Fmt::template Carry<RB>& c) {
  if constexpr (Fmt::RANGE) X.store4(row, 32 * rb + j, v, &c.top[rb]);
  else X.store4(row, 32 * rb + j, v);
}

// ReLU, rescale to the activations' units, write-back into the k-minor layout: D rows of register r on lane (j, h) are
// (r & 3) + 8 (r >> 2) + 4 h -> 4 consecutive features = one store4. KEEP: bit (rb * 16 + r) of mask[ob] = value > 0 -- the format of
// the exact tile's write-back (distr_mlp.hpp::writeback; the C/D layout of the 16-bit MFMAs is that of v_mfma_f32_32x32x2_f32), so
// the saved mask blocks feed the same backward kernel.
template <class Fmt, int NOB, int RB, bool KEEP>
__device__ __forceinline__ void split_writeback(typename Fmt::template Act<RB>& X, const f32x16 (&acc)[NOB][RB], int row0, int lane, uint32_t (&mask)[4],
                                                typename Fmt::template Carry<RB>& c) {
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob) {
    uint32_t m = 0u;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int32_t rbits = max(__float_as_int(acc[ob][rb][4 * q + i]), 0);
          v[i] = __int_as_float(rbits);
          if constexpr (Fmt::SCALED) v[i] *= Fmt::BACK;
          if (KEEP) m |= min((uint32_t)rbits, 1u) << (rb * 16 + 4 * q + i);
        }
        split_store_relu<Fmt, RB>(X, row0 + 32 * ob + 8 * q + 4 * h, rb, j, v, c);
      }
    if (KEEP) {
      asm volatile("" : "+v"(m));      // (see distr_mlp.hpp::writeback: keeps LLVM from carrying the accumulators instead of the bits)
      mask[ob] = m;
    }
  }
}

// One wide layer; c.a = its first weight block on entry, the next layer's first block on return (see split_dense)
template <class Fmt, int K, int NOB, int RB, bool KEEP, int NOBN>
__device__ __forceinline__ void split_layer(const uint32_t* __restrict__ Wp, const uint32_t* __restrict__ WpNext, const float* __restrict__ bias, int nbias,
                                            typename Fmt::template Act<RB>& X, int wave, int lane, uint32_t (&mask)[4], typename Fmt::template Carry<RB>& c) {
  const int h = lane >> 5;
  f32x16 acc[NOB][RB];
  const int row0 = wave * 32 * NOB;
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + 32 * ob + (r & 3) + 8 * (r >> 2) + 4 * h;
      float bv = 0.f;
      if (row < nbias) {
        if constexpr (Fmt::SCALED) bv = bias[row] * Fmt::BIAS;
        else bv = bias[row];
      }
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) acc[ob][rb][r] = bv;
    }
  split_dense<Fmt, K, NOB, RB, NOBN>(Wp, WpNext, X, acc, wave, lane, c.a);
  __syncthreads();                         // everybody is done reading the layer input
  split_writeback<Fmt, NOB, RB, KEEP>(X, acc, row0, lane, mask, c);
  __syncthreads();
}

// Preconditions as mlp_forward: S.xyz rows 0..2 hold the TILE points. Returns (every thread, ray = tid & (TILE - 1)) the pre-tanh
// output; masks[l] = ReLU bitmasks of layer l in the exact tile's format (KEEP).
// Fmt::RANGE: a ray with an activation at or beyond the format's range (inf / NaN pattern in c.top) gets NaN as its result -- which
// the callers test -- whatever the later layers made of the inf (a ReLU taken on the bit pattern turns a negative NaN into 0).
template <class Fmt, int RB, bool KEEP>
__device__ __forceinline__ float split_forward(const DecoderDev& D, const DecoderSplit& P, const float* __restrict__ c0, const float* __restrict__ c4,
                                               SmemSplit<Fmt, RB>& S, uint32_t (&masks)[8][4]) {
  constexpr int TILE = 32 * RB;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int j = lane & 31, h = lane >> 5;
  auto& X = S.act;
  typename Fmt::template Carry<RB> c;      // c.a: first weight block of the next layer, travelling across the write-backs
  uint32_t* over = reinterpret_cast<uint32_t*>(S.part + 4 * TILE);      // Fmt::RANGE: [TILE] per-ray flags
  if constexpr (Fmt::RANGE) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) c.top[rb] = 0u;
    if (tid < TILE) over[tid] = 0u;
  }
  // lin0 (K = 3): the f32 fmaf chain of the exact tile (bias, then x, y, z), computed in the accumulator layout of the wide layers
  // (lane (j, h), register r <-> row, column) so that its ReLU bits land in the common mask format
  {
    float px[RB], py[RB], pz[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) { px[rb] = S.xyz[32 * rb + j]; py[rb] = S.xyz[TILE + 32 * rb + j]; pz[rb] = S.xyz[2 * TILE + 32 * rb + j]; }
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) {
      uint32_t m = 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 v[RB];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = wave * 128 + 32 * ob + 8 * q + 4 * h + i;
          const float b0 = c0[row], wx = D.W0x[row], wy = D.W0x[HID + row], wz = D.W0x[2 * HID + row];
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) {
            float t = __builtin_fmaf(wx, px[rb], b0);
            t = __builtin_fmaf(wy, py[rb], t);
            t = __builtin_fmaf(wz, pz[rb], t);
            const int32_t rbits = max(__float_as_int(t), 0);
            v[rb][i] = __int_as_float(rbits);
            if constexpr (Fmt::SCALED) v[rb][i] *= Fmt::SX;
            if (KEEP) m |= min((uint32_t)rbits, 1u) << (rb * 16 + 4 * q + i);
          }
        }
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) split_store_relu<Fmt, RB>(X, wave * 128 + 32 * ob + 8 * q + 4 * h, rb, j, v[rb], c);
      }
      if (KEEP) {
        asm volatile("" : "+v"(m));      // (opaque, like split_writeback: otherwise LLVM keeps lin0's 128 raw values alive instead of the 4 words)
        masks[0][ob] = m;
      }
    }
  }
  __syncthreads();
  split_load_a<Fmt, 4>(P.Wp[1], 0, wave, lane, c.a);
  split_layer<Fmt, 512, 4, RB, KEEP, 4>(P.Wp[1], P.Wp[2], D.bias[1], HID, X, wave, lane, masks[1], c);
  split_layer<Fmt, 512, 4, RB, KEEP, 2>(P.Wp[2], P.Wp[3], D.bias[2], HID, X, wave, lane, masks[2], c);
  masks[3][2] = 0; masks[3][3] = 0;
  split_layer<Fmt, 512, 2, RB, KEEP, 4>(P.Wp[3], P.Wp[4], D.bias[3], 253, X, wave, lane, masks[3], c);      // lin3: 512 -> 253 (+ 3 rows that carry xyz into lin4)
  if (tid < 3 * TILE) {                    // rows 253..255 <- xyz (signed)
    if constexpr (Fmt::SCALED) X.store1(253 + tid / TILE, tid % TILE, S.xyz[tid] * Fmt::SX);
    else X.store1(253 + tid / TILE, tid % TILE, S.xyz[tid]);
  }
  __syncthreads();
  split_layer<Fmt, 256, 4, RB, KEEP, 4>(P.Wp[4], P.Wp[5], c4, HID, X, wave, lane, masks[4], c);             // lin4: [x3 (253) | xyz (3)] -> 512, latent part folded into c4
  split_layer<Fmt, 512, 4, RB, KEEP, 4>(P.Wp[5], P.Wp[6], D.bias[5], HID, X, wave, lane, masks[5], c);
  split_layer<Fmt, 512, 4, RB, KEEP, 4>(P.Wp[6], P.Wp[7], D.bias[6], HID, X, wave, lane, masks[6], c);
  split_layer<Fmt, 512, 4, RB, KEEP, 4>(P.Wp[7], nullptr, D.bias[7], HID, X, wave, lane, masks[7], c);
  // lin8: four 128-long f32 chains per ray (one per wave) on x7, combined in the exact tile's order
  const int ray = tid & (TILE - 1);
  {
    float p = 0.f;
    const float* w8 = D.w8 + wave * 128;
#pragma unroll 8
    for (int k = 0; k < 128; ++k) {
      float x = X.read(wave * 128 + k, ray);
      if constexpr (Fmt::SCALED) x *= 1.0f / Fmt::SX;
      p = __builtin_fmaf(w8[k], x, p);
    }
    S.part[wave * TILE + ray] = p;
    if constexpr (Fmt::RANGE) {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
        if (Fmt::top_overflowed(c.top[rb])) over[32 * rb + j] = 1u;
    }
  }
  __syncthreads();
  const float y = ((S.part[ray] + S.part[TILE + ray]) + (S.part[2 * TILE + ray] + S.part[3 * TILE + ray])) + D.b8;
  if constexpr (Fmt::RANGE) return over[ray] ? __builtin_nanf("") : y;
  else return y;
}

// ---------------------------------------------------------------------------------------- backward tile (dX chain)
// Gate + write-back of a backward layer: delta = mask bit ? acc (in the deltas' units) : 0 (bits in the forward's format), k-minor layout
template <class Fmt, int NOB, int RB>
__device__ __forceinline__ void split_writeback_gate(typename Fmt::template Act<RB>& X, const f32x16 (&acc)[NOB][RB], int row0, int lane, const uint32_t (&mask)[4]) {
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob) {
    const uint32_t m = mask[ob];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if constexpr (Fmt::SCALED) v[i] = gate(acc[ob][rb][4 * q + i] * Fmt::BACK, (m >> (rb * 16 + 4 * q + i)) & 1u);
          else v[i] = gate(acc[ob][rb][4 * q + i], (m >> (rb * 16 + 4 * q + i)) & 1u);
        }
        X.store4(row0 + 32 * ob + 8 * q + 4 * h, 32 * rb + j, v);
      }
  }
}

// dst[row] = sum over the tile's rays of delta[row][ray], in the exact tile's ray order (row_sums). Fmt::NORMALISED: the tile holds
// e = delta / d8 in units of SD, so the sum is weighted by d8 / SD (S.xyz row 0).
template <class Fmt, int RB>
__device__ __forceinline__ void split_row_sums(const SmemSplit<Fmt, RB>& S, float* __restrict__ dst, int tid) {
  constexpr int TILE = 32 * RB;
  const int lane = tid & 63;
#pragma unroll 1
  for (int rr = 0; rr < 2; ++rr) {
    const int row = tid + rr * 256;
    float s = 0.f;
#pragma unroll 8
    for (int i = 0; i < TILE; ++i) {
      const int ray = (i + lane) & (TILE - 1);
      if constexpr (Fmt::NORMALISED) s += S.act.read(row, ray) * S.xyz[ray];
      else s += S.act.read(row, ray);
    }
    dst[row] = s;
  }
}

// The dX chain of mlp_backward (distr_mlp.hpp) in split arithmetic. Preconditions: masks = the ReLU bitmasks of the forward
// being differentiated (saved mask blocks); S.aux row 0 = d8[ray] = coef (1 - y^2). On return S.aux rows 1..3 hold d(coef f)/d xyz
// per ray; sd0 / sd4 receive the row sums over the tile's rays of delta0 / delta4 (latent gradient).
// Fmt::NORMALISED (f16x3): d8 is a loss gradient: its magnitude has no bound, f16 has 5 exponent bits. The chain is linear in d8, so it
// runs on the NORMALISED deltas e_l = delta_l / d8 (e7 = relu'(h7) w8: a property of the decoder alone, |e| ~ 1e-3 .. 1; planes hold
// SD e) and d8 multiplies the results per ray: the row sums are weighted sums, the xyz gradient is scaled at the end. An e beyond the
// range (SD |e| > 65504) turns into inf / NaN planes, which the chain carries into non-finite gradients -- visible, not clamped.
template <class Fmt, int RB>
__device__ __forceinline__ void split_backward(const DecoderDev& D, const DecoderSplit& P, SmemSplit<Fmt, RB>& S, uint32_t (&masks)[8][4],
                                               float* __restrict__ sd0, float* __restrict__ sd4) {
  constexpr int TILE = 32 * RB;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int h = lane >> 5, j = lane & 31;
  const int ray = tid & (TILE - 1);
  auto& X = S.act;
  if constexpr (Fmt::NORMALISED) {         // S.xyz row 0 = d8 / SD (the saved-mask backward does not stage points: S.xyz is free)
    if (tid < TILE) S.xyz[tid] = S.aux[tid] * (1.0f / Fmt::SD);
  }
  u32x4 a[4][Fmt::NP];
  split_load_a<Fmt, 4>(P.Wb[7], 0, wave, lane, a);
  // delta7[k][ray] = relu'(h7) * w8[k] * d8[ray]   (exact f32, like the exact tile); NORMALISED: SD e7[k][ray] = relu'(h7) * w8[k] * SD
  {
    float d8[RB];
    if constexpr (!Fmt::NORMALISED) {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) d8[rb] = S.aux[32 * rb + j];
    }
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) {
      const uint32_t m = masks[7][ob];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 v[RB];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = wave * 128 + 32 * ob + 8 * q + 4 * h + i;
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) {
            if constexpr (Fmt::NORMALISED) v[rb][i] = gate(D.w8[row] * Fmt::SD, (m >> (16 * rb + 4 * q + i)) & 1u);
            else v[rb][i] = gate(D.w8[row] * d8[rb], (m >> (16 * rb + 4 * q + i)) & 1u);
          }
        }
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) X.store4(wave * 128 + 32 * ob + 8 * q + 4 * h, 32 * rb + j, v[rb]);
      }
    }
  }
  __syncthreads();
  auto zero = [&](auto& acc) {
#pragma unroll
    for (auto& ob : acc)
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) ob[rb][r] = 0.f;
  };
#pragma unroll
  for (int l = 7; l >= 5; --l) {  // delta_l (512) -> delta_{l-1} (512)
    f32x16 acc[4][RB];
    zero(acc);
    if (l > 5) split_dense<Fmt, 512, 4, RB, 4>(P.Wb[l], P.Wb[l - 1], X, acc, wave, lane, a);
    else split_dense<Fmt, 512, 4, RB, 2>(P.Wb[5], P.Wb[4], X, acc, wave, lane, a);
    __syncthreads();
    split_writeback_gate<Fmt, 4, RB>(X, acc, wave * 128, lane, masks[l - 1]);
    __syncthreads();
  }
  if (sd4) split_row_sums<Fmt, RB>(S, sd4, tid);  // X = delta4
  {  // lin4^T: delta4 (512) -> [delta3 (253) | d xyz (3)]
    f32x16 acc[2][RB];
    zero(acc);
    split_dense<Fmt, 512, 2, RB, 4>(P.Wb[4], P.Wb[3], X, acc, wave, lane, a);
    __syncthreads();
    split_writeback_gate<Fmt, 2, RB>(X, acc, wave * 64, lane, masks[3]);  // rows 253..255 have mask 0 -> written as 0
    if (wave == 3 && h == 1) {
#pragma unroll
      for (int r = 13; r < 16; ++r)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          if constexpr (Fmt::NORMALISED) S.aux[(1 + r - 13) * TILE + 32 * rb + j] = acc[1][rb][r] * (1.0f / (Fmt::SW * Fmt::SD));   // (per unit d8)
          else S.aux[(1 + r - 13) * TILE + 32 * rb + j] = acc[1][rb][r];
        }
    }
    __syncthreads();
  }
  {  // lin3^T: delta3 (256 rows, 253 real) -> delta2 (512)
    f32x16 acc[4][RB];
    zero(acc);
    split_dense<Fmt, 256, 4, RB, 4>(P.Wb[3], P.Wb[2], X, acc, wave, lane, a);
    __syncthreads();
    split_writeback_gate<Fmt, 4, RB>(X, acc, wave * 128, lane, masks[2]);
    __syncthreads();
  }
#pragma unroll
  for (int l = 2; l >= 1; --l) {
    f32x16 acc[4][RB];
    zero(acc);
    if (l > 1) split_dense<Fmt, 512, 4, RB, 4>(P.Wb[2], P.Wb[1], X, acc, wave, lane, a);
    else split_dense<Fmt, 512, 4, RB, 4>(P.Wb[1], nullptr, X, acc, wave, lane, a);
    __syncthreads();
    split_writeback_gate<Fmt, 4, RB>(X, acc, wave * 128, lane, masks[l - 1]);
    __syncthreads();
  }
  if (sd0) split_row_sums<Fmt, RB>(S, sd0, tid);  // X = delta0
  // d xyz through lin0's xyz columns: 3 x four 128-long f32 chains per ray
  {
    float p0 = 0.f, p1 = 0.f, p2 = 0.f;
    const float* wx = D.W0x + wave * 128;
#pragma unroll 4
    for (int k = 0; k < 128; ++k) {
      const float d = X.read(wave * 128 + k, ray);
      p0 = __builtin_fmaf(wx[k], d, p0);
      p1 = __builtin_fmaf(wx[HID + k], d, p1);
      p2 = __builtin_fmaf(wx[2 * HID + k], d, p2);
    }
    S.part[(0 * 4 + wave) * TILE + ray] = p0;
    S.part[(1 * 4 + wave) * TILE + ray] = p1;
    S.part[(2 * 4 + wave) * TILE + ray] = p2;
  }
  __syncthreads();
  if (tid < 3 * TILE) {
    const int c = tid / TILE, r = tid % TILE;
    const float* p = S.part + c * 4 * TILE + r;
    if constexpr (Fmt::NORMALISED) {
      const float unit = S.aux[(1 + c) * TILE + r] + ((p[0] + p[TILE]) + (p[2 * TILE] + p[3 * TILE])) * (1.0f / Fmt::SD);
      S.aux[(1 + c) * TILE + r] = unit * S.aux[r];     // x d8 of the ray
    } else {
      S.aux[(1 + c) * TILE + r] = S.aux[(1 + c) * TILE + r] + ((p[0] + p[TILE]) + (p[2 * TILE] + p[3 * TILE]));
    }
  }
  __syncthreads();
}

// decode_sdf (core/utils/decoder_utils.py:53-74) for n explicit points in split arithmetic; Fmt::RANGE: a point whose evaluation left
// the format's range gets NaN (not a clamped number)
template <int ARITH>
__global__ void __launch_bounds__(256, 1) k_eval_split(const float* __restrict__ xyz, int64_t n, const float* __restrict__ c0c4, float clamp,
                                                       float* __restrict__ sdf, DecoderDev D, DecoderSplit P) {
  using Fmt = SplitFmt<ARITH>;
  __shared__ SmemSplit<Fmt, 2> S;
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * 64;
  if (base >= n) return;
  if (tid < 64) {
    const int64_t r = base + tid;
    const bool v = r < n;
    S.xyz[tid] = v ? xyz[r * 3] : 0.f; S.xyz[64 + tid] = v ? xyz[r * 3 + 1] : 0.f; S.xyz[128 + tid] = v ? xyz[r * 3 + 2] : 0.f;
  }
  __syncthreads();
  uint32_t masks[8][4];
  const float pre = split_forward<Fmt, 2, false>(D, P, c0c4, c0c4 + HID, S, masks);
  if (tid < 64 && base + tid < n) {
    const float s = tanh_spec(pre);
    const float out = (clamp >= 0.f) ? clampf(s, -clamp, clamp) : s;
    if constexpr (Fmt::RANGE) sdf[base + tid] = !(fabsf(pre) <= 3.0e38f) ? __builtin_nanf("") : out;
    else sdf[base + tid] = out;
  }
}

}  // namespace distr
