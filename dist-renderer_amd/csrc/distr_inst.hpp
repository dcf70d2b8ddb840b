// distr_inst.hpp -- THE list of variants of the big template kernels (k_step, k_tail, k_march, k_march16, k_bwd): one line per
// instantiation, with its template arguments, in the DISTR_GROUP_<n> list of the translation unit that holds its code (libdistr.so builds
// those units in parallel: distr.binding.build_library compiles distr_api.hip and distr_inst.hip once per group side by side and links
// them, ~1.5 min instead of ~4.5 on 8 cores). Two things are generated from the lists, and nothing else names a variant:
//   * the declarations at the end: `template` for the group a unit builds (DISTR_INST_GROUP), `extern template` for all of them in
//     distr_api.hip, which launches the kernels and holds none of their code;
//   * the launchers of distr_api.hip (launch_step ... launch_bwd): run-time values to a listed instantiation, anything else refused.
// So a variant exists exactly when it has a line here; tests/test_host_logic.py checks on a built tree that distr_api.hip's device code
// defines none of these kernels.
#pragma once
#include "distr_kernels.hpp"

namespace distr {

// Every list takes one macro per kernel family and calls it once per variant, in the order the unit emits them:
//   STEP(KEEP, ARITH, COMPACT)  TAIL(KEEP)  MARCH(MODE, RB, KEEP, ARITH, WIDE, COMPACT)  MARCH16(MODE, KEEP)  BWD(MODE, RB, ARITH, WIDE, COMPACT)
// KEEP = save the ReLU masks, RB = 32-ray blocks of a tile, ARITH = DISTR_ARITH_* (0 f32, 1 bf16x6, 2 f16x3), WIDE = the layout for
// code lengths below 256, COMPACT = the 64-ray / 64-sample tile walks the live hidden units of a tile only (exact f32, narrow layout;
// distr_mlp.hpp; the backward: the tile over saved masks, BWD_SAVED, whose live sets are known before its chain starts). STEP's COMPACT is a
// level: 0 none, 1 the 64-ray role, 2 the 64- and the 32-ray role.

// the full-resolution step of the exact-f32 march (the headline kernel)
#define DISTR_GROUP_1(STEP, TAIL, MARCH, MARCH16, BWD) \
  STEP(true, 0, 0) STEP(false, 0, 0)
// the persistent tail launch
#define DISTR_GROUP_2(STEP, TAIL, MARCH, MARCH16, BWD) \
  TAIL(true) TAIL(false)
// exact-f32 march tiles: coarse levels, 'trivial', point lists; 16-ray / cluster tiles
#define DISTR_GROUP_3(STEP, TAIL, MARCH, MARCH16, BWD) \
  MARCH(MODE_EVAL, 2, false, 0, false, false) \
  MARCH(MODE_COARSE, 1, true, 0, false, false) MARCH(MODE_COARSE, 1, false, 0, false, false) MARCH(MODE_COARSE, 2, true, 0, false, false) MARCH(MODE_COARSE, 2, false, 0, false, false) \
  MARCH(MODE_FINE, 2, true, 0, false, false) MARCH(MODE_FINE, 2, false, 0, false, false) \
  MARCH16(MODE_EVAL, false) MARCH16(MODE_COARSE, true) MARCH16(MODE_COARSE, false)
// the step kernel in the two opt-in arithmetics
#define DISTR_GROUP_4(STEP, TAIL, MARCH, MARCH16, BWD) \
  STEP(true, 1, 0) STEP(false, 1, 0) STEP(true, 2, 0) STEP(false, 2, 0)
// march tiles in the two opt-in arithmetics
#define DISTR_GROUP_5(STEP, TAIL, MARCH, MARCH16, BWD) \
  MARCH(MODE_COARSE, 1, true, 1, false, false) MARCH(MODE_COARSE, 1, false, 1, false, false) MARCH(MODE_COARSE, 2, true, 1, false, false) MARCH(MODE_COARSE, 2, false, 1, false, false) \
  MARCH(MODE_FINE, 2, true, 1, false, false) MARCH(MODE_FINE, 2, false, 1, false, false) \
  MARCH(MODE_COARSE, 1, true, 2, false, false) MARCH(MODE_COARSE, 1, false, 2, false, false) MARCH(MODE_COARSE, 2, true, 2, false, false) MARCH(MODE_COARSE, 2, false, 2, false, false) \
  MARCH(MODE_FINE, 2, true, 2, false, false) MARCH(MODE_FINE, 2, false, 2, false, false)
// backward kernels
#define DISTR_GROUP_6(STEP, TAIL, MARCH, MARCH16, BWD) \
  BWD(BWD_FULL, 2, 0, false, false) BWD(BWD_POINTGRAD, 2, 0, false, false) \
  BWD(BWD_SAVED, 1, 0, false, false) BWD(BWD_SAVED, 1, 1, false, false) BWD(BWD_SAVED, 1, 2, false, false) \
  BWD(BWD_SAVED, 2, 0, false, false) BWD(BWD_SAVED, 2, 1, false, false) BWD(BWD_SAVED, 2, 2, false, false)
// the wide layout (code length < 256): 64-ray march tiles; 64- and 32-sample backward tiles
#define DISTR_GROUP_7(STEP, TAIL, MARCH, MARCH16, BWD) \
  MARCH(MODE_EVAL, 2, false, 0, true, false) MARCH(MODE_COARSE, 2, true, 0, true, false) MARCH(MODE_COARSE, 2, false, 0, true, false) \
  MARCH(MODE_FINE, 2, true, 0, true, false) MARCH(MODE_FINE, 2, false, 0, true, false) \
  BWD(BWD_FULL, 2, 0, true, false) BWD(BWD_POINTGRAD, 2, 0, true, false) BWD(BWD_SAVED, 2, 0, true, false) BWD(BWD_SAVED, 1, 0, true, false)

// the compacted 64-ray tile (DISTR_DENSE_COMPACT, the default): the step kernel with a dense 32-ray role (level 1: DISTR_COMPACT32=0) ...
#define DISTR_GROUP_8(STEP, TAIL, MARCH, MARCH16, BWD) \
  STEP(true, 0, 1) STEP(false, 0, 1)
// ... and the 64-ray march tiles
#define DISTR_GROUP_9(STEP, TAIL, MARCH, MARCH16, BWD) \
  MARCH(MODE_EVAL, 2, false, 0, false, true) MARCH(MODE_COARSE, 2, true, 0, false, true) MARCH(MODE_COARSE, 2, false, 0, false, true) \
  MARCH(MODE_FINE, 2, true, 0, false, true) MARCH(MODE_FINE, 2, false, 0, false, true)

// ... and the 64-sample backward tile over saved masks
#define DISTR_GROUP_10(STEP, TAIL, MARCH, MARCH16, BWD) \
  BWD(BWD_SAVED, 2, 0, false, true)

// ... and the step kernel whose 32-ray role is compacted too (level 2: DISTR_COMPACT32, the default)
#define DISTR_GROUP_11(STEP, TAIL, MARCH, MARCH16, BWD) \
  STEP(true, 0, 2) STEP(false, 0, 2)

constexpr int DISTR_NUM_INST_GROUPS = 11;

#define DISTR_ALL_GROUPS(...) \
  DISTR_GROUP_1(__VA_ARGS__) DISTR_GROUP_2(__VA_ARGS__) DISTR_GROUP_3(__VA_ARGS__) DISTR_GROUP_4(__VA_ARGS__) DISTR_GROUP_5(__VA_ARGS__) \
  DISTR_GROUP_6(__VA_ARGS__) DISTR_GROUP_7(__VA_ARGS__) DISTR_GROUP_8(__VA_ARGS__) DISTR_GROUP_9(__VA_ARGS__) DISTR_GROUP_10(__VA_ARGS__) \
  DISTR_GROUP_11(__VA_ARGS__)
#define DISTR_NO_VARIANT(...)      // for the families a use of the lists does not ask for

// in a group's translation unit only that group is instantiated; the launching unit declares all of them extern
#ifdef DISTR_INST_GROUP
#define DISTR_INST_DEF template
#define DISTR_INST_CAT_(a, b) a##b
#define DISTR_INST_CAT(a, b) DISTR_INST_CAT_(a, b)
#define DISTR_INST_LIST DISTR_INST_CAT(DISTR_GROUP_, DISTR_INST_GROUP)
#else
#define DISTR_INST_DEF extern template
#define DISTR_INST_LIST DISTR_ALL_GROUPS
#endif

#define DISTR_K_STEP(K, AR, C) DISTR_INST_DEF __global__ void k_step<K, AR, C>(MarchArgs, DecoderDev, DecoderDev16, StepGrid);
#define DISTR_K_TAIL(K) DISTR_INST_DEF __global__ void k_tail<K>(MarchArgs, DecoderDev, DecoderDev16);
#define DISTR_K_MARCH(M, RB, K, AR, W, C) DISTR_INST_DEF __global__ void k_march<M, RB, K, AR, W, C>(MarchArgs, DecoderDev);
#define DISTR_K_MARCH16(M, K) DISTR_INST_DEF __global__ void k_march16<M, K>(MarchArgs, DecoderDev, DecoderDev16);
#define DISTR_K_BWD(M, RB, AR, W, C) DISTR_INST_DEF __global__ void k_bwd<M, RB, AR, W, C>(BwdArgs, DecoderDev);

DISTR_INST_LIST(DISTR_K_STEP, DISTR_K_TAIL, DISTR_K_MARCH, DISTR_K_MARCH16, DISTR_K_BWD)

}  // namespace distr
