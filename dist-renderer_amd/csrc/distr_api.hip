// distr_api.hip -- host side of libdistr.so: C ABI (include/distr.h), weight-fragment packer, workspace carving,
// kernel launch sequences. Built with: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fPIC (-c, next to the distr_inst.hip
// groups; distr.binding.build_library links them into libdistr.so).
// No device allocation / synchronisation happens inside forward/backward (caller-owned workspaces, caller's stream).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "distr_inst.hpp"      // distr_kernels.hpp + the big template kernels as extern templates (their code: distr_inst.hip, per group)
#include "distr_losses.hpp"
#include "distr_mesh.hpp"
#include "distr_mlp_split.hpp"
#include "distr_samples.hpp"
#include "distr_normal_grad.hpp"
#include "distr_color_batch.hpp"
#include "distr_color_loss.hpp"
#include "distr_train.hpp"

using namespace distr;

struct distr_ctx {
  int device = 0;
  std::mutex mu;             // entry points serialise per context (exchange regions, event pool, error text); launches stay async
  std::string err;
  float* dec_buf = nullptr;  // one device allocation holding every packed array
  float* dec_buf_color = nullptr;   // same for the colour decoder (distr_set_color_decoder)
  DecoderDev DC{};
  bool has_color = false;
  DecoderDev D{};
  DecoderDev16 D16{};
  DecoderSplit planes[2]{};         // [arith - 1]: split-bf16 / split-f16 weight planes of the shape decoder (distr_mlp_split.hpp) ...
  uint32_t* dec_buf_split = nullptr;   // ... in one allocation of their own
  bool h3_ok = false;               // f16x3: every layer's largest |weight| lies in [H3_WMIN, H3_WMAX); otherwise h3_why names the first
  std::string h3_why;               // layer outside it
  bool has_decoder = false;
  bool profiling = false;
  int hybrid_threshold = 8192;  // t32: largest remainder of a march step (rays) that runs on 32-ray tiles (fine_split)
  int tail16_threshold = 4096;  // t16: ... and on 16-ray tiles (16x16x4 MFMA)
  bool compact32 = true;        // DISTR_COMPACT32=0: the 32-ray role of the exact-f32 step kernel keeps the dense loop (a time knob; only effective with dense_compact)
  bool dense_compact = true;    // DISTR_DENSE_COMPACT=0: the exact-f32 64-ray tile (march and saved-mask backward) multiplies every hidden unit, live for the tile or not (a time knob)
  bool live_order = true;       // DISTR_LIVE_ORDER=0: every full-resolution step appends its survivors atomically, in completion order (no k_live_pack; a time knob)
  bool ray_blocks = true;       // DISTR_RAY_BLOCKS=0: the setup kernels enumerate pixels in strips of 256 instead of 16 x 16 blocks (a time knob)
  int debug_steps = -1;         // distr_debug_live_list: the forward stops behind this many full-resolution steps (no tail launch, no finalize)
  bool save_masks = true;       // save ReLU masks in the forward so that the backward skips the decoder recompute
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  size_t ev_used = 0;
  // exchange regions of the cluster tiles (distr_mlp.hpp, "Cluster tile"): granule slots in ordinary (cached) device memory +
  // assembly words in uncached memory, one region per stream that renders through this context (concurrent renders on different
  // streams must not share them)
  struct XRegion { char* buf = nullptr; uint32_t* flags = nullptr; uint32_t epoch = 0; hipStream_t stream = nullptr; bool used = false; uint64_t last_use = 0; };
  uint64_t xr_clock = 0;
  bool xchg_ts = false;         // DISTR_XCHG_TS=1: cluster 0 / member 0 writes phase stamps behind the flag words (distr_debug_xchg_ts)
  static constexpr int NXR = 8;
  XRegion xr[NXR];
  bool cluster = true;          // DISTR_CLUSTER=0: single-workgroup 16-ray tiles only
  int max_cl = 8;               // DISTR_CLUSTER=4|8: largest cluster size
  int min_cl = 2;               // smallest cluster: pair tiles (2 CUs per 16 rays) for 1008 < rays <= 2032 (DISTR_CLUSTER_MIN=4: off)
  int cluster_test_abort = 0;   // DISTR_CLUSTER_TEST_ABORT (tests): 1 = every cluster aborts at assembly (fallback path); 2 = member 0 of every cluster
                                // gives up while staging h7, behind its last slice (the others complete without noticing: Xchg::test_abort)
  bool sticky = true;           // DISTR_STICKY=0: cluster tiles never keep their rays across march steps (sticky_tile16)
  int xchg_sc1 = 0;             // DISTR_XCHG_SC1=1 (tests): write-through slice stores even for clusters on one XCD (the mixed-XCD path)
  int cluster_spread = 0;       // DISTR_CLUSTER_SPREAD=1 (tests): cluster members on consecutive workgroups = different XCDs (Xchg::spread)
  // Persistent tail launch (k_tail): the full-resolution steps from `tail_from` on run inside one launch. tail_from is a HOST decision
  // taken without synchronising: the step at which the PREVIOUS render of the same configuration first had at most tail_rays live rays
  // (k_finalize writes it to a host-mapped word, read here whenever the next render is enqueued: stale is fine, k_tail is correct for any
  // count); no hint yet (a configuration's first render): no tail launch. tail_rays sits just above the 496 rays at which a step's tiles
  // turn sticky: a step inside k_tail costs a few microseconds MORE than a launch of its own (claim + release / acquire fences against a
  // launch boundary, profiles/r06_tail_steps.md), what the tail launch saves is every launch the host would issue behind the last live
  // ray -- so it takes over right where the sticky tiles would.
  bool tail = true;             // DISTR_TAIL=0: one launch per step to the end (rounds 1-5)
  int tail_px = 0;              // DISTR_TAIL_PX: renders of at most this many pixels start the tail launch at step 0 (0: hint only)
  int tail_rays = 640;          // DISTR_TAIL_RAYS
  int tail_force = -1;          // DISTR_TAIL_FROM=n (tests): tail_from = n for every render of the recursive marchers
  int tail_absent = 0;          // DISTR_TAIL_TEST_ABSENT=n (tests): the first n workgroups of the tail launch leave at once (never resident)
  struct TailHint { int32_t key[16]; bool used = false; uint64_t last_use = 0; };
  static constexpr int NHINT = 16;
  TailHint hints[NHINT];
  int32_t* hint_host = nullptr; // 2 x NHINT host-mapped words (hipHostMalloc): -1 = nothing written yet; [i] tail launch, [NHINT + i] end of the ordered steps
  int32_t* hint_dev = nullptr;
  bool hint_failed = false;
};

namespace {

int fail(distr_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}

// Every entry point that launches or allocates runs with the CONTEXT's device current and restores the caller's device on exit
// (a context for a GPU other than the caller's current one must not depend on, or leave behind, a changed current device).
struct EntryGuard {
  std::lock_guard<std::mutex> lock;
  int prev = -1, dev;
  explicit EntryGuard(distr_ctx* ctx) : lock(ctx->mu), dev(ctx->device) {
    if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~EntryGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
};

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(ctx, DISTR_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

#define LAUNCH_CHECK(name)                                                                    \
  do {                                                                                        \
    hipError_t e_ = hipGetLastError();                                                        \
    if (e_ != hipSuccess) return fail(ctx, DISTR_ERR_HIP, "launch %s: %s", name, hipGetErrorString(e_)); \
  } while (0)

// A-fragment packing for v_mfma_f32_32x32x2_f32 (see distr_mlp.hpp::dense):
//   dst float4 index ((g*4 + w)*NOB + ob)*64 + lane = { W[o][8g+2s+h] : s=0..3 }, o = w*32*NOB + 32*ob + (lane&31), h = lane>>5
void pack_fragments(const float* W, int K, int O, float* dst) {
  const int NOB = O / 128, NG = K / 8;
  for (int g = 0; g < NG; ++g)
    for (int w = 0; w < 4; ++w)
      for (int ob = 0; ob < NOB; ++ob)
        for (int lane = 0; lane < 64; ++lane) {
          const int o = w * 32 * NOB + 32 * ob + (lane & 31), h = lane >> 5;
          float* d = dst + ((((size_t)g * 4 + w) * NOB + ob) * 64 + lane) * 4;
          for (int s = 0; s < 4; ++s) d[s] = W[(size_t)o * K + 8 * g + 2 * s + h];
        }
}

// k-major pack for the compacted 64-ray tile (distr_mlp.hpp, "compacted 64-ray tile"): one row of O floats per input feature k, a wave's
// rows interleaved so that the 4 (NOB) floats at [RW * w + NOB * j + ob] are lane j's A operands of all its row blocks:
//   dst[k * O + RW * w + NOB * j + ob] = W[RW * w + 32 * ob + j][k],  RW = 32 * NOB rows per wave, NOB = O / 128
void pack_kmajor(const float* W, int K, int O, float* dst) {
  const int NOB = O / 128, RW = 32 * NOB;
  for (int k = 0; k < K; ++k)
    for (int w = 0; w < 4; ++w)
      for (int j = 0; j < 32; ++j)
        for (int ob = 0; ob < NOB; ++ob) dst[(size_t)k * O + RW * w + NOB * j + ob] = W[(size_t)(RW * w + 32 * ob + j) * K + k];
}

// A-fragments of v_mfma_f32_16x16x4_f32 (distr_mlp.hpp::dense16):
//   float4 index ((g*4 + w)*NB + ob)*64 + lane = { W[w*16*NB + 16*ob + (lane&15)][16g + 4s + (lane>>4)] : s = 0..3 }
void pack_fragments16(const float* W, int K, int O, float* dst) {
  const int NB = O / 64, NG = K / 16;
  for (int g = 0; g < NG; ++g)
    for (int w = 0; w < 4; ++w)
      for (int ob = 0; ob < NB; ++ob)
        for (int lane = 0; lane < 64; ++lane) {
          const int o = w * 16 * NB + 16 * ob + (lane & 15), kq = lane >> 4;
          float* d = dst + ((((size_t)g * 4 + w) * NB + ob) * 64 + lane) * 4;
          for (int s = 0; s < 4; ++s) d[s] = W[(size_t)o * K + 16 * g + 4 * s + kq];
        }
}

// bf16 (round to nearest even) of an f32, as its upper 16 bits
inline uint16_t to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float from_bf16(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// One f32 as the planes of a split format (distr_mlp_split.hpp), round to nearest even of the running remainder; false: left the range.
// bf16x6: W = w0 + w1 + w2 with w0 = bf16(W), w1 = bf16(W - w0), w2 = bf16(W - w0 - w1)
inline bool split_bf16x3(float v, uint16_t* pl) {
  pl[0] = to_bf16(v);
  const float r1 = v - from_bf16(pl[0]);
  pl[1] = to_bf16(r1);
  pl[2] = to_bf16(r1 - from_bf16(pl[1]));
  return true;
}
// f16x3: SW W = w0 + w1 with w0 = f16(SW W), w1 = f16(SW W - w0) (denormals kept)
inline bool split_f16x2(float w, uint16_t* pl) {
  const float v = FmtH3::SW * w;
  const _Float16 h0 = (_Float16)v;
  const _Float16 h1 = (_Float16)(v - (float)h0);
  memcpy(&pl[0], &h0, 2); memcpy(&pl[1], &h1, 2);
  return fabsf(v) < 65504.f;
}

// A-fragment planes of v_mfma_f32_32x32x16_{bf16,f16} (distr_mlp_split.hpp::split_dense): fragment index
// (((kb * 4 + wave) * NOB + ob) * NP + plane) * 64 + lane holds the 8 values W_plane[o][16 kb + 8 h + 0..7],
// o = wave * 32 NOB + 32 ob + (lane & 31), h = lane >> 5. Returns false when a weight leaves the format's range.
template <class Split>
bool pack_fragments_split(const float* W, int K, int O, int NP, Split split, uint16_t* dst) {
  const int NOB = O / 128, NKB = K / 16;
  bool ok = true;
  for (int kb = 0; kb < NKB; ++kb)
    for (int w = 0; w < 4; ++w)
      for (int ob = 0; ob < NOB; ++ob)
        for (int lane = 0; lane < 64; ++lane) {
          const int o = w * 32 * NOB + 32 * ob + (lane & 31), h = lane >> 5;
          for (int i = 0; i < 8; ++i) {
            uint16_t pl[3];
            if (!split(W[(size_t)o * K + 16 * kb + 8 * h + i], pl)) ok = false;
            for (int p = 0; p < NP; ++p)
              dst[((((((size_t)kb * 4 + w) * NOB + ob) * NP + p) * 64 + lane) * 8) + i] = pl[p];
          }
        }
  return ok;
}

struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base((char*)b) {}
  template <typename T>
  T* take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? (T*)(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
};

// The pyramid of a cfg, finest level first (index = LevelView index): scale[0] = 1, steps[l] = dense steps of coarse level l.
// distr_render_cfg::num_levels == 0: the default scale_list [4,2,1] ([2,1] with coarse_steps = {s, 0}) described by coarse_steps;
// else level_scale / level_steps (coarsest first, like scale_list / march_step_list of renderer.py:25-26). Returns why not, or null.
struct Pyramid { int nlev; int scale[MAX_LEVELS]; int steps[MAX_LEVELS]; };
const char* pyramid_of(const distr_render_cfg& c, Pyramid& p) {
  memset(&p, 0, sizeof(p));
  p.nlev = 1; p.scale[0] = 1;
  if (c.marcher != DISTR_MARCH_PYRAMID_RECURSIVE) return nullptr;
  if (c.num_levels == 0) {
    // coarse_steps[1] == 0: the two-level pyramid scale_list=[2,1] (coarse_steps[0] steps at half resolution); a level with no steps
    // does not exist in the reference (ray_marching_trivial concatenates an empty list)
    if (c.coarse_steps[0] < 1 || c.coarse_steps[1] < 0) return "pyramid needs >=1 step per coarse level";
    p.nlev = (c.coarse_steps[1] == 0) ? 2 : 3;
    for (int l = 1; l < p.nlev; ++l) { p.scale[l] = 1 << l; p.steps[l] = c.coarse_steps[p.nlev - 1 - l]; }
  } else {
    if (c.num_levels < 2 || c.num_levels > MAX_LEVELS) return "num_levels must be 0 (coarse_steps) or 2..4";
    p.nlev = c.num_levels;
    for (int l = 0; l < p.nlev; ++l) { p.scale[l] = c.level_scale[p.nlev - 1 - l]; p.steps[l] = l ? c.level_steps[p.nlev - 1 - l] : 0; }
    if (p.scale[0] != 1) return "the last entry of level_scale (scale_list) must be 1 (renderer.py:726)";
    for (int l = 1; l < p.nlev; ++l) {
      if (p.scale[l] <= p.scale[l - 1] || p.scale[l] % p.scale[l - 1] != 0 || p.scale[l] / p.scale[l - 1] > 8)
        return "level_scale: every scale must be an integer multiple (2..8 x) of the next finer one";
    }
  }
  for (int l = 1; l < p.nlev; ++l) {
    if (p.steps[l] < 1) return "pyramid needs >=1 step per coarse level";
    if (p.steps[l] > 15) return "at most 15 steps per coarse level";
  }
  return nullptr;
}

int check_cfg(distr_ctx* ctx, const distr_render_cfg* c) {
  if (!c) return fail(ctx, DISTR_ERR_INVALID_ARG, "cfg is null");
  if (c->struct_size != sizeof(distr_render_cfg))      // ABI handshake (include/distr.h): a caller built against another header
    return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_render_cfg.struct_size is %u, this library (ABI %u) expects %zu: caller compiled against "
                "another include/distr.h, or the struct was not initialised with DISTR_INIT", c->struct_size, DISTR_ABI_VERSION, sizeof(distr_render_cfg));
  if (c->H < 1 || c->W < 1 || (int64_t)c->H * c->W >= (1 << 26)) return fail(ctx, DISTR_ERR_INVALID_ARG, "bad image size %dx%d", c->H, c->W);
  if (c->buffer_size < 1 || c->buffer_size > MAX_BS) return fail(ctx, DISTR_ERR_UNSUPPORTED, "buffer_size %d not in [1,%d]", c->buffer_size, MAX_BS);
  if (c->marcher < 0 || c->marcher > 2) return fail(ctx, DISTR_ERR_INVALID_ARG, "unknown marcher %d", c->marcher);
  int fine = c->march_step, coarse_rows = 0;
  if (c->marcher == DISTR_MARCH_PYRAMID_RECURSIVE) {
    Pyramid py;
    if (const char* why = pyramid_of(*c, py)) return fail(ctx, DISTR_ERR_UNSUPPORTED, "%s", why);
    for (int l = 1; l < py.nlev; ++l) { fine -= py.steps[l]; coarse_rows += py.steps[l]; }
    if (c->rows != 0 && c->rows != c->H && 4 % py.scale[py.nlev - 1] != 0)
      return fail(ctx, DISTR_ERR_UNSUPPORTED, "row bands (row0 a multiple of 4) need a pyramid whose coarsest scale divides 4");
  }
  if (fine < 1 || fine > MAX_STEPS) return fail(ctx, DISTR_ERR_INVALID_ARG, "march_step %d leaves %d full-resolution steps (need 1..%d)", c->march_step, fine, MAX_STEPS);
  // fewer marched rows than selected rows: the reference's torch.topk raises ("selected index k out of range", renderer.py:314-318) unless an
  // early break happens to pad the lists (:562-567) -- refused here, where the reference fails at render time
  if (coarse_rows + fine < c->buffer_size)
    return fail(ctx, DISTR_ERR_INVALID_ARG, "buffer_size %d exceeds the %d rows a ray's march produces (march_step %d): the reference's top-k selection raises there",
                c->buffer_size, coarse_rows + fine, c->march_step);
  if (!(c->radius > 0.f) || !(c->threshold >= 0.f)) return fail(ctx, DISTR_ERR_INVALID_ARG, "bad radius/threshold");
  if (c->arith != DISTR_ARITH_F32 && c->arith != DISTR_ARITH_BF16X6 && c->arith != DISTR_ARITH_F16X3) return fail(ctx, DISTR_ERR_INVALID_ARG, "unknown arith %d", c->arith);
  if (c->arith != DISTR_ARITH_F32 && ctx && ctx->has_decoder && ctx->D.nlat != LAT)
    return fail(ctx, DISTR_ERR_UNSUPPORTED, "arith %s: the split arithmetics are built for code length %d only (this decoder: %d); use f32",
                c->arith == DISTR_ARITH_BF16X6 ? "bf16x6" : "f16x3", LAT, ctx->D.nlat);
  if (c->arith == DISTR_ARITH_F16X3 && ctx && ctx->has_decoder && !ctx->h3_ok)
    return fail(ctx, DISTR_ERR_UNSUPPORTED, "arith f16x3: %s; use bf16x6 or f32 for this decoder", ctx->h3_why.c_str());
  if (c->rows != 0) {
    if (c->rows < 0 || c->row0 < 0 || c->row0 + c->rows > c->H) return fail(ctx, DISTR_ERR_INVALID_ARG, "row band [%d,+%d) outside the %d-row image", c->row0, c->rows, c->H);
    if ((c->row0 & 3) || ((c->rows & 3) && c->row0 + c->rows != c->H))
      return fail(ctx, DISTR_ERR_INVALID_ARG, "row band [%d,+%d) must start on a multiple of 4 and span a multiple of 4 rows (or end at H)", c->row0, c->rows);
  }
  return DISTR_OK;
}

inline bool is_capturing(hipStream_t stream) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
  return cs != hipStreamCaptureStatusNone;
}

// Exchange region of `stream` (allocated on the stream's first render: 32 MiB of granule slots + 128 KiB of uncached assembly
// words; steady state never allocates). Null (-> single-workgroup tiles) when disabled, out of regions, or the allocation fails.
distr_ctx::XRegion* xchg_region(distr_ctx* ctx, hipStream_t stream) {
  if (!ctx->cluster) return nullptr;
  // a launch sequence that is being captured into a graph would replay with the epochs of the capture (the barrier words
  // would already match) and must not allocate or query streams: single-workgroup tiles for captured renders
  if (is_capturing(stream)) return nullptr;
  distr_ctx::XRegion* free_slot = nullptr;
  for (auto& r : ctx->xr) {
    if (r.used && r.stream == stream) { r.last_use = ++ctx->xr_clock; return &r; }
    if (!r.used && !free_slot) free_slot = &r;
  }
  if (!free_slot) {
    // all regions taken: hand the least recently used one whose stream has nothing in flight to the new stream
    distr_ctx::XRegion* lru = nullptr;
    for (auto& r : ctx->xr) {
      if (lru && r.last_use >= lru->last_use) continue;
      const hipError_t q = hipStreamQuery(r.stream);
      if (q == hipErrorNotReady) continue;            // still working: its barrier words are live
      if (q != hipSuccess) (void)hipGetLastError();   // stale handle of a destroyed stream
      lru = &r;
    }
    if (!lru) return nullptr;
    lru->stream = stream; lru->last_use = ++ctx->xr_clock;
    return lru;
  }
  constexpr size_t buf_bytes = (size_t)256 * XCLUSTER_BYTES, flag_bytes = (size_t)256 * 128 * sizeof(uint32_t) + 64 * sizeof(long long);
  int cur = -1;
  (void)hipGetDevice(&cur);
  if (cur != ctx->device) (void)hipSetDevice(ctx->device);       // the region must live on the context's device
  struct Restore { int cur, dev; ~Restore() { if (cur >= 0 && cur != dev) (void)hipSetDevice(cur); } } restore{cur, ctx->device};
  // (granule tags start at 8 = epoch 1 << 3: a zeroed slot never validates)
  if (hipMalloc((void**)&free_slot->buf, buf_bytes) != hipSuccess ||
      hipExtMallocWithFlags((void**)&free_slot->flags, flag_bytes, hipDeviceMallocUncached) != hipSuccess ||
      hipMemset(free_slot->buf, 0, buf_bytes) != hipSuccess ||
      hipMemset(free_slot->flags, 0, flag_bytes) != hipSuccess) {
    (void)hipGetLastError();
    if (free_slot->buf) { (void)hipFree(free_slot->buf); free_slot->buf = nullptr; }
    if (free_slot->flags) { (void)hipFree(free_slot->flags); free_slot->flags = nullptr; }
    ctx->cluster = false;
    return nullptr;
  }
  free_slot->used = true; free_slot->stream = stream; free_slot->epoch = 0; free_slot->last_use = ++ctx->xr_clock;
  return free_slot;
}

// Exchange parameters of the next launch on region `r`. `epochs` = barrier epochs the launch may use (1; a step launch whose
// cluster tiles may go sticky uses one per remaining march step). Epochs stay below 2^28 (an arrival word is epoch << 4 | XCC id,
// a granule tag epoch << 3 | layer): before the counter gets there, the assembly words AND the granule slots are cleared on the
// stream (no stale word or tag may equal a future one) and counting restarts at 1.
inline Xchg next_xchg(distr_ctx::XRegion* r, hipStream_t s, bool ts, int max_cl, int test_abort, int min_cl, uint32_t epochs = 1, bool sticky = false,
                      int force_sc1 = 0) {
  Xchg x{nullptr, nullptr, 0, max_cl, min_cl, test_abort, nullptr, 0, 0, 1, force_sc1, 0, 0};
  if (r && ts) x.ts = reinterpret_cast<long long*>(r->flags + 256 * 128);
  if (r) {
    if (r->epoch > 0x0fffffffu - epochs - 1) {
      (void)hipMemsetAsync(r->flags, 0, (size_t)256 * 128 * sizeof(uint32_t), s);
      (void)hipMemsetAsync(r->buf, 0, (size_t)256 * XCLUSTER_BYTES, s);
      r->epoch = 0;
    }
    x.buf = r->buf; x.flags = r->flags; x.epoch = r->epoch + 1; x.epochs = epochs; x.sticky = sticky ? 1 : 0;
    r->epoch += epochs;
  }
  return x;
}

// Slot of this render configuration in the tail-hint table (least recently used entry replaced; its word restarts at -1 = no hint).
// Null when the host-mapped words cannot be had (allocation failed once, or the stream is capturing: no allocation inside a capture).
int32_t* tail_hint_slot(distr_ctx* ctx, const distr_render_cfg& c, int nviews, bool capturing, int32_t** dev_word) {
  *dev_word = nullptr;
  if (ctx->hint_failed) return nullptr;
  if (!ctx->hint_host) {
    if (capturing) return nullptr;
    void* h = nullptr;
    void* d = nullptr;
    if (hipHostMalloc(&h, 2 * distr_ctx::NHINT * sizeof(int32_t), hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
      (void)hipGetLastError();
      if (h) (void)hipHostFree(h);
      ctx->hint_failed = true;
      return nullptr;
    }
    ctx->hint_host = (int32_t*)h; ctx->hint_dev = (int32_t*)d;
    static_assert(distr_ctx::NHINT == HINT_ORDER_OFF, "k_finalize writes the order hint NHINT words behind the tail hint");
    for (int i = 0; i < 2 * distr_ctx::NHINT; ++i) ctx->hint_host[i] = -1;
  }
  Pyramid py;
  (void)pyramid_of(c, py);
  const int32_t key[16] = {c.H, c.W, c.row0, c.rows, c.march_step, c.marcher, c.buffer_size, nviews, py.nlev, py.scale[1], py.scale[2], py.scale[3],
                           py.steps[1], py.steps[2], py.steps[3], 0};
  static uint64_t clock = 0;
  int lru = 0;
  for (int i = 0; i < distr_ctx::NHINT; ++i) {
    auto& h = ctx->hints[i];
    if (h.used && memcmp(h.key, key, sizeof(key)) == 0) { h.last_use = ++clock; *dev_word = ctx->hint_dev + i; return ctx->hint_host + i; }
    if (!h.used) { lru = i; break; }
    if (h.last_use < ctx->hints[lru].last_use) lru = i;
  }
  auto& h = ctx->hints[lru];
  if (h.used && capturing) return nullptr;      // (re-using a slot resets its word from the host: not while a capture records device writes to it)
  memcpy(h.key, key, sizeof(key));
  h.used = true; h.last_use = ++clock;
  __atomic_store_n(ctx->hint_host + lru, -1, __ATOMIC_RELAXED);
  __atomic_store_n(ctx->hint_host + distr_ctx::NHINT + lru, -1, __ATOMIC_RELAXED);
  *dev_word = ctx->hint_dev + lru;
  return ctx->hint_host + lru;
}

inline int band_rows(const distr_render_cfg& c) { return c.rows > 0 ? c.rows : c.H; }
inline int band_row0(const distr_render_cfg& c) { return c.rows > 0 ? c.row0 : 0; }

// Lays the forward workspace out; with base==nullptr only sizes are computed.
size_t make_view(const distr_render_cfg& c, void* base, View& V, bool save_masks, int nviews = 1) {
  Carver cv(base);
  memset(&V, 0, sizeof(V));
  V.cfg = c;
  V.nviews = nviews;
  V.rows = band_rows(c); V.row0 = band_row0(c);
  V.band = (V.rows != c.H) ? 1 : 0;
  V.P = V.rows * c.W;
  V.pyramid = (c.marcher == DISTR_MARCH_PYRAMID_RECURSIVE) ? 1 : 0;
  Pyramid py;
  (void)pyramid_of(c, py);             // (check_cfg has accepted it)
  V.nlev = py.nlev;
  V.fine_steps = c.march_step;
  for (int l = 1; l < V.nlev; ++l) V.fine_steps -= py.steps[l];
  V.C = cv.take<Consts>(1);
  V.lv[0].h = V.rows; V.lv[0].w = c.W; V.lv[0].scale = 1.f; V.lv[0].off = 0.f;
  V.lv[0].y0 = V.row0; V.lv[0].full_h = c.H; V.lv[0].rdiv = 1; V.lv[0].sdiv = 1;
  for (int l = 1; l < V.nlev; ++l) {     // get_downscaled_grid_map (renderer.py:604-629): ceil(h / ratio) cells, centres scale * i + (scale - 1) / 2
    const int r = py.scale[l] / py.scale[l - 1];
    V.lv[l].rdiv = r; V.lv[l].sdiv = py.scale[l];
    V.lv[l].h = (V.lv[l - 1].h + r - 1) / r;
    V.lv[l].w = (V.lv[l - 1].w + r - 1) / r;
    V.lv[l].y0 = V.lv[l - 1].y0 / r;                 // a band's row0 is a multiple of the coarsest scale: exact
    V.lv[l].full_h = (V.lv[l - 1].full_h + r - 1) / r;
    V.lv[l].scale = (float)py.scale[l];
    V.lv[l].off = (V.lv[l].scale - 1.f) / 2.f;
  }
  for (int l = 0; l < V.nlev; ++l) {
    LevelView& L = V.lv[l];
    L.n = L.h * L.w;
    L.steps = py.steps[l];
    L.valid = cv.take<uint8_t>(L.n);
    L.list = cv.take<int32_t>(L.n);
    if (l > 0) {
      L.cinit = cv.take<float>(L.n);
      L.cm = cv.take<float>(L.n);
      L.rs = cv.take<float>((size_t)L.steps * L.n);
      L.rzb = cv.take<float>((size_t)L.steps * L.n);
      L.rza = cv.take<float>((size_t)L.steps * L.n);
    }
  }
  const size_t P = V.P, bs = c.buffer_size;
  V.live[0] = cv.take<int32_t>(P);
  V.live[1] = cv.take<int32_t>(P);
  V.lslot = cv.take<int32_t>(P + 64);
  V.tcount = cv.take<int32_t>(P / 16 + 4);
  V.m = cv.take<float>(P); V.init_now = cv.take<float>(P); V.maxbound = cv.take<float>(P);
  V.minabs = cv.take<float>(P); V.first_sdf = cv.take<float>(P);
  V.tk_s = cv.take<float>(bs * P); V.tk_zb = cv.take<float>(bs * P); V.tk_za = cv.take<float>(bs * P);
  V.tk_src = cv.take<int32_t>(bs * P);
  V.tk_slot = cv.take<int32_t>(bs * P);
  V.tclaim = cv.take<int32_t>(P / 16 + 2);
  V.tail_from = V.fine_steps;
  V.order_until = V.fine_steps;
  V.zdepth_s = cv.take<float>(P); V.depth_pre = cv.take<float>(P); V.nrm_t = cv.take<float>(3 * P);
  V.mask_s = cv.take<uint8_t>(P);
  V.nlist = cv.take<int32_t>(P); V.n_sdf = cv.take<float>(P); V.n_g = cv.take<float>(3 * P);
  V.save_masks = (save_masks && c.save_for_backward && (c.grad_depth || c.grad_mask)) ? 1 : 0;
  if (V.save_masks) {
    V.mfine = (int64_t)P * (bs + 1);
    int64_t off = 0;
    for (int l = 1; l < V.nlev; ++l) { V.moff[l] = off; off += (int64_t)V.lv[l].steps * V.lv[l].n; }
    V.morigin = V.mfine + off;
    V.mstore = cv.take<uint4>((size_t)(V.morigin + 1) * 32);
  }
  V.vstride = (int64_t)((cv.off + 255) & ~(size_t)255);    // view b of a batch: the same layout b * vstride bytes further
  return (size_t)V.vstride;
}

constexpr int BWD_CHUNK = 64;   // tiles per reduction chunk

size_t bwd_bytes(const distr_render_cfg& c) {
  const size_t P = (size_t)band_rows(c) * c.W;
  const size_t smax = P * c.buffer_size + 1;
  const size_t tiles = (smax + 31) / 32 + 256;
  const size_t nblk = (P + 255) / 256, nchunks = (tiles + BWD_CHUNK - 1) / BWD_CHUNK;
  const size_t b = ((smax * sizeof(Sample) + 255) & ~(size_t)255) + tiles * PSTRIDE * sizeof(float) + nchunks * PSTRIDE * sizeof(float) +
                   nblk * (2 * sizeof(int32_t) + 16 * sizeof(float)) + 2048;
  return (b + 255) & ~(size_t)255;
}

// The backward workspace of view 0 of a batch, carved (view b: bstride = bwd_bytes further): the one layout of render_backward_impl,
// which fills it, and distr_render_samples_export_batch, which reads the sample list back out of it. P: pixels of the rendered band.
struct BwdCarve { BwdWs W; size_t smax; int nblk; unsigned nchunks; };
BwdCarve carve_bwd(const distr_render_cfg& c, int P, void* ws_bwd) {
  BwdCarve b;
  b.smax = (size_t)P * c.buffer_size + 1;
  Carver cv(ws_bwd);
  b.W.bstride = (int64_t)bwd_bytes(c);
  b.W.samples = cv.take<Sample>(b.smax);
  const unsigned prows = (unsigned)((b.smax + 31) / 32) + 256;     // partial rows (sized for 32-sample tiles: bwd_bytes)
  b.W.partial = cv.take<float>((size_t)prows * PSTRIDE);
  b.nblk = (P + 255) / 256;
  b.nchunks = (prows + BWD_CHUNK - 1) / BWD_CHUNK;
  b.W.chunk_part = cv.take<float>((size_t)b.nchunks * PSTRIDE);
  b.W.BB.cnt = cv.take<int32_t>(b.nblk); b.W.BB.off = cv.take<int32_t>(b.nblk); b.W.BB.acc = cv.take<float>((size_t)b.nblk * 16);
  return b;
}

inline dim3 grid1(int64_t n, int per = 256) { return dim3((unsigned)((n + per - 1) / per)); }
inline dim3 gridv(const View& V, int64_t n) { return dim3((unsigned)((n + 255) / 256), (unsigned)V.nviews); }   // (blocks of 256, view)
// the setup kernels over a w x h grid (setup_pixel): 16 x 16 pixel blocks, or strips of 256 pixels
inline dim3 grid_setup(const View& V, int w, int h) { return V.blocks ? dim3((unsigned)block_grid(w, h), (unsigned)V.nviews) : gridv(V, (int64_t)w * h); }

struct MarchTimer {  // optional hipEvent bracket around the march kernel launches
  distr_ctx* ctx; hipStream_t s; bool on;
  MarchTimer(distr_ctx* c, hipStream_t st) : ctx(c), s(st), on(c->profiling) {}
  void begin() {
    if (!on) return;
    if (ctx->ev_used == ctx->ev_pool.size()) {
      hipEvent_t a, b;
      (void)hipEventCreate(&a); (void)hipEventCreate(&b);
      ctx->ev_pool.emplace_back(a, b);
    }
    (void)hipEventRecord(ctx->ev_pool[ctx->ev_used].first, s);
  }
  void end() {
    if (!on) return;
    (void)hipEventRecord(ctx->ev_pool[ctx->ev_used].second, s);
    ctx->ev_used++;
  }
};

// workspace carving: every array on a 256-byte boundary, the base aligned up (the byte counts include that slack)
struct WsCarve {
  uintptr_t at;
  size_t used = 0;
  explicit WsCarve(void* base) : at(((uintptr_t)base + 255) & ~(uintptr_t)255) {}
  template <typename T> T* take(size_t n) {
    T* p = (T*)(at + used);
    used += (n * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
  size_t bytes() const { return used + 256; }
};

// ---- point lists: n points decoded with one code (plain), or S segments with a code each (segmented), one launch sequence either way
struct PointList {
  int64_t n;                 // points (of all segments)
  unsigned tiles;            // 64-point tiles (every segment's count rounded up on its own)
  int32_t nseg;              // 0: the plain list -- one code, null table, zero SegCounts
  SegCounts cnt;
  float* c0c4;               // workspace: [codes][2 * HID] latent constants | (segmented) tile table | (backward) [tiles][PSTRIDE] partials
  SegTable* tab;
  float* partial;
  const char *bad_args, *small_ws;     // texts of the two refusals of point_list_prologue
};

PointList plain_list(int64_t n) {
  PointList pl;
  memset(&pl, 0, sizeof(pl));
  pl.n = n; pl.tiles = (unsigned)((n + 63) / 64);
  pl.bad_args = "bad argument"; pl.small_ws = "workspace too small";
  return pl;
}

// the plan of a segmented list, or why the list is refused: the error code, and the text through fail() (ctx may be null: the workspace sizes)
int seg_list(distr_ctx* ctx, int32_t nseg, const int64_t* counts, PointList& pl) {
  memset(&pl, 0, sizeof(pl));
  if (nseg < 1 || nseg > DISTR_MAX_VIEWS) return fail(ctx, DISTR_ERR_INVALID_ARG, "nseg %d: 1..%d", nseg, DISTR_MAX_VIEWS);
  if (!counts) return fail(ctx, DISTR_ERR_INVALID_ARG, "null counts (host array of nseg)");
  int64_t tiles = 0;
  for (int s = 0; s < nseg; ++s) {
    if (counts[s] < 0) return fail(ctx, DISTR_ERR_INVALID_ARG, "counts[%d] = %lld: negative", s, (long long)counts[s]);
    if (counts[s] > ((int64_t)1 << 30) || (pl.n += counts[s]) > ((int64_t)1 << 30))
      return fail(ctx, DISTR_ERR_UNSUPPORTED, "segmented point list: more than 2^30 points");
    pl.cnt.n[s] = counts[s];
    tiles += (counts[s] + SEG_TILE - 1) / SEG_TILE;
  }
  pl.tiles = (unsigned)tiles; pl.nseg = nseg;
  pl.bad_args = "null device pointer"; pl.small_ws = "segmented point list: workspace too small";
  return DISTR_OK;
}

// Lays the workspace of a list out (base == nullptr: sizes only) and returns the bytes the layout takes. The plain list: c0c4 at the
// 256-byte aligned base and, 2 * HID * sizeof(float) = 4096 being a multiple of 256, partial at c0c4 + 2 * HID floats with no table between
// them -- the layout distr_mlp_workspace_bytes / distr_mlp_backward_workspace_bytes size (the latter for ceil(n / 32) tiles: more than the
// ceil(n / 64) taken here, and that size is ABI).
static_assert(2 * HID * sizeof(float) % 256 == 0, "plain point list: partial follows c0c4 without padding");
size_t carve_list(void* base, PointList& pl, bool backward) {
  WsCarve c(base);
  pl.c0c4 = c.take<float>((size_t)std::max(pl.nseg, 1) * 2 * HID);
  pl.tab = pl.nseg ? c.take<SegTable>(1) : nullptr;
  pl.partial = backward ? c.take<float>((size_t)pl.tiles * PSTRIDE) : nullptr;
  return c.bytes();
}

// Prologue of the entry points that run decoder D on a point list: the null-pointer check (ptrs_ok: the caller's per-point arrays are
// there; an empty list needs none), the workspace size, the carve, then the constants the tiles read instead of the latent columns of
// lin0 / lin4 and the tile table of a segmented list (k_latent_consts). An empty list gets the checks and the carve only.
int point_list_prologue(distr_ctx* ctx, const DecoderDev& D, PointList& pl, const float* latent, int64_t latent_stride, bool ptrs_ok, void* ws,
                        size_t ws_bytes, bool backward, hipStream_t s) {
  if (pl.n < 0 || !latent || !ws || (pl.n > 0 && !ptrs_ok)) return fail(ctx, DISTR_ERR_INVALID_ARG, "%s", pl.bad_args);
  const size_t need = pl.nseg ? carve_list(nullptr, pl, backward) : backward ? distr_mlp_backward_workspace_bytes(pl.n) : distr_mlp_workspace_bytes(pl.n);
  if (ws_bytes < need) return fail(ctx, DISTR_ERR_WORKSPACE, "%s", pl.small_ws);
  carve_list(ws, pl, backward);
  if (pl.n == 0) return DISTR_OK;
  hipLaunchKernelGGL(k_latent_consts, pl.nseg ? dim3(4, (unsigned)pl.nseg) : dim3(4), dim3(256), 0, s, pl.c0c4, D, latent, latent_stride, pl.tab, pl.cnt);
  LAUNCH_CHECK("k_latent_consts");
  return DISTR_OK;
}

// Tail of every point-list backward: the code gradient(s) from the tiles' partial sums, a row per segment; zeros for an empty list.
int list_latent_grad(distr_ctx* ctx, const DecoderDev& D, const PointList& pl, float* g_latent, hipStream_t s) {
  if (!g_latent) return DISTR_OK;
  if (pl.n == 0) {
    HIP_TRY(hipMemsetAsync(g_latent, 0, (size_t)std::max(pl.nseg, 1) * D.nlat * sizeof(float), s));
    return DISTR_OK;
  }
  hipLaunchKernelGGL(k_points_latent_grad, dim3((unsigned)std::max(pl.nseg, 1)), dim3(256), 0, s, (const float*)pl.partial, pl.nseg ? 0 : (int)pl.tiles, D,
                     g_latent, (const SegTable*)pl.tab);
  LAUNCH_CHECK("k_points_latent_grad");
  return DISTR_OK;
}

}  // namespace

extern "C" {

const char* distr_version(void) { return "distr 0.6 (ABI 6; gfx950, f32 MFMA)"; }

uint32_t distr_abi_version(void) { return DISTR_ABI_VERSION; }

int distr_create_abi(distr_ctx** out, int hip_device, uint32_t abi_version) {
  if (!out) return DISTR_ERR_INVALID_ARG;
  *out = nullptr;
  distr_ctx* ctx = new distr_ctx();
  ctx->device = hip_device;
  if (abi_version != DISTR_ABI_VERSION) {
    ctx->err = "caller was built for distr ABI " + std::to_string(abi_version) + ", this library implements ABI " +
               std::to_string(DISTR_ABI_VERSION) + ": rebuild the caller against this include/distr.h";
    *out = ctx;
    return DISTR_ERR_INVALID_ARG;
  }
  if (const char* e = getenv("DISTR_HYBRID_THRESHOLD")) ctx->hybrid_threshold = atoi(e);
  if (const char* e = getenv("DISTR_TAIL16_THRESHOLD")) ctx->tail16_threshold = atoi(e);
  if (const char* e = getenv("DISTR_CLUSTER")) { ctx->cluster = atoi(e) != 0; if (atoi(e) >= 4) ctx->max_cl = atoi(e); }
  if (const char* e = getenv("DISTR_CLUSTER_MIN")) ctx->min_cl = atoi(e);
  if (const char* e = getenv("DISTR_XCHG_TS")) ctx->xchg_ts = atoi(e) != 0;
  if (const char* e = getenv("DISTR_CLUSTER_TEST_ABORT")) ctx->cluster_test_abort = atoi(e);     // 1: abort at assembly; 2: member 0 drops out behind its last slice
  if (const char* e = getenv("DISTR_SAVE_MASKS")) ctx->save_masks = atoi(e) != 0;
  for (const char* name : {"DISTR_DENSE_COMPACT", "DISTR_COMPACT32"})
    if (const char* e = getenv(name)) {
      if (strcmp(e, "0") != 0 && strcmp(e, "1") != 0) {
        ctx->err = std::string(name) + " must be 0 or 1 (got '" + e + "')";
        *out = ctx;
        return DISTR_ERR_INVALID_ARG;
      }
      (strcmp(name, "DISTR_COMPACT32") == 0 ? ctx->compact32 : ctx->dense_compact) = e[0] == '1';
    }
  for (const char* name : {"DISTR_LIVE_ORDER", "DISTR_RAY_BLOCKS"})
    if (const char* e = getenv(name)) {
      if (strcmp(e, "0") != 0 && strcmp(e, "1") != 0) {
        ctx->err = std::string(name) + " must be 0 or 1 (got '" + e + "')";
        *out = ctx;
        return DISTR_ERR_INVALID_ARG;
      }
      (strcmp(name, "DISTR_LIVE_ORDER") == 0 ? ctx->live_order : ctx->ray_blocks) = e[0] == '1';
    }
  if (const char* e = getenv("DISTR_STICKY")) ctx->sticky = atoi(e) != 0;
  if (const char* e = getenv("DISTR_XCHG_SC1")) ctx->xchg_sc1 = atoi(e) != 0;
  if (const char* e = getenv("DISTR_CLUSTER_SPREAD")) ctx->cluster_spread = atoi(e) != 0;
  if (const char* e = getenv("DISTR_TAIL")) ctx->tail = atoi(e) != 0;
  if (const char* e = getenv("DISTR_TAIL_PX")) ctx->tail_px = atoi(e);
  if (const char* e = getenv("DISTR_TAIL_RAYS")) ctx->tail_rays = atoi(e);
  if (const char* e = getenv("DISTR_TAIL_FROM")) ctx->tail_force = atoi(e);
  if (const char* e = getenv("DISTR_TAIL_TEST_ABSENT")) ctx->tail_absent = atoi(e);
  {
    // invariants of the tile-size split (fine_split and the host-side grid sizes rely on them): multiples of 64,
    // 64 <= t16 <= t32, and t16 + t32 below one full round (16384 rays) so that "remainder" ranges never reach a round
    const int t32 = ctx->hybrid_threshold, t16 = std::min(ctx->tail16_threshold, ctx->hybrid_threshold);
    if (t32 < 64 || t16 < 64 || (t32 & 63) || (ctx->tail16_threshold & 63) || t32 + t16 >= 16384) {
      ctx->err = "DISTR_HYBRID_THRESHOLD / DISTR_TAIL16_THRESHOLD must be multiples of 64 with 64 <= tail16, 64 <= hybrid and "
                 "min(tail16, hybrid) + hybrid < 16384 (got hybrid " + std::to_string(ctx->hybrid_threshold) + ", tail16 " +
                 std::to_string(ctx->tail16_threshold) + ")";
      *out = ctx;
      return DISTR_ERR_INVALID_ARG;
    }
  }
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || hip_device < 0 || hip_device >= n) {
    // keep the context so the caller can read the message
    ctx->err = std::string("no usable HIP device ") + std::to_string(hip_device) + " (" + (e == hipSuccess ? "count=" + std::to_string(n) : hipGetErrorString(e)) + ")";
    *out = ctx;
    return DISTR_ERR_HIP;
  }
  *out = ctx;
  return DISTR_OK;
}

void distr_destroy(distr_ctx* ctx) {
  if (!ctx) return;
  if (ctx->dec_buf) { (void)hipSetDevice(ctx->device); (void)hipFree(ctx->dec_buf); }
  if (ctx->dec_buf_color) { (void)hipSetDevice(ctx->device); (void)hipFree(ctx->dec_buf_color); }
  if (ctx->dec_buf_split) { (void)hipSetDevice(ctx->device); (void)hipFree(ctx->dec_buf_split); }
  for (auto& r : ctx->xr) { if (r.buf) (void)hipFree(r.buf); if (r.flags) (void)hipFree(r.flags); }
  if (ctx->hint_host) (void)hipHostFree(ctx->hint_host);
  for (auto& p : ctx->ev_pool) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
  delete ctx;
}

const char* distr_last_error(const distr_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// Packs one DeepSDF-8x512-shaped decoder for the tile kernels. nlat = latent length (the latent columns of lin0 / lin4 are
// folded into per-call constants, so the tile itself never sees them); rows3 = real rows of lin3 (509 - C for an SDF decoder of code
// length C, 253 for the colour decoder); nout = rows of lin8 (1: SDF, 3: colour). Narrow layout (rows3 <= 253): the tile's lin3 has
// 256 rows: the real ones, zero rows up to 253 (ReLU(0) = 0, and they meet zero lin4 columns, so values stay exact), xyz at 253..255 --
// lin4's K stays 256. Wide layout (rows3 > 253, code length < 256): lin3 has 512 rows the same way (real, zero up to 509, xyz at
// 509..511) and lin4 K = 512. The split-bf16 / split-f16 planes are packed for C = 256 only (the only decoders they may run).
static int build_decoder(distr_ctx* ctx, int nlat, int rows3, int nout, const float* w, size_t n_floats, float** dev_buf, DecoderDev& D,
                         DecoderDev16* D16, DecoderSplit* planes = nullptr, uint32_t** dev_buf_split = nullptr,
                         bool* h3_ok = nullptr, bool compact = false, std::string* h3_why = nullptr) {
  if (rows3 < 1 || rows3 > 509) return fail(ctx, DISTR_ERR_UNSUPPORTED, "lin3 with %d rows does not fit the 509-row tile", rows3);
  const bool wide = rows3 > 253;
  const int R3 = wide ? 509 : 253;         // row of lin3's output (and column of lin4) where xyz is carried
  const int in0 = nlat + 3, in4 = rows3 + nlat + 3;
  const int OUT[9] = {512, 512, 512, rows3, 512, 512, 512, 512, nout};
  const int IN[9] = {in0, 512, 512, 512, in4, 512, 512, 512, 512};
  size_t need = 0;
  for (int l = 0; l < 9; ++l) need += (size_t)OUT[l] * IN[l] + OUT[l];
  if (n_floats != need) return fail(ctx, DISTR_ERR_INVALID_ARG, "weight buffer has %zu floats, expected %zu", n_floats, need);
  const float* W[9]; const float* b[9];
  const float* p = w;
  for (int l = 0; l < 9; ++l) { W[l] = p; p += (size_t)OUT[l] * IN[l]; b[l] = p; p += OUT[l]; }

  // padded dense matrices [O][K] of the eight MFMA layers
  const int Kp[8] = {8, 512, 512, 512, wide ? 512 : 256, 512, 512, 512};
  const int Op[8] = {512, 512, 512, wide ? 512 : 256, 512, 512, 512, 512};
  std::vector<std::vector<float>> Wp(8);
  for (int l = 0; l < 8; ++l) Wp[l].assign((size_t)Op[l] * Kp[l], 0.f);
  for (int o = 0; o < 512; ++o) for (int k = 0; k < 3; ++k) Wp[0][(size_t)o * 8 + k] = W[0][(size_t)o * in0 + nlat + k];
  for (int l : {1, 2, 5, 6, 7}) memcpy(Wp[l].data(), W[l], sizeof(float) * 512 * 512);
  for (int o = 0; o < rows3; ++o) memcpy(&Wp[3][(size_t)o * 512], &W[3][(size_t)o * 512], sizeof(float) * 512);
  for (int o = 0; o < 512; ++o) {
    for (int k = 0; k < rows3; ++k) Wp[4][(size_t)o * Kp[4] + k] = W[4][(size_t)o * in4 + k];
    for (int k = 0; k < 3; ++k) Wp[4][(size_t)o * Kp[4] + R3 + k] = W[4][(size_t)o * in4 + rows3 + nlat + k];
  }

  std::vector<float> host;
  auto reserve = [&](size_t n) { size_t off = (host.size() + 63) & ~(size_t)63; host.resize(off + n, 0.f); return off; };
  size_t offWf[8], offWb[8] = {0}, offB[8] = {0};
  for (int l = 0; l < 8; ++l) {
    offWf[l] = reserve(Wp[l].size());
    pack_fragments(Wp[l].data(), Kp[l], Op[l], host.data() + offWf[l]);
  }
  auto transposed = [&](int l) {   // Wp[l] as [K][O]: the backward dX chain multiplies by it (K' = Op[l], O' = Kp[l])
    std::vector<float> Wt((size_t)Kp[l] * Op[l]);
    for (int o = 0; o < Op[l]; ++o) for (int k = 0; k < Kp[l]; ++k) Wt[(size_t)k * Op[l] + o] = Wp[l][(size_t)o * Kp[l] + k];
    return Wt;
  };
  for (int l = 1; l < 8; ++l) {
    const std::vector<float> Wt = transposed(l);
    offWb[l] = reserve(Wt.size());
    pack_fragments(Wt.data(), /*K'=*/Op[l], /*O'=*/Kp[l], host.data() + offWb[l]);
  }
  size_t offWk = 0, offWkb = 0;
  compact = compact && !wide;     // the compacted tile exists in the narrow layout only
  if (compact) {
    offWk = reserve(WK_FLOATS);
    for (int l = 1; l < 8; ++l) pack_kmajor(Wp[l].data(), Kp[l], Op[l], host.data() + offWk + wk_offset(l));
    // the same pack of the transposed matrices (backward dX chain: K' = Op[l], O' = Kp[l]; lin3^T and lin4^T swap their sizes, so layer l
    // keeps its offset)
    offWkb = reserve(WK_FLOATS);
    for (int l = 1; l < 8; ++l) {
      const std::vector<float> Wt = transposed(l);
      pack_kmajor(Wt.data(), /*K'=*/Op[l], /*O'=*/Kp[l], host.data() + offWkb + wk_offset(l));
    }
  }
  size_t offW16[8];
  for (int l = 0; l < 8; ++l) {
    const int K16 = (l == 0) ? 16 : Kp[l];
    std::vector<float> W16((size_t)Op[l] * K16, 0.f);
    for (int o = 0; o < Op[l]; ++o) for (int k = 0; k < Kp[l]; ++k) W16[(size_t)o * K16 + k] = Wp[l][(size_t)o * Kp[l] + k];
    offW16[l] = reserve(W16.size());
    pack_fragments16(W16.data(), K16, Op[l], host.data() + offW16[l]);
  }
  for (int l : {1, 2, 3, 5, 6, 7}) {
    offB[l] = reserve(Op[l]);
    memcpy(host.data() + offB[l], b[l], sizeof(float) * OUT[l]);
  }
  const size_t o_W0lat_t = reserve((size_t)nlat * HID), o_W4lat_t = reserve((size_t)nlat * HID);
  const size_t o_W0lat = reserve((size_t)HID * nlat), o_W4lat = reserve((size_t)HID * nlat);
  for (int o = 0; o < HID; ++o) for (int k = 0; k < nlat; ++k) {
    const float v0 = W[0][(size_t)o * in0 + k], v4 = W[4][(size_t)o * in4 + rows3 + k];
    host[o_W0lat_t + (size_t)k * HID + o] = v0; host[o_W0lat + (size_t)o * nlat + k] = v0;
    host[o_W4lat_t + (size_t)k * HID + o] = v4; host[o_W4lat + (size_t)o * nlat + k] = v4;
  }
  const size_t o_b0 = reserve(HID), o_b4 = reserve(HID), o_w8 = reserve((size_t)nout * HID), o_W0x = reserve(3 * HID);
  memcpy(host.data() + o_b0, b[0], sizeof(float) * HID);
  memcpy(host.data() + o_b4, b[4], sizeof(float) * HID);
  memcpy(host.data() + o_w8, W[8], sizeof(float) * nout * HID);
  for (int o = 0; o < HID; ++o) for (int k = 0; k < 3; ++k) host[o_W0x + (size_t)k * HID + o] = W[0][(size_t)o * in0 + nlat + k];

  if (*dev_buf) { HIP_TRY(hipFree(*dev_buf)); *dev_buf = nullptr; }       // (the entry point's guard made ctx->device current)
  HIP_TRY(hipMalloc((void**)dev_buf, host.size() * sizeof(float)));
  HIP_TRY(hipMemcpy(*dev_buf, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  const float* d = *dev_buf;
  for (int l = 0; l < 8; ++l) { D.Wf[l] = d + offWf[l]; D.Wb[l] = l ? d + offWb[l] : nullptr; D.bias[l] = (l == 0 || l == 4) ? nullptr : d + offB[l]; }
  D.W0lat_t = d + o_W0lat_t; D.W4lat_t = d + o_W4lat_t; D.W0lat = d + o_W0lat; D.W4lat = d + o_W4lat;
  D.b0 = d + o_b0; D.b4 = d + o_b4; D.w8 = d + o_w8; D.W0x = d + o_W0x;
  D.b8 = b[8][0];
  D.b8x[0] = nout > 1 ? b[8][1] : 0.f; D.b8x[1] = nout > 2 ? b[8][2] : 0.f;
  D.nlat = nlat;
  D.Wk = compact ? d + offWk : nullptr;
  D.Wkb = compact ? d + offWkb : nullptr;
  if (D16) for (int l = 0; l < 8; ++l) D16->Wf[l] = d + offW16[l];
#ifdef DISTR_DIAG
  // DIAGNOSTICS BUILDS ONLY (-DDISTR_DIAG; values are wrong): every 512 x 512 layer of the 16-ray / cluster tiles reads lin1's fragments, so
  // that their weight stream (2 MB instead of 6.3 MB) stays in one XCD's 4 MiB L2 -- separates "waiting for weights" from "issuing
  // instructions" in the tail. Not in the product library: an environment variable must never be able to change a render's values.
  if (D16 && getenv("DISTR_DEBUG_ALIAS_WEIGHTS")) {
    fprintf(stderr, "distr: DISTR_DEBUG_ALIAS_WEIGHTS is set -- the 16-ray / cluster tiles compute with the WRONG weights (timing diagnostics only)\n");
    for (int l : {2, 5, 6, 7}) D16->Wf[l] = D16->Wf[1];
  }
#endif
  if (planes) {   // split planes of lin1..lin7 and of their transposes (backward dX chain: K' = Op[l], O' = Kp[l]) for the opt-in arithmetic
    std::vector<uint16_t> hb;   // modes: bf16x6 2 x 9.4 MB, f16x3 2 x 6.3 MB, own allocation
    size_t off[2][2][8] = {};   // [format][transposed][layer]
    bool fits[2][8] = {};       // [format][layer]: every weight stayed inside the format's range
    auto pack = [&](int f, int NP, auto split) {
      for (int t = 0; t < 2; ++t)
        for (int l = 1; l < 8; ++l) {
          const std::vector<float> W = t ? transposed(l) : std::vector<float>();
          off[f][t][l] = (hb.size() + 127) & ~(size_t)127;
          hb.resize(off[f][t][l] + Wp[l].size() * NP, 0);
          const bool ok = pack_fragments_split(t ? W.data() : Wp[l].data(), t ? Op[l] : Kp[l], t ? Kp[l] : Op[l], NP, split, hb.data() + off[f][t][l]);
          if (!t) fits[f][l] = ok;
        }
    };
    pack(0, FmtB6::NP, split_bf16x3);
    pack(1, FmtH3::NP, split_f16x2);
    *h3_ok = true;
    for (int l = 1; l < 8; ++l) {
      // the accepted range of the f16x3 mode, per layer and on both sides (distr_mlp_split.hpp: H3_WMAX, H3_WMIN)
      float wmax = 0.f;
      for (float v : Wp[l]) wmax = fmaxf(wmax, fabsf(v));
      const bool high = !fits[1][l] || !(wmax < H3_WMAX), low = wmax < H3_WMIN;
      if ((high || low) && *h3_ok) {
        *h3_ok = false;
        if (h3_why) {
          char msg[200];
          if (high) snprintf(msg, sizeof(msg), "lin%d's largest |weight| %g times %g leaves the f16 range (the bound is %g)", l, (double)wmax, (double)FmtH3::SW, (double)H3_WMAX);
          else snprintf(msg, sizeof(msg), "lin%d's largest |weight| %g is below %g: its outputs' second f16 plane falls into the denormals and accuracy is lost silently", l, (double)wmax, (double)H3_WMIN);
          *h3_why = msg;
        }
      }
    }
    if (*dev_buf_split) { HIP_TRY(hipFree(*dev_buf_split)); *dev_buf_split = nullptr; }
    HIP_TRY(hipMalloc((void**)dev_buf_split, hb.size() * sizeof(uint16_t)));
    HIP_TRY(hipMemcpy(*dev_buf_split, hb.data(), hb.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    for (int f = 0; f < 2; ++f) {
      planes[f].Wp[0] = nullptr; planes[f].Wb[0] = nullptr;
      for (int l = 1; l < 8; ++l) {
        planes[f].Wp[l] = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint16_t*>(*dev_buf_split) + off[f][0][l]);
        planes[f].Wb[l] = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint16_t*>(*dev_buf_split) + off[f][1][l]);
      }
    }
  }
  return DISTR_OK;
}

int distr_set_decoder(distr_ctx* ctx, const distr_decoder_desc* desc, const float* w, size_t n_floats) {
  if (!ctx || !desc || !w) return fail(ctx, DISTR_ERR_INVALID_ARG, "null argument");
  EntryGuard guard_(ctx);
  if (desc->struct_size != sizeof(distr_decoder_desc)) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_decoder_desc.struct_size is %u, expected %zu", desc->struct_size, sizeof(distr_decoder_desc));
  if (desc->latent_size < 1 || desc->latent_size > MAX_LAT || desc->hidden != HID || desc->num_linear != 9 || desc->latent_in != 4)
    return fail(ctx, DISTR_ERR_UNSUPPORTED, "decoder (latent %d, hidden %d, %d linears, latent_in %d) unsupported: kernels are "
                "specialised for DeepSDF 8x512 with latent_in=[4] and a code length of 1..%d", desc->latent_size, desc->hidden,
                desc->num_linear, desc->latent_in, MAX_LAT);
  const int nlat = desc->latent_size;
  int rc;
  if (nlat == LAT) {
    rc = build_decoder(ctx, nlat, 509 - nlat, 1, w, n_floats, &ctx->dec_buf, ctx->D, &ctx->D16, ctx->planes, &ctx->dec_buf_split, &ctx->h3_ok, ctx->dense_compact, &ctx->h3_why);
  } else {   // no split-arithmetic planes: bf16x6 / f16x3 refuse other code lengths (check_cfg, distr_mlp_eval_*)
    rc = build_decoder(ctx, nlat, 509 - nlat, 1, w, n_floats, &ctx->dec_buf, ctx->D, &ctx->D16, nullptr, nullptr, nullptr, ctx->dense_compact);
    if (!rc && ctx->dec_buf_split) { HIP_TRY(hipFree(ctx->dec_buf_split)); ctx->dec_buf_split = nullptr; ctx->planes[0] = ctx->planes[1] = DecoderSplit{}; ctx->h3_ok = false; }
  }
  if (rc) return rc;
  ctx->has_decoder = true;
  return DISTR_OK;
}

int distr_set_color_decoder(distr_ctx* ctx, const distr_decoder_desc* desc, const float* w, size_t n_floats) {
  if (!ctx || !desc || !w) return fail(ctx, DISTR_ERR_INVALID_ARG, "null argument");
  EntryGuard guard_(ctx);
  if (desc->struct_size != sizeof(distr_decoder_desc)) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_decoder_desc.struct_size is %u, expected %zu", desc->struct_size, sizeof(distr_decoder_desc));
  if (desc->latent_size <= LAT || desc->latent_size > 4096 || desc->hidden != HID || desc->num_linear != 9 || desc->latent_in != 4)
    return fail(ctx, DISTR_ERR_UNSUPPORTED, "colour decoder (latent %d, hidden %d, %d linears, latent_in %d) unsupported: expected the "
                "DeepSDF 8x512 shape with latent = 256 + color_size and last_dim = 3", desc->latent_size, desc->hidden, desc->num_linear, desc->latent_in);
  int rc = build_decoder(ctx, desc->latent_size, 253, 3, w, n_floats, &ctx->dec_buf_color, ctx->DC, nullptr);
  if (rc) return rc;
  ctx->has_color = true;
  return DISTR_OK;
}

}  // extern "C"

// ---- the colour decoder on a point list, plain or segmented: distr_color_eval / _backward, their *_multi forms, the colour stage of a batch
namespace {

// the two ways to a list of the colour decoder; the caller holds the EntryGuard
int color_plain_list(distr_ctx* ctx, int64_t n, bool backward, PointList& pl) {
  if (!ctx->has_color) return fail(ctx, DISTR_ERR_NO_DECODER, "distr_set_color_decoder has not been called");
  pl = plain_list(n);
  pl.bad_args = "null device pointer"; pl.small_ws = backward ? "colour backward workspace too small" : "colour workspace too small";
  return DISTR_OK;
}

int color_seg_list(distr_ctx* ctx, int32_t nseg, const int64_t* counts, int64_t latent_stride, PointList& pl) {
  if (int rc = seg_list(ctx, nseg, counts, pl)) return rc;
  if (!ctx->has_color) return fail(ctx, DISTR_ERR_NO_DECODER, "distr_set_color_decoder has not been called");
  if (latent_stride != 0 && latent_stride < ctx->DC.nlat) return fail(ctx, DISTR_ERR_INVALID_ARG, "latent_stride %lld: 0 (shared code) or >= %d", (long long)latent_stride, ctx->DC.nlat);
  return DISTR_OK;
}

// the two launches on a list whose workspace is carved and whose constants and tile table are written
int color_eval_launch(distr_ctx* ctx, const PointList& pl, const float* xyz, float* rgb, hipStream_t s) {
  hipLaunchKernelGGL(k_color, dim3(pl.tiles), dim3(NTHREADS), 0, s, xyz, pl.nseg ? (int64_t)0 : pl.n, (const float*)pl.c0c4, rgb, ctx->DC, (const SegTable*)pl.tab);
  LAUNCH_CHECK("k_color");
  return DISTR_OK;
}

int color_bwd_launch(distr_ctx* ctx, const PointList& pl, const float* xyz, const float* g_rgb, float* g_xyz, hipStream_t s) {
  hipLaunchKernelGGL(k_color_bwd, dim3(pl.tiles), dim3(NTHREADS), 0, s, xyz, pl.nseg ? (int64_t)0 : pl.n, (const float*)pl.c0c4, g_rgb, g_xyz, pl.partial, ctx->DC,
                     (const SegTable*)pl.tab);
  LAUNCH_CHECK("k_color_bwd");
  return DISTR_OK;
}

int color_eval_list(distr_ctx* ctx, PointList& pl, const float* latent_cat, int64_t latent_stride, const float* xyz, float* rgb, void* ws, size_t ws_bytes,
                    hipStream_t s) {
  const int rc = point_list_prologue(ctx, ctx->DC, pl, latent_cat, latent_stride, xyz && rgb, ws, ws_bytes, false, s);
  if (rc || pl.n == 0) return rc;
  return color_eval_launch(ctx, pl, xyz, rgb, s);
}

int color_backward_list(distr_ctx* ctx, PointList& pl, const float* latent_cat, int64_t latent_stride, const float* xyz, const float* g_rgb, float* g_xyz,
                        float* g_latent_cat, void* ws, size_t ws_bytes, hipStream_t s) {
  int rc = point_list_prologue(ctx, ctx->DC, pl, latent_cat, latent_stride, xyz && g_rgb, ws, ws_bytes, true, s);
  if (rc) return rc;
  if (pl.n > 0 && (rc = color_bwd_launch(ctx, pl, xyz, g_rgb, g_xyz, s))) return rc;
  return list_latent_grad(ctx, ctx->DC, pl, g_latent_cat, s);
}

}  // namespace

extern "C" {

int distr_color_eval(distr_ctx* ctx, const float* latent_cat, const float* xyz, int64_t n, float* rgb, void* ws, size_t ws_bytes,
                     void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  PointList pl;
  if (int rc = color_plain_list(ctx, n, false, pl)) return rc;
  return color_eval_list(ctx, pl, latent_cat, 0, xyz, rgb, ws, ws_bytes, (hipStream_t)stream);
}

int distr_color_backward(distr_ctx* ctx, const float* latent_cat, const float* xyz, int64_t n, const float* g_rgb, float* g_xyz,
                         float* g_latent_cat, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  PointList pl;
  if (int rc = color_plain_list(ctx, n, true, pl)) return rc;
  return color_backward_list(ctx, pl, latent_cat, 0, xyz, g_rgb, g_xyz, g_latent_cat, ws, ws_bytes, (hipStream_t)stream);
}

size_t distr_color_multi_workspace_bytes(int32_t nseg, const int64_t* counts_host) {
  PointList pl;
  return seg_list(nullptr, nseg, counts_host, pl) == DISTR_OK ? carve_list(nullptr, pl, false) : 0;
}

size_t distr_color_backward_multi_workspace_bytes(int32_t nseg, const int64_t* counts_host) {
  PointList pl;
  return seg_list(nullptr, nseg, counts_host, pl) == DISTR_OK ? carve_list(nullptr, pl, true) : 0;
}

int distr_color_eval_multi(distr_ctx* ctx, int32_t nseg, const int64_t* counts_host, const float* latent_cat, int64_t latent_stride, const float* xyz,
                           float* rgb, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  PointList pl;
  if (int rc = color_seg_list(ctx, nseg, counts_host, latent_stride, pl)) return rc;
  return color_eval_list(ctx, pl, latent_cat, latent_stride, xyz, rgb, ws, ws_bytes, (hipStream_t)stream);
}

int distr_color_backward_multi(distr_ctx* ctx, int32_t nseg, const int64_t* counts_host, const float* latent_cat, int64_t latent_stride,
                               const float* xyz, const float* g_rgb, float* g_xyz, float* g_latent_cat, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  PointList pl;
  if (int rc = color_seg_list(ctx, nseg, counts_host, latent_stride, pl)) return rc;
  return color_backward_list(ctx, pl, latent_cat, latent_stride, xyz, g_rgb, g_xyz, g_latent_cat, ws, ws_bytes, (hipStream_t)stream);
}

int distr_workspace_bytes(distr_ctx* ctx, const distr_render_cfg* cfg, size_t* fwd, size_t* bwd) {
  int rc = check_cfg(ctx, cfg);
  if (rc) return rc;
  View V;
  if (fwd) *fwd = make_view(*cfg, nullptr, V, ctx->save_masks);
  if (bwd) *bwd = bwd_bytes(*cfg);
  return DISTR_OK;
}

namespace {

inline int32_t cfg_view_flags(const distr_render_cfg& c) {
  return (c.grad_depth ? VF_GRAD_DEPTH : 0) | (c.grad_mask ? VF_GRAD_MASK : 0) | (c.grad_camera ? VF_GRAD_CAMERA : 0);
}

// per-view gradient switches of a batch: null -> every view uses cfg's; a view may only switch OFF what cfg has on (the
// workspace layout, e.g. whether ReLU masks are saved, follows cfg)
int make_view_flags(distr_ctx* ctx, const distr_render_cfg& c, int nviews, const int32_t* view_flags, ViewFlags& vf) {
  memset(&vf, 0, sizeof(vf));
  const int32_t all = cfg_view_flags(c);
  for (int b = 0; b < nviews; ++b) {
    const int32_t f = view_flags ? view_flags[b] : all;
    if (f & ~all) return fail(ctx, DISTR_ERR_INVALID_ARG, "view_flags[%d] = %d enables a gradient that cfg (flags %d) has off", b, f, all);
    vf.f[b] = (uint8_t)f;
  }
  return DISTR_OK;
}

inline int64_t pad_to(int64_t v, int64_t g) { return (v + g - 1) / g * g; }
inline int32_t up8(int64_t v) { return (int32_t)((v + 7) / 8 * 8); }

// ---- The variants of k_step, k_tail, k_march, k_march16 and k_bwd: distr_inst.hpp lists them. What the list holds, and what the callers
// below therefore settle before they ask for one:
//   * the wide layout (code length < 256) exists in f32 on 64-ray / 64- and 32-sample tiles only: no k_step, k_tail or k_march16, so wide
//     decoders render launch-per-step without tail launch, cluster, sticky, 16- or 32-ray tiles (those generated loops are laid out for
//     the narrow lin3); values are the same, only the schedule differs;
//   * the split arithmetics (1 bf16x6, 2 f16x3) have no 16-ray role (k_march16 and k_tail are f32 only), no MODE_EVAL tiles, and their
//     backward is the one over saved masks; check_cfg admits them for code length 256 only, so never together with wide.
// A launcher looks the requested variant up in the list, launches it and checks the launch (`what` names it in the error text). A
// combination without a line in the list is refused: no other instantiation is ever named, so this unit holds none of their code.
inline bool wide_decoder(const distr_ctx* ctx) { return ctx->D.nlat < LAT; }

#define DISTR_LAUNCH_IF(cond, kernel, ...) \
  if (cond) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(NTHREADS), 0, s, __VA_ARGS__); LAUNCH_CHECK(what); return DISTR_OK; }
// per family: which run-time values select a line of the list, and the kernel's arguments
#define DISTR_TRY_STEP(K, AR, C) DISTR_LAUNCH_IF(keep == K && arith == AR && compact == C, (k_step<K, AR, C>), A, ctx->D, ctx->D16, G)
#define DISTR_TRY_TAIL(K) DISTR_LAUNCH_IF(keep == K, (k_tail<K>), A, ctx->D, ctx->D16)
#define DISTR_TRY_MARCH(M, RB, K, AR, W, C) \
  DISTR_LAUNCH_IF(mode == M && rb == RB && keep == K && arith == AR && wide == W && compact == C, (k_march<M, RB, K, AR, W, C>), A, ctx->D)
#define DISTR_TRY_MARCH16(M, K) DISTR_LAUNCH_IF(mode == M && keep == K, (k_march16<M, K>), A, ctx->D, ctx->D16)
#define DISTR_TRY_BWD(M, RB, AR, W, C) \
  DISTR_LAUNCH_IF(mode == M && rb == RB && arith == AR && wide == W && compact == C, (k_bwd<M, RB, AR, W, C>), B, ctx->D)

// The compacted 64-ray tile (DISTR_DENSE_COMPACT) is a column of the lists: taken wherever the exact-f32 64-ray tile of the narrow layout
// runs and the context packed the k-major weights for it (D.Wk); every other tile keeps the dense loop.
inline bool compact_tile(const distr_ctx* ctx, int rb, int arith) { return ctx->D.Wk != nullptr && rb == 2 && arith == 0; }

// k_step's compaction level: 1 = its 64-ray role walks live units, 2 = its 32-ray role too (DISTR_COMPACT32, on top of DISTR_DENSE_COMPACT)
inline int step_compact_level(const distr_ctx* ctx, int arith) { return compact_tile(ctx, 2, arith) ? (ctx->compact32 ? 2 : 1) : 0; }

int launch_step(distr_ctx* ctx, const char* what, bool keep, int arith, unsigned grid, hipStream_t s, const MarchArgs& A, const StepGrid& G) {
  const int compact = step_compact_level(ctx, arith);
  DISTR_ALL_GROUPS(DISTR_TRY_STEP, DISTR_NO_VARIANT, DISTR_NO_VARIANT, DISTR_NO_VARIANT, DISTR_NO_VARIANT)
  return fail(ctx, DISTR_ERR_UNSUPPORTED, "no variant k_step<%d, %d, %d> (distr_inst.hpp)", (int)keep, arith, compact);
}

int launch_tail(distr_ctx* ctx, const char* what, bool keep, unsigned grid, hipStream_t s, const MarchArgs& A) {
  DISTR_ALL_GROUPS(DISTR_NO_VARIANT, DISTR_TRY_TAIL, DISTR_NO_VARIANT, DISTR_NO_VARIANT, DISTR_NO_VARIANT)
  return fail(ctx, DISTR_ERR_UNSUPPORTED, "no variant k_tail<%d> (distr_inst.hpp)", (int)keep);
}

int launch_march(distr_ctx* ctx, const char* what, int mode, int rb, bool keep, int arith, bool wide, unsigned grid, hipStream_t s, const MarchArgs& A) {
  const bool compact = compact_tile(ctx, rb, arith);      // (D.Wk is not packed for the wide layout)
  DISTR_ALL_GROUPS(DISTR_NO_VARIANT, DISTR_NO_VARIANT, DISTR_TRY_MARCH, DISTR_NO_VARIANT, DISTR_NO_VARIANT)
  return fail(ctx, DISTR_ERR_UNSUPPORTED, "no variant k_march<%d, %d, %d, %d, %d, %d> (distr_inst.hpp)", mode, rb, (int)keep, arith, (int)wide, (int)compact);
}

int launch_march16(distr_ctx* ctx, const char* what, int mode, bool keep, unsigned grid, hipStream_t s, const MarchArgs& A) {
  DISTR_ALL_GROUPS(DISTR_NO_VARIANT, DISTR_NO_VARIANT, DISTR_NO_VARIANT, DISTR_TRY_MARCH16, DISTR_NO_VARIANT)
  return fail(ctx, DISTR_ERR_UNSUPPORTED, "no variant k_march16<%d, %d> (distr_inst.hpp)", mode, (int)keep);
}

int launch_bwd(distr_ctx* ctx, const char* what, int mode, int rb, int arith, bool wide, unsigned grid, hipStream_t s, const BwdArgs& B) {
  // the compacted backward: the 64-sample tile over saved masks only (BWD_FULL / BWD_POINTGRAD recompute the forward and keep the dense loop)
  const bool compact = mode == BWD_SAVED && !wide && compact_tile(ctx, rb, arith) && ctx->D.Wkb != nullptr;
  DISTR_ALL_GROUPS(DISTR_NO_VARIANT, DISTR_NO_VARIANT, DISTR_NO_VARIANT, DISTR_NO_VARIANT, DISTR_TRY_BWD)
  return fail(ctx, DISTR_ERR_UNSUPPORTED, "no variant k_bwd<%d, %d, %d, %d, %d> (distr_inst.hpp)", mode, rb, arith, (int)wide, (int)compact);
}

// What a forward render has decided before its first march launch.
struct RenderPlan {
  int t16, t32;                 // largest remainders (rays) that run on 16- / 32-ray tiles (t16 = 0: no 16-ray role)
  bool wide;                    // wide_decoder(): 64-ray tiles, one launch per step
  bool b6, h3;                  // split-bf16 / split-f16 tiles (h3 implies b6): 64- and 32-ray roles only, no cluster tiles
  bool recursive;               // live-ray lists + tile-size split (fine_split)
  distr_ctx::XRegion* xr;       // exchange region of the cluster tiles, or null
  int arith() const { return h3 ? DISTR_ARITH_F16X3 : b6 ? DISTR_ARITH_BF16X6 : DISTR_ARITH_F32; }
};

// persistent tail launch: from which full-resolution step on (see distr_ctx::tail); sets V.tail_from, returns the device word k_finalize
// writes the next render's hint to (or null)
int32_t* choose_tail_from(distr_ctx* ctx, View& V, hipStream_t s) {
  int32_t* hint_dev = nullptr;
  if (V.cfg.marcher == DISTR_MARCH_TRIVIAL || V.cfg.arith != DISTR_ARITH_F32 || !ctx->tail || V.cfg.concurrent || ctx->tail16_threshold <= 0 ||
      wide_decoder(ctx))
    return hint_dev;
  if (ctx->debug_steps >= 0) return nullptr;      // (distr_debug_live_list: one launch per step, a pack behind each, no hint read or written)
  int32_t* hint = tail_hint_slot(ctx, V.cfg, V.nviews, is_capturing(s), &hint_dev);
  if (ctx->tail_force >= 0) V.tail_from = std::min(ctx->tail_force, V.fine_steps);
  else if ((int64_t)V.nviews * V.P <= ctx->tail_px) V.tail_from = 0;
  else if (hint) {
    const int32_t h = __atomic_load_n(hint, __ATOMIC_RELAXED);
    if (h >= 0 && h + 2 <= V.fine_steps) V.tail_from = h;      // (nothing to gain from a tail of one step)
  }
  if (hint) {
    // the previous render's first step without rounds, plus one step of margin: behind it no k_live_pack is launched
    const int32_t o = __atomic_load_n(hint + distr_ctx::NHINT, __ATOMIC_RELAXED);
    if (o >= 0) V.order_until = std::min(o + 1, V.fine_steps);
  }
  return hint_dev;
}

int setup_levels(distr_ctx* ctx, const View& V, const float* latent, int64_t lat_stride, const float* R, const float* T, const ViewFlags& vf,
                 hipStream_t s) {
  hipLaunchKernelGGL(k_prep, dim3(4, (unsigned)V.nviews), dim3(256), 0, s, V, ctx->D, latent, lat_stride, R, T, vf);
  LAUNCH_CHECK("k_prep");
  for (int l = 0; l < V.nlev; ++l) {
    hipLaunchKernelGGL(k_setup_level, grid_setup(V, V.lv[l].w, V.lv[l].h), dim3(256), 0, s, V, l);
    LAUNCH_CHECK("k_setup_level");
    if (V.band) {
      hipLaunchKernelGGL(k_maxinit_full, gridv(V, (int64_t)V.lv[l].full_h * V.lv[l].w), dim3(256), 0, s, V, l);
      LAUNCH_CHECK("k_maxinit_full");
    }
  }
  return DISTR_OK;
}

// the coarse levels of the pyramid, coarsest first: one march launch per step
int march_coarse(distr_ctx* ctx, const View& V, MarchArgs& A, const RenderPlan& p, MarchTimer& timer, hipStream_t s) {
  const int nviews = V.nviews;
  const bool keep = V.save_masks != 0;
  for (int l = V.nlev - 1; l >= 1; --l) {
    hipLaunchKernelGGL(k_coarse_init, gridv(V, V.lv[l].n), dim3(256), 0, s, V, l);
    LAUNCH_CHECK("k_coarse_init");
    for (int st = 0; st < V.lv[l].steps; ++st) {
      A.lvl = l; A.step = st; A.origin_tile = 0;
      // tile size of a coarse level from the (host-known) pixel count of all views: a level that fits one round of 16- / 32-ray
      // tiles runs on those (small images: 111 / 212 us per step instead of 380 us)
      const int64_t ln = V.lv[l].n;
      const bool c16 = !p.b6 && !p.wide && nviews * pad_to(ln, 16) <= p.t16;
      const int crb = (!p.wide && nviews * pad_to(ln, 32) <= p.t32) ? 1 : 2;
      const int ctile = c16 ? 16 : 32 * crb;
      unsigned tiles = (unsigned)nviews * (unsigned)((ln + ctile - 1) / ctile);
      A.xc = next_xchg(c16 ? p.xr : nullptr, s, ctx->xchg_ts, ctx->max_cl, ctx->cluster_test_abort, ctx->min_cl, 1, false, ctx->xchg_sc1);
      A.xc.spread = ctx->cluster_spread;
      if (c16 && p.xr) tiles = std::max(tiles, 256u);      // cluster tiles: up to 8 workgroups per 16 rays
      timer.begin();
      const int rc = c16 ? launch_march16(ctx, "k_march<coarse>", MODE_COARSE, keep, tiles, s, A)
                         : launch_march(ctx, "k_march<coarse>", MODE_COARSE, crb, keep, p.arith(), p.wide, tiles, s, A);
      if (rc) return rc;
      timer.end();
    }
  }
  return DISTR_OK;
}

// the full-resolution steps: a march launch per step ('trivial', wide decoders), or k_step per step up to tail_from and k_tail from there
int march_fine(distr_ctx* ctx, const View& V, MarchArgs& A, const RenderPlan& p, MarchTimer& timer, hipStream_t s) {
  const int nviews = V.nviews, P = V.P, t16 = p.t16, t32 = p.t32;
  const unsigned NV = (unsigned)nviews;
  const bool keep = V.save_masks != 0;
  hipLaunchKernelGGL(k_fine_init, grid_setup(V, V.lv[0].w, V.lv[0].h), dim3(256), 0, s, V);
  LAUNCH_CHECK("k_fine_init");
  // upper bounds of a step's live rays in the virtual concatenation of the views (every view padded to 16 / 64 rays)
  const int64_t N64 = (int64_t)nviews * pad_to(P, 64);
  for (int st = 0; st < V.fine_steps; ++st) {
    if (ctx->debug_steps >= 0 && st >= ctx->debug_steps) break;
    A.lvl = 0; A.step = st;
    timer.begin();
    if (st == V.tail_from) {
      // every remaining step inside this launch (k_tail): 256 workgroups, one per compute unit
      A.origin_tile = 1;
      A.xc = next_xchg(p.xr, s, ctx->xchg_ts, ctx->max_cl, ctx->cluster_test_abort, ctx->min_cl, (uint32_t)(V.fine_steps - st), ctx->sticky, ctx->xchg_sc1);
      A.xc.spread = ctx->cluster_spread;
      A.xc.t_go = TAIL_T_GO;
      A.tail_absent = ctx->tail_absent;
      if (int rc = launch_tail(ctx, "k_tail", keep, 256, s, A)) return rc;
      timer.end();
      break;
    }
    if (!p.recursive || p.wide) {
      // 'trivial': every in-sphere ray, every step, on 64-ray tiles. Wide decoders: also the recursive marchers' live-ray lists (t16 =
      // t32 = 0: fine_split hands every ray to the 64-ray role), f(origin) on the last step like k_step
      A.origin_tile = (p.recursive ? st == V.fine_steps - 1 : st == 0) ? 1 : 0;
      const unsigned tiles = NV * (unsigned)((P + 63) / 64) + (A.origin_tile ? NV : 0u);
      if (int rc = launch_march(ctx, "k_march<fine>", MODE_FINE, 2, keep, p.arith(), p.wide, tiles, s, A)) return rc;
      timer.end();
      continue;
    }
    // one launch per step: the three tile sizes are roles of the same grid (k_step, fine_split). Roles that are provably empty
    // from the pixel count alone get no workgroups: with N64 <= bound the remainder rules never reach the 64-ray role (bound <
    // one round, distr_create), with N64 <= t16 the 32-ray role stays empty too.
    const int64_t bound = (t16 < t32) ? (int64_t)t32 + t16 : t32;
    const bool skip64 = N64 <= bound;
    // ordered live list (step_ordered): only a step whose 64-ray role has work keeps it, only the compacted 64-ray tile gains from it
    A.live_order = (ctx->live_order && !skip64 && st + 1 < V.fine_steps && st < V.order_until && compact_tile(ctx, 2, p.arith())) ? 1 : 0;   // (the last step leaves no list anybody reads)
    const bool skip32 = t32 <= t16 || N64 <= t16;
    StepGrid G;
    G.n64 = skip64 ? 0 : std::min(up8(N64 / 64), 256);            // persistent: at most one 64-ray workgroup per CU
    A.origin_tile = (st == V.fine_steps - 1) ? 1 : 0;
    if (p.b6) {
      // split-bf16: no 16-ray role; the views' origin tiles (last step) close the 32-ray role's grid
      G.n32 = up8(std::min<int64_t>(N64, t32) / 32 + (A.origin_tile ? nviews : 0));
      G.n16 = 0;
      A.xc = next_xchg(nullptr, s, false, ctx->max_cl, 0, ctx->min_cl);
    } else {
      G.n32 = skip32 ? 0 : up8(std::min<int64_t>(N64, t32) / 32);
      A.xc = next_xchg(p.xr, s, ctx->xchg_ts, ctx->max_cl, ctx->cluster_test_abort, ctx->min_cl, (uint32_t)(V.fine_steps - st), ctx->sticky && !V.cfg.concurrent, ctx->xchg_sc1);
      A.xc.spread = ctx->cluster_spread;
      unsigned n16 = (unsigned)(std::min<int64_t>(N64, t16) / 16) + (A.origin_tile ? NV : 0u);
      if (p.xr) n16 = std::max(n16, 256u);                           // cluster tiles: 8 / 4 / 2 workgroups per tile of at most 32 / 64 / 128
      G.n16 = up8(n16);
    }
    if (int rc = launch_step(ctx, "k_step", keep, p.arith(), (unsigned)(G.n64 + G.n32 + G.n16), s, A, G)) return rc;
    timer.end();
    if (A.live_order) {
      // closes the gaps of the slots an ordered step left (the device decides from the step's count; behind any other step its workgroups
      // leave at once). Outside the timer's bracket: the profile lists march launches.
      hipLaunchKernelGGL(k_live_pack, dim3((unsigned)((P / 16 + PACK_CHUNKS) / PACK_CHUNKS), NV), dim3(256), 0, s, V, st, t16, t32);
      LAUNCH_CHECK("k_live_pack");
    }
  }
  return DISTR_OK;
}

int finalize_and_normals(distr_ctx* ctx, const View& V, bool wide, int32_t* hint_dev, float* zdepth, uint8_t* mask,
                         float* min_sdf, float* depth, float* normal, hipStream_t s) {
  const int P = V.P;
  hipLaunchKernelGGL(k_finalize, gridv(V, P), dim3(256), 0, s, V, zdepth, mask, min_sdf, depth, hint_dev, (int32_t)ctx->tail_rays,
                     (int32_t)((V.cfg.arith != DISTR_ARITH_F32) ? 0 : std::min(ctx->tail16_threshold, ctx->hybrid_threshold)), (int32_t)ctx->hybrid_threshold);
  LAUNCH_CHECK("k_finalize");
  if (!V.cfg.want_normal) return DISTR_OK;
  if (V.cfg.use_depth2normal) {
    hipLaunchKernelGGL(k_depth2normal, gridv(V, P), dim3(256), 0, s, V, depth, normal);
    LAUNCH_CHECK("k_depth2normal");
    return DISTR_OK;
  }
  if (normal) HIP_TRY(hipMemsetAsync(normal, 0, (size_t)V.nviews * P * 3 * sizeof(float), s));
  BwdArgs B;
  memset(&B, 0, sizeof(B));
  B.V = V; B.zdepth = V.zdepth_s; B.zstride = V.vstride;
  if (int rc = launch_bwd(ctx, "k_bwd<pointgrad>", BWD_POINTGRAD, 2, 0, wide, (unsigned)V.nviews * (unsigned)((P + 63) / 64), s, B)) return rc;
  hipLaunchKernelGGL(k_normal_finish, gridv(V, P), dim3(256), 0, s, V, normal, (float*)nullptr, 1);
  LAUNCH_CHECK("k_normal_finish");
  return DISTR_OK;
}

int render_forward_impl(distr_ctx* ctx, const distr_render_cfg* cfg, int nviews, const int32_t* view_flags, const float* latent,
                        int64_t lat_stride, const float* R, const float* T, float* zdepth, uint8_t* mask, float* min_sdf,
                        float* depth, float* normal, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx->has_decoder) return fail(ctx, DISTR_ERR_NO_DECODER, "distr_set_decoder has not been called");
  int rc = check_cfg(ctx, cfg);
  if (rc) return rc;
  if (nviews < 1 || nviews > DISTR_MAX_VIEWS) return fail(ctx, DISTR_ERR_INVALID_ARG, "nviews %d not in [1, %d]", nviews, DISTR_MAX_VIEWS);
  if (lat_stride != 0 && lat_stride < ctx->D.nlat) return fail(ctx, DISTR_ERR_INVALID_ARG, "latent_stride must be 0 (shared shape code) or >= %d", ctx->D.nlat);
  if (!latent || !R || !T || !ws) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  View V;
  const size_t single = make_view(*cfg, ws, V, ctx->save_masks, nviews);
  if (ws_bytes < single * nviews) return fail(ctx, DISTR_ERR_WORKSPACE, "forward workspace too small: %zu < %zu", ws_bytes, single * nviews);
  V.blocks = ctx->ray_blocks ? 1 : 0;
  ViewFlags vf;
  rc = make_view_flags(ctx, *cfg, nviews, view_flags, vf);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  int32_t* hint_dev = choose_tail_from(ctx, V, s);
  if ((rc = setup_levels(ctx, V, latent, lat_stride, R, T, vf, s))) return rc;
  RenderPlan p;
  p.wide = wide_decoder(ctx);
  p.b6 = cfg->arith != DISTR_ARITH_F32;
  p.h3 = cfg->arith == DISTR_ARITH_F16X3;
  p.recursive = cfg->marcher != DISTR_MARCH_TRIVIAL;
  p.t32 = ctx->hybrid_threshold; p.t16 = p.b6 ? 0 : std::min(ctx->tail16_threshold, ctx->hybrid_threshold);
  MarchTimer timer(ctx, s);
  MarchArgs A;
  memset(&A, 0, sizeof(A));
  A.V = V;
  A.planes[0] = ctx->planes[0]; A.planes[1] = ctx->planes[1];
  const bool split = p.recursive && !p.wide;         // else every ray on 64-ray tiles
  A.t16 = split ? p.t16 : 0; A.t32 = split ? p.t32 : 0; A.which = 64;
  // f(origin) of every view (sample point of padded rows) is evaluated by nviews extra workgroups of ONE march launch: for the
  // recursive marchers they ride on the 16-ray role of the last step (free: a tail step); 'trivial' puts them on its first launch
  p.xr = (split && !p.b6) ? xchg_region(ctx, s) : nullptr;
  if ((rc = march_coarse(ctx, V, A, p, timer, s))) return rc;
  if ((rc = march_fine(ctx, V, A, p, timer, s))) return rc;
  if (ctx->debug_steps >= 0) return DISTR_OK;
  return finalize_and_normals(ctx, V, p.wide, hint_dev, zdepth, mask, min_sdf, depth, normal, s);
}

int render_backward_impl(distr_ctx* ctx, const distr_render_cfg* cfg, int nviews, const void* ws, size_t ws_bytes, const float* g_zdepth,
                         const float* g_min_sdf, const float* g_depth, const float* g_normal, float* g_latent, float* g_R,
                         float* g_T, void* ws_bwd, size_t ws_bwd_bytes, void* stream) {
  if (!ctx->has_decoder) return fail(ctx, DISTR_ERR_NO_DECODER, "distr_set_decoder has not been called");
  int rc = check_cfg(ctx, cfg);
  if (rc) return rc;
  if (nviews < 1 || nviews > DISTR_MAX_VIEWS) return fail(ctx, DISTR_ERR_INVALID_ARG, "nviews %d not in [1, %d]", nviews, DISTR_MAX_VIEWS);
  if (!ws || !ws_bwd) return fail(ctx, DISTR_ERR_INVALID_ARG, "null workspace");
  if (!cfg->save_for_backward) return fail(ctx, DISTR_ERR_INVALID_ARG, "forward was run with save_for_backward=0");
  View V;
  const size_t single = make_view(*cfg, const_cast<void*>(ws), V, ctx->save_masks, nviews);
  if (ws_bytes < single * nviews) return fail(ctx, DISTR_ERR_WORKSPACE, "forward workspace too small: %zu < %zu", ws_bytes, single * nviews);
  const size_t bsingle = bwd_bytes(*cfg);
  if (ws_bwd_bytes < bsingle * nviews) return fail(ctx, DISTR_ERR_WORKSPACE, "backward workspace too small: %zu < %zu", ws_bwd_bytes, bsingle * nviews);
  hipStream_t s = (hipStream_t)stream;
  const DecoderDev& D = ctx->D;
  const int P = V.P;
  const unsigned NV = (unsigned)nviews;
  constexpr int TILE = 64;
  const BwdCarve bc = carve_bwd(*cfg, P, ws_bwd);
  const BwdWs& W = bc.W;
  const size_t smax = bc.smax;
  const unsigned tiles = (unsigned)((smax + TILE - 1) / TILE);
  const int nblk = bc.nblk;
  const unsigned nchunks = bc.nchunks;
  hipLaunchKernelGGL(k_bwd_prep<false>, dim3(nblk, NV), dim3(256), 0, s, V, g_zdepth, g_min_sdf, g_depth, g_normal, W);
  LAUNCH_CHECK("k_bwd_prep<count>");
  hipLaunchKernelGGL(k_bwd_scan, dim3(NV), dim3(256), 0, s, V, W, nblk);
  LAUNCH_CHECK("k_bwd_scan");
  hipLaunchKernelGGL(k_bwd_prep<true>, dim3(nblk, NV), dim3(256), 0, s, V, g_zdepth, g_min_sdf, g_depth, g_normal, W);
  LAUNCH_CHECK("k_bwd_prep<emit>");
  BwdArgs B;
  memset(&B, 0, sizeof(B));
  B.V = V; B.samples = W.samples; B.partial = W.partial; B.bstride = W.bstride; B.planes[0] = ctx->planes[0]; B.planes[1] = ctx->planes[1];
  // tile-size split of every view's sample list (bwd_range): full rounds on 64-sample tiles, a small remainder on 32-sample tiles
  const bool wide = wide_decoder(ctx);       // (wide decoders: the same tile split, so the same partial rows and reduction order)
  const bool bsplit = V.save_masks != 0;
  B.split = bsplit ? 1 : 0;
  if (bsplit) {     // the dX chain in the arithmetic of the forward it differentiates
    rc = launch_bwd(ctx, "k_bwd", BWD_SAVED, 2, cfg->arith, wide, NV * (unsigned)((smax + 63) / 64), s, B);
    if (!rc) rc = launch_bwd(ctx, "k_bwd", BWD_SAVED, 1, cfg->arith, wide, NV * (unsigned)((std::min<size_t>(smax, 8192) + 31) / 32), s, B);
  } else rc = launch_bwd(ctx, "k_bwd", BWD_FULL, 2, 0, wide, NV * tiles, s, B);     // DISTR_SAVE_MASKS=0: recompute the forward
  if (rc) return rc;
  hipLaunchKernelGGL(k_bwd_reduce, dim3((2 * HID + 12 + 255) / 256, nchunks, NV), dim3(256), 0, s, V, W, BWD_CHUNK, bsplit ? -1 : TILE);
  LAUNCH_CHECK("k_bwd_reduce");
  hipLaunchKernelGGL(k_bwd_final, dim3(NV), dim3(256), 0, s, V, D, W, (int)nchunks, BWD_CHUNK, bsplit ? -1 : TILE, g_latent, g_R, g_T);
  LAUNCH_CHECK("k_bwd_final");
  return DISTR_OK;
}

int render_normal_impl(distr_ctx* ctx, const distr_render_cfg* cfg, int nviews, const float* latent, int64_t lat_stride, const float* R,
                       const float* T, const float* zdepth, const uint8_t* mask, float* normal3xP, void* ws, size_t ws_bytes,
                       void* stream) {
  if (!ctx->has_decoder) return fail(ctx, DISTR_ERR_NO_DECODER, "distr_set_decoder has not been called");
  int rc = check_cfg(ctx, cfg);
  if (rc) return rc;
  if (nviews < 1 || nviews > DISTR_MAX_VIEWS) return fail(ctx, DISTR_ERR_INVALID_ARG, "nviews %d not in [1, %d]", nviews, DISTR_MAX_VIEWS);
  if (lat_stride != 0 && lat_stride < ctx->D.nlat) return fail(ctx, DISTR_ERR_INVALID_ARG, "latent_stride must be 0 (shared shape code) or >= %d", ctx->D.nlat);
  if (!latent || !R || !T || !zdepth || !mask || !normal3xP || !ws) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  View V;
  const size_t single = make_view(*cfg, ws, V, ctx->save_masks, nviews);
  if (ws_bytes < single * nviews) return fail(ctx, DISTR_ERR_WORKSPACE, "workspace too small: %zu < %zu", ws_bytes, single * nviews);
  hipStream_t s = (hipStream_t)stream;
  const DecoderDev& D = ctx->D;
  const int P = V.P;
  const unsigned NV = (unsigned)nviews;
  ViewFlags vf;
  rc = make_view_flags(ctx, *cfg, nviews, nullptr, vf);
  if (rc) return rc;
  hipLaunchKernelGGL(k_prep, dim3(4, NV), dim3(256), 0, s, V, D, latent, lat_stride, R, T, vf);
  LAUNCH_CHECK("k_prep");
  HIP_TRY(hipMemsetAsync(normal3xP, 0, (size_t)nviews * P * 3 * sizeof(float), s));
  hipLaunchKernelGGL(k_mask_list, dim3((unsigned)((P + 255) / 256), NV), dim3(256), 0, s, V, mask);
  LAUNCH_CHECK("k_mask_list");
  BwdArgs B;
  memset(&B, 0, sizeof(B));
  B.V = V; B.zdepth = zdepth; B.zstride = (int64_t)P * sizeof(float);
  if ((rc = launch_bwd(ctx, "k_bwd<pointgrad>", BWD_POINTGRAD, 2, 0, wide_decoder(ctx), NV * (unsigned)((P + 63) / 64), s, B))) return rc;
  hipLaunchKernelGGL(k_normal_finish, dim3((unsigned)((P + 255) / 256), NV), dim3(256), 0, s, V, (float*)nullptr, normal3xP, 0);
  LAUNCH_CHECK("k_normal_finish");
  return DISTR_OK;
}

}  // namespace

int distr_render_forward(distr_ctx* ctx, const distr_render_cfg* cfg, const float* latent, const float* R, const float* T,
                         float* zdepth, uint8_t* mask, float* min_sdf, float* depth, float* normal, void* ws, size_t ws_bytes,
                         void* stream) {
  return distr_render_forward_batch(ctx, cfg, 1, nullptr, latent, 0, R, T, zdepth, mask, min_sdf, depth, normal, ws, ws_bytes, stream);
}

int distr_render_forward_batch(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, const int32_t* view_flags,
                               const float* latent, int64_t latent_stride, const float* R, const float* T, float* zdepth,
                               uint8_t* mask, float* min_sdf, float* depth, float* normal, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  return render_forward_impl(ctx, cfg, nviews, view_flags, latent, latent_stride, R, T, zdepth, mask, min_sdf, depth, normal, ws,
                             ws_bytes, stream);
}

int distr_render_backward(distr_ctx* ctx, const distr_render_cfg* cfg, const void* ws, size_t ws_bytes, const float* g_zdepth,
                          const float* g_min_sdf, const float* g_depth, const float* g_normal, float* g_latent, float* g_R,
                          float* g_T, void* ws_bwd, size_t ws_bwd_bytes, void* stream) {
  return distr_render_backward_batch(ctx, cfg, 1, ws, ws_bytes, g_zdepth, g_min_sdf, g_depth, g_normal, g_latent, g_R, g_T, ws_bwd, ws_bwd_bytes, stream);
}

int distr_render_backward_batch(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, const void* ws, size_t ws_bytes,
                                const float* g_zdepth, const float* g_min_sdf, const float* g_depth, const float* g_normal,
                                float* g_latent, float* g_R, float* g_T, void* ws_bwd, size_t ws_bwd_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  return render_backward_impl(ctx, cfg, nviews, ws, ws_bytes, g_zdepth, g_min_sdf, g_depth, g_normal, g_latent, g_R, g_T, ws_bwd,
                              ws_bwd_bytes, stream);
}

// ---- the backward's gradient-sample list, written out (include/distr_render_train.h)
int64_t distr_render_max_samples(const distr_render_cfg* cfg) {
  if (check_cfg(nullptr, cfg)) return 0;
  return (int64_t)band_rows(*cfg) * cfg->W * cfg->buffer_size + 1;
}

int distr_render_samples_export_batch(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, const void* ws_fwd, size_t ws_fwd_bytes,
                                      const void* ws_bwd, size_t ws_bwd_bytes, float* xyz, float* coef, int32_t* src, int64_t cap,
                                      int32_t* counts_dev, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  int rc = check_cfg(ctx, cfg);
  if (rc) return rc;
  if (nviews < 1 || nviews > DISTR_MAX_VIEWS) return fail(ctx, DISTR_ERR_INVALID_ARG, "nviews %d not in [1, %d]", nviews, DISTR_MAX_VIEWS);
  if (!cfg->save_for_backward) return fail(ctx, DISTR_ERR_INVALID_ARG, "sample export: the forward was run with save_for_backward=0");
  if (!ws_fwd || !ws_bwd) return fail(ctx, DISTR_ERR_INVALID_ARG, "null workspace");
  if (!xyz || !coef || !counts_dev) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  View V;
  const size_t single = make_view(*cfg, const_cast<void*>(ws_fwd), V, ctx->save_masks, nviews);
  const BwdCarve bc = carve_bwd(*cfg, V.P, const_cast<void*>(ws_bwd));
  if (cap < (int64_t)bc.smax) return fail(ctx, DISTR_ERR_INVALID_ARG, "sample export: cap %lld is below the %zu rows a view's list can hold", (long long)cap, bc.smax);
  if (ws_fwd_bytes < single * nviews) return fail(ctx, DISTR_ERR_WORKSPACE, "forward workspace too small: %zu < %zu", ws_fwd_bytes, single * nviews);
  if (ws_bwd_bytes < (size_t)bc.W.bstride * nviews) return fail(ctx, DISTR_ERR_WORKSPACE, "backward workspace too small: %zu < %zu", ws_bwd_bytes, (size_t)bc.W.bstride * nviews);
  // (a list never holds more than smax <= cap rows: the grid covers those, whatever stride the caller chose)
  hipLaunchKernelGGL(k_samples_export, dim3((unsigned)((bc.smax + 255) / 256), (unsigned)nviews), dim3(256), 0, (hipStream_t)stream, V, bc.W, xyz, coef,
                     src, cap, counts_dev);
  LAUNCH_CHECK("k_samples_export");
  return DISTR_OK;
}

int distr_render_normal(distr_ctx* ctx, const distr_render_cfg* cfg, const float* latent, const float* R, const float* T,
                        const float* zdepth, const uint8_t* mask, float* normal3xP, void* ws, size_t ws_bytes, void* stream) {
  return distr_render_normal_batch(ctx, cfg, 1, latent, 0, R, T, zdepth, mask, normal3xP, ws, ws_bytes, stream);
}

int distr_render_normal_batch(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, const float* latent, int64_t latent_stride,
                              const float* R, const float* T, const float* zdepth, const uint8_t* mask, float* normal3xP, void* ws,
                              size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  return render_normal_impl(ctx, cfg, nviews, latent, latent_stride, R, T, zdepth, mask, normal3xP, ws, ws_bytes, stream);
}

size_t distr_mlp_workspace_bytes(int64_t n) { (void)n; return 2 * HID * sizeof(float) + 256; }

size_t distr_mlp_backward_workspace_bytes(int64_t n) {
  const size_t tiles = (size_t)((n + 31) / 32);
  return distr_mlp_workspace_bytes(n) + tiles * PSTRIDE * sizeof(float) + 256;
}

size_t distr_mlp_multi_workspace_bytes(int32_t nseg, const int64_t* counts_host) {
  PointList pl;
  return seg_list(nullptr, nseg, counts_host, pl) == DISTR_OK ? carve_list(nullptr, pl, false) : 0;
}

size_t distr_mlp_backward_multi_workspace_bytes(int32_t nseg, const int64_t* counts_host) {
  PointList pl;
  return seg_list(nullptr, nseg, counts_host, pl) == DISTR_OK ? carve_list(nullptr, pl, true) : 0;
}

}  // extern "C"

// ---- decode_sdf on a point list, plain or segmented: the entry points below and the lists of distr_depth_samples_*
namespace {

// the two ways to a list of the SDF decoder, each with the checks that come before the pointers'; the caller holds the EntryGuard
int sdf_plain_list(distr_ctx* ctx, int64_t n, PointList& pl) {
  if (!ctx->has_decoder) return fail(ctx, DISTR_ERR_NO_DECODER, "distr_set_decoder has not been called");
  pl = plain_list(n);
  return DISTR_OK;
}

int sdf_seg_list(distr_ctx* ctx, int32_t nseg, const int64_t* counts, int64_t latent_stride, PointList& pl) {
  if (int rc = seg_list(ctx, nseg, counts, pl)) return rc;
  if (!ctx->has_decoder) return fail(ctx, DISTR_ERR_NO_DECODER, "distr_set_decoder has not been called");
  if (latent_stride != 0 && latent_stride < ctx->D.nlat) return fail(ctx, DISTR_ERR_INVALID_ARG, "latent_stride %lld: 0 (shared code) or >= %d", (long long)latent_stride, ctx->D.nlat);
  return DISTR_OK;
}

// sdf of every point
int mlp_eval_list(distr_ctx* ctx, PointList& pl, const float* latent, int64_t latent_stride, const float* xyz, float clamp, float* sdf, void* ws,
                  size_t ws_bytes, hipStream_t s) {
  int rc = point_list_prologue(ctx, ctx->D, pl, latent, latent_stride, xyz && sdf, ws, ws_bytes, false, s);
  if (rc || pl.n == 0) return rc;
  MarchArgs A;
  memset(&A, 0, sizeof(A));
  A.xyz = xyz; A.sdf_out = sdf; A.c0c4 = pl.c0c4; A.seg = pl.tab; A.n = pl.nseg ? 0 : pl.n; A.clamp = clamp;
  MarchTimer timer(ctx, s);
  timer.begin();
  // a plain list that fits one wave of 16-ray tiles runs on those (107 us instead of a 380 us 64-ray tile: decode_sdf on a few
  // thousand points is latency-bound); same values bit for bit
  const bool wide = wide_decoder(ctx);
  if (!pl.nseg && !wide && pl.n <= std::min(ctx->tail16_threshold, ctx->hybrid_threshold))
    rc = launch_march16(ctx, "k_march<eval>", MODE_EVAL, false, (unsigned)((pl.n + 15) / 16), s, A);
  else rc = launch_march(ctx, "k_march<eval>", MODE_EVAL, 2, false, 0, wide, pl.tiles, s, A);
  timer.end();
  return rc;
}

// (sdf, d sdf / d xyz) of every point of the unclamped decoder
int mlp_grad_list(distr_ctx* ctx, PointList& pl, const float* latent, int64_t latent_stride, const float* xyz, float* sdf, float* grad, void* ws,
                  size_t ws_bytes, hipStream_t s) {
  const int rc = point_list_prologue(ctx, ctx->D, pl, latent, latent_stride, xyz && sdf && grad, ws, ws_bytes, false, s);
  if (rc || pl.n == 0) return rc;
  BwdArgs B;
  memset(&B, 0, sizeof(B));
  B.n = pl.nseg ? 0 : pl.n; B.xyz = xyz; B.c0c4 = pl.c0c4; B.seg = pl.tab; B.out_sdf = sdf; B.out_g = grad;
  return launch_bwd(ctx, "k_bwd<pointgrad>", BWD_POINTGRAD, 2, 0, wide_decoder(ctx), pl.tiles, s, B);
}

// backward of mlp_eval_list: g_xyz and / or one g_latent row per code
int mlp_backward_list(distr_ctx* ctx, PointList& pl, const float* latent, int64_t latent_stride, const float* xyz, const float* g_sdf, float clamp,
                      float* g_xyz, float* g_latent, void* ws, size_t ws_bytes, hipStream_t s) {
  int rc = point_list_prologue(ctx, ctx->D, pl, latent, latent_stride, xyz && g_sdf, ws, ws_bytes, true, s);
  if (rc) return rc;
  if (pl.n > 0) {
    BwdArgs B;
    memset(&B, 0, sizeof(B));
    B.n = pl.nseg ? 0 : pl.n; B.xyz = xyz; B.c0c4 = pl.c0c4; B.seg = pl.tab; B.coef = g_sdf; B.clamp = clamp; B.partial = pl.partial; B.out_g = g_xyz;
    if ((rc = launch_bwd(ctx, "k_bwd<pointgrad+latent>", BWD_POINTGRAD, 2, 0, wide_decoder(ctx), pl.tiles, s, B))) return rc;
  }
  return list_latent_grad(ctx, ctx->D, pl, g_latent, s);
}

}  // namespace

extern "C" {

int distr_mlp_eval(distr_ctx* ctx, const float* latent, const float* xyz, int64_t n, float clamp, float* sdf, void* ws,
                   size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  PointList pl;
  if (int rc = sdf_plain_list(ctx, n, pl)) return rc;
  return mlp_eval_list(ctx, pl, latent, 0, xyz, clamp, sdf, ws, ws_bytes, (hipStream_t)stream);
}

int distr_mlp_eval_multi(distr_ctx* ctx, int32_t nseg, const int64_t* counts_host, const float* latent, int64_t latent_stride, const float* xyz,
                         float clamp, float* sdf, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  PointList pl;
  if (int rc = sdf_seg_list(ctx, nseg, counts_host, latent_stride, pl)) return rc;
  return mlp_eval_list(ctx, pl, latent, latent_stride, xyz, clamp, sdf, ws, ws_bytes, (hipStream_t)stream);
}

// decode_sdf in one of the split arithmetics (h3: f16x3, else bf16x6)
static int mlp_eval_split(distr_ctx* ctx, bool h3, const float* latent, const float* xyz, int64_t n, float clamp, float* sdf, void* ws,
                          size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  if (!ctx->has_decoder) return fail(ctx, DISTR_ERR_NO_DECODER, "distr_set_decoder has not been called");
  if (ctx->D.nlat != LAT) return fail(ctx, DISTR_ERR_UNSUPPORTED, "%s: built for code length %d only (this decoder: %d); use f32", h3 ? "f16x3" : "bf16x6", LAT, ctx->D.nlat);
  if (h3 && !ctx->h3_ok) return fail(ctx, DISTR_ERR_UNSUPPORTED, "f16x3: %s; use bf16x6 or f32 for this decoder", ctx->h3_why.c_str());
  hipStream_t s = (hipStream_t)stream;
  PointList pl = plain_list(n);      // (exact f32: the latent columns stay a per-call constant)
  const int rc = point_list_prologue(ctx, ctx->D, pl, latent, 0, xyz && sdf, ws, ws_bytes, false, s);
  if (rc || n == 0) return rc;
  MarchTimer timer(ctx, s);
  timer.begin();
  auto* kernel = h3 ? k_eval_split<DISTR_ARITH_F16X3> : k_eval_split<DISTR_ARITH_BF16X6>;
  hipLaunchKernelGGL(kernel, dim3(pl.tiles), dim3(NTHREADS), 0, s, xyz, n, (const float*)pl.c0c4, clamp, sdf, ctx->D, ctx->planes[h3 ? 1 : 0]);
  timer.end();
  LAUNCH_CHECK(h3 ? "k_eval_split<f16x3>" : "k_eval_split<bf16x6>");
  return DISTR_OK;
}

int distr_mlp_eval_bf16x6(distr_ctx* ctx, const float* latent, const float* xyz, int64_t n, float clamp, float* sdf, void* ws,
                          size_t ws_bytes, void* stream) {
  return mlp_eval_split(ctx, false, latent, xyz, n, clamp, sdf, ws, ws_bytes, stream);
}

int distr_mlp_eval_f16x3(distr_ctx* ctx, const float* latent, const float* xyz, int64_t n, float clamp, float* sdf, void* ws,
                         size_t ws_bytes, void* stream) {
  return mlp_eval_split(ctx, true, latent, xyz, n, clamp, sdf, ws, ws_bytes, stream);
}

int distr_mlp_grad(distr_ctx* ctx, const float* latent, const float* xyz, int64_t n, float* sdf, float* grad, void* ws,
                   size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  PointList pl;
  if (int rc = sdf_plain_list(ctx, n, pl)) return rc;
  return mlp_grad_list(ctx, pl, latent, 0, xyz, sdf, grad, ws, ws_bytes, (hipStream_t)stream);
}

int distr_mlp_grad_multi(distr_ctx* ctx, int32_t nseg, const int64_t* counts_host, const float* latent, int64_t latent_stride, const float* xyz,
                         float* sdf, float* grad, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  PointList pl;
  if (int rc = sdf_seg_list(ctx, nseg, counts_host, latent_stride, pl)) return rc;
  return mlp_grad_list(ctx, pl, latent, latent_stride, xyz, sdf, grad, ws, ws_bytes, (hipStream_t)stream);
}

int distr_mlp_backward(distr_ctx* ctx, const float* latent, const float* xyz, int64_t n, const float* g_sdf, float clamp,
                       float* g_xyz, float* g_latent, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  PointList pl;
  if (int rc = sdf_plain_list(ctx, n, pl)) return rc;
  return mlp_backward_list(ctx, pl, latent, 0, xyz, g_sdf, clamp, g_xyz, g_latent, ws, ws_bytes, (hipStream_t)stream);
}

int distr_mlp_backward_multi(distr_ctx* ctx, int32_t nseg, const int64_t* counts_host, const float* latent, int64_t latent_stride,
                             const float* xyz, const float* g_sdf, float clamp, float* g_xyz, float* g_latent, void* ws, size_t ws_bytes,
                             void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  PointList pl;
  if (int rc = sdf_seg_list(ctx, nseg, counts_host, latent_stride, pl)) return rc;
  return mlp_backward_list(ctx, pl, latent, latent_stride, xyz, g_sdf, clamp, g_xyz, g_latent, ws, ws_bytes, (hipStream_t)stream);
}

int distr_debug_mlp_layer(distr_ctx* ctx, const float* latent, const float* xyz, int64_t n, int layer, float* out, void* ws,
                          size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  if (!ctx->has_decoder) return fail(ctx, DISTR_ERR_NO_DECODER, "distr_set_decoder has not been called");
  if (wide_decoder(ctx)) return fail(ctx, DISTR_ERR_UNSUPPORTED, "test aid built for the narrow tile layout (code length >= 256)");
  if (n == 0) return fail(ctx, DISTR_ERR_INVALID_ARG, "bad argument");      // (no empty list here: there is nothing to look at)
  hipStream_t s = (hipStream_t)stream;
  PointList pl = plain_list(n);
  const int rc = point_list_prologue(ctx, ctx->D, pl, latent, 0, n > 0 && xyz && out && layer >= 0 && layer <= 7, ws, ws_bytes, false, s);
  if (rc) return rc;
  if (ctx->D.Wk) hipLaunchKernelGGL((k_debug_layer<2, true>), dim3(pl.tiles), dim3(NTHREADS), 0, s, xyz, n, (const float*)pl.c0c4, layer, out, ctx->D, (long long*)nullptr);
  else hipLaunchKernelGGL((k_debug_layer<2>), dim3(pl.tiles), dim3(NTHREADS), 0, s, xyz, n, (const float*)pl.c0c4, layer, out, ctx->D, (long long*)nullptr);
  LAUNCH_CHECK("k_debug_layer");
  return DISTR_OK;
}

// the 32-point tile as k_step's 32-ray role runs it: compacted (level 2) on its own layout, else the dense loop on Smem<1>.
// layer < 0: the stamped build (out = sdf[n], ts_out[tiles][40]); else the layer's activations by feature (out = [n][512])
static int debug_tile32(distr_ctx* ctx, const float* latent, const float* xyz, int64_t n, int layer, float* out, long long* ts_out, void* ws,
                        size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  if (!ctx->has_decoder) return fail(ctx, DISTR_ERR_NO_DECODER, "distr_set_decoder has not been called");
  if (wide_decoder(ctx)) return fail(ctx, DISTR_ERR_UNSUPPORTED, "test aid built for the narrow tile layout (code length >= 256)");
  if (n == 0) return fail(ctx, DISTR_ERR_INVALID_ARG, "bad argument");      // (no empty list here: there is nothing to look at)
  hipStream_t s = (hipStream_t)stream;
  PointList pl = plain_list(n);
  const bool timing = layer < 0;
  const int rc = point_list_prologue(ctx, ctx->D, pl, latent, 0, n > 0 && xyz && out && (timing ? ts_out != nullptr : layer <= 7), ws, ws_bytes, false, s);
  if (rc) return rc;
  const unsigned tiles = (unsigned)((n + 31) / 32);
  if (step_compact_level(ctx, 0) == 2) hipLaunchKernelGGL((k_debug_layer<1, true>), dim3(tiles), dim3(NTHREADS), 0, s, xyz, n, (const float*)pl.c0c4, timing ? 8 : layer, out, ctx->D, ts_out);
  else hipLaunchKernelGGL((k_debug_layer<1>), dim3(tiles), dim3(NTHREADS), 0, s, xyz, n, (const float*)pl.c0c4, timing ? 8 : layer, out, ctx->D, ts_out);
  LAUNCH_CHECK("k_debug_layer<32>");
  return DISTR_OK;
}

int distr_debug_mlp_layer32(distr_ctx* ctx, const float* latent, const float* xyz, int64_t n, int layer, float* out, void* ws, size_t ws_bytes,
                            void* stream) {
  if (layer < 0) return ctx ? fail(ctx, DISTR_ERR_INVALID_ARG, "bad argument") : DISTR_ERR_INVALID_ARG;
  return debug_tile32(ctx, latent, xyz, n, layer, out, nullptr, ws, ws_bytes, stream);
}

int distr_debug_tile_timing32(distr_ctx* ctx, const float* latent, const float* xyz, int64_t n, float* sdf_out, long long* ts_out, void* ws,
                              size_t ws_bytes, void* stream) {
  return debug_tile32(ctx, latent, xyz, n, -1, sdf_out, ts_out, ws, ws_bytes, stream);
}

int distr_debug_tile_timing(distr_ctx* ctx, const float* latent, const float* xyz, int64_t n, float* sdf_out, long long* ts_out,
                            void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  if (!ctx->has_decoder) return fail(ctx, DISTR_ERR_NO_DECODER, "distr_set_decoder has not been called");
  if (wide_decoder(ctx)) return fail(ctx, DISTR_ERR_UNSUPPORTED, "test aid built for the narrow tile layout (code length >= 256)");
  if (n == 0) return fail(ctx, DISTR_ERR_INVALID_ARG, "bad argument");      // (no empty list here: there is nothing to look at)
  hipStream_t s = (hipStream_t)stream;
  PointList pl = plain_list(n);
  const int rc = point_list_prologue(ctx, ctx->D, pl, latent, 0, n > 0 && xyz && sdf_out && ts_out, ws, ws_bytes, false, s);
  if (rc) return rc;
  if (ctx->D.Wk) hipLaunchKernelGGL((k_debug_layer<2, true>), dim3(pl.tiles), dim3(NTHREADS), 0, s, xyz, n, (const float*)pl.c0c4, 8, sdf_out, ctx->D, ts_out);
  else hipLaunchKernelGGL((k_debug_layer<2>), dim3(pl.tiles), dim3(NTHREADS), 0, s, xyz, n, (const float*)pl.c0c4, 8, sdf_out, ctx->D, ts_out);
  LAUNCH_CHECK("k_debug_layer<timing>");
  return DISTR_OK;
}

// the counters a finished render left in its workspace (Consts), read back once the stream has drained; V = the render's layout
static int read_consts(distr_ctx* ctx, const distr_render_cfg* cfg, const void* ws, hipStream_t s, View& V, const Consts** C) {
  make_view(*cfg, const_cast<void*>(ws), V, ctx->save_masks);
  static thread_local std::vector<char> hostbuf;
  hostbuf.resize(sizeof(Consts));
  HIP_TRY(hipMemcpyAsync(hostbuf.data(), V.C, sizeof(Consts), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *C = (const Consts*)hostbuf.data();
  return DISTR_OK;
}

int distr_get_render_stats(distr_ctx* ctx, const distr_render_cfg* cfg, const void* ws, distr_render_stats* out, void* stream) {
  if (!ctx || !ws || !out) return fail(ctx, DISTR_ERR_INVALID_ARG, "null argument");
  EntryGuard guard_(ctx);
  int rc = check_cfg(ctx, cfg);
  if (rc) return rc;
  if (out->struct_size != sizeof(distr_render_stats))   // never write past what the caller allocated
    return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_render_stats.struct_size is %u, expected %zu (set it before the call)", out->struct_size, sizeof(distr_render_stats));
  View V;
  const Consts* C;
  if ((rc = read_consts(ctx, cfg, ws, (hipStream_t)stream, V, &C))) return rc;
  memset(out, 0, sizeof(*out));
  out->struct_size = (uint32_t)sizeof(*out);
  out->num_in_sphere = C->cnt_level[0];
  int64_t ev = 0, launches = 0;
  for (int l = 1; l < V.nlev; ++l) { ev += (int64_t)V.lv[l].steps * C->cnt_level[l]; launches += V.lv[l].steps; }
  if (cfg->marcher == DISTR_MARCH_TRIVIAL) ev += (int64_t)V.fine_steps * C->cnt_level[0];
  else for (int t = 0; t < V.fine_steps; ++t) ev += C->cnt_live[t] + C->cnt_sticky[t];
  launches += (C->tail_from < V.fine_steps) ? C->tail_from + 1 : V.fine_steps;     // (steps from tail_from on share one launch: k_tail)
  out->num_point_evals = ev;
  out->num_march_launches = launches;
  out->num_valid = C->cnt_valid;
  out->num_grad_samples = C->cnt_samples;
  out->cluster_fallbacks = C->xchg_err;
  out->f16_overflows = C->f16_overflow;
  out->tail_from = C->tail_from;
  out->tail_steals = C->tail_steals;
  return DISTR_OK;
}

int distr_profile_enable(distr_ctx* ctx, int enable) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  ctx->profiling = enable != 0;
  ctx->ev_used = 0;
  return DISTR_OK;
}

int distr_profile_read(distr_ctx* ctx, int64_t* launches, double* total_ms, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  double tot = 0.0;
  for (size_t i = 0; i < ctx->ev_used; ++i) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_pool[i].first, ctx->ev_pool[i].second));
    tot += ms;
  }
  if (launches) *launches = (int64_t)ctx->ev_used;
  if (total_ms) *total_ms = tot;
  ctx->ev_used = 0;
  return DISTR_OK;
}

int distr_profile_read_list(distr_ctx* ctx, float* ms_out, int64_t cap, int64_t* n, void* stream) {
  if (!ctx || !n) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  *n = (int64_t)ctx->ev_used;
  for (size_t i = 0; i < ctx->ev_used && (int64_t)i < cap && ms_out; ++i)
    HIP_TRY(hipEventElapsedTime(&ms_out[i], ctx->ev_pool[i].first, ctx->ev_pool[i].second));
  return DISTR_OK;
}

int distr_get_live_counts(distr_ctx* ctx, const distr_render_cfg* cfg, const void* ws, int32_t* out, int32_t cap, int32_t* n,
                          void* stream) {
  if (!ctx || !ws || !out || !n) return fail(ctx, DISTR_ERR_INVALID_ARG, "null argument");
  EntryGuard guard_(ctx);
  int rc = check_cfg(ctx, cfg);
  if (rc) return rc;
  View V;
  const Consts* C;
  if ((rc = read_consts(ctx, cfg, ws, (hipStream_t)stream, V, &C))) return rc;
  int k = 0;
  for (int l = V.nlev - 1; l >= 1; --l)
    for (int st = 0; st < V.lv[l].steps; ++st) { if (k < cap) out[k] = C->cnt_level[l]; ++k; }
  for (int t = 0; t < V.fine_steps; ++t) { if (k < cap) out[k] = (cfg->marcher == DISTR_MARCH_TRIVIAL) ? C->cnt_level[0] : C->cnt_live[t] + C->cnt_sticky[t]; ++k; }
  *n = k;
  return DISTR_OK;
}

// ---- the ordered live list seen from outside (include/distr_live_order.h)
int32_t distr_block_grid(int32_t w, int32_t h) { return block_grid(w, h); }

int32_t distr_block_pixel(int32_t w, int32_t h, int32_t block, int32_t thread) {
  if (block < 0 || block >= block_grid(w, h) || thread < 0 || thread >= 256) return -1;
  return block_pixel(w, h, block, thread);
}

int distr_get_kstep_stats(distr_ctx* ctx, const distr_render_cfg* cfg, const void* ws, int64_t* out, int32_t cap, int32_t* n, void* stream) {
  if (!ctx || !ws || !out || !n) return fail(ctx, DISTR_ERR_INVALID_ARG, "null argument");
  EntryGuard guard_(ctx);
  int rc = check_cfg(ctx, cfg);
  if (rc) return rc;
  View V;
  const Consts* C;
  if ((rc = read_consts(ctx, cfg, ws, (hipStream_t)stream, V, &C))) return rc;
  int k = 0;
  auto put = [&](unsigned long long word) {
    if (k < cap) {
      const int64_t tiles = (int64_t)(word >> KSTEP_BITS);
      out[3 * k] = tiles; out[3 * k + 1] = (int64_t)(word & ((1ull << KSTEP_BITS) - 1)); out[3 * k + 2] = tiles * KSTEP_DENSE;
    }
    ++k;
  };
  for (int l = V.nlev - 1; l >= 1; --l)
    for (int st = 0; st < V.lv[l].steps; ++st) put(C->kstep_coarse[l][st & 15]);
  for (int t = 0; t < V.fine_steps; ++t) put(C->kstep_fine[t]);
  *n = k;
  return DISTR_OK;
}

int distr_get_kstep32_stats(distr_ctx* ctx, const distr_render_cfg* cfg, const void* ws, int64_t* out, int32_t cap, int32_t* n, void* stream) {
  if (!ctx || !ws || !out || !n) return fail(ctx, DISTR_ERR_INVALID_ARG, "null argument");
  EntryGuard guard_(ctx);
  int rc = check_cfg(ctx, cfg);
  if (rc) return rc;
  View V;
  const Consts* C;
  if ((rc = read_consts(ctx, cfg, ws, (hipStream_t)stream, V, &C))) return rc;
  for (int t = 0; t < V.fine_steps && t < cap; ++t) {
    const unsigned long long word = C->kstep_fine32[t];
    const int64_t tiles = (int64_t)(word >> KSTEP_BITS);
    out[3 * t] = tiles; out[3 * t + 1] = (int64_t)(word & ((1ull << KSTEP_BITS) - 1)); out[3 * t + 2] = tiles * KSTEP_DENSE;
  }
  *n = V.fine_steps;
  return DISTR_OK;
}

int distr_debug_live_list(distr_ctx* ctx, const distr_render_cfg* cfg, const float* latent, const float* R, const float* T, int32_t step,
                          int32_t* read, int32_t* left, int32_t cap, int32_t* nread, int32_t* nleft, int32_t* ordered, void* ws, size_t ws_bytes,
                          void* stream) {
  if (!ctx || !read || !left || !nread || !nleft || !ordered) return fail(ctx, DISTR_ERR_INVALID_ARG, "null argument");
  EntryGuard guard_(ctx);
  int rc = check_cfg(ctx, cfg);
  if (rc) return rc;
  View V;
  (void)make_view(*cfg, ws, V, ctx->save_masks);
  if (cfg->marcher == DISTR_MARCH_TRIVIAL || step < 0 || step + 1 >= V.fine_steps)
    return fail(ctx, DISTR_ERR_INVALID_ARG, "step %d: a recursive marcher's step with a successor (full-resolution steps: %d)", step, V.fine_steps);
  ctx->debug_steps = step + 1;
  rc = render_forward_impl(ctx, cfg, 1, nullptr, latent, 0, R, T, nullptr, nullptr, nullptr, nullptr, nullptr, ws, ws_bytes, stream);
  ctx->debug_steps = -1;
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const Consts* C;
  if ((rc = read_consts(ctx, cfg, ws, s, V, &C))) return rc;
  const int32_t c0 = C->cnt_live[step], c = C->cnt_live[step + 1];
  if (c0 < 0 || c0 > V.P || c < 0 || c > V.P) return fail(ctx, DISTR_ERR_HIP, "live counts %d -> %d of step %d outside [0, %d]", c0, c, step, V.P);
  *nread = c0; *nleft = c;
  const int t32 = ctx->hybrid_threshold, t16 = (cfg->arith != DISTR_ARITH_F32) ? 0 : std::min(ctx->tail16_threshold, ctx->hybrid_threshold);
  const int64_t prev = c0, N64 = pad_to(V.P, 64);
  const bool host_on = ctx->live_order && !wide_decoder(ctx) && compact_tile(ctx, 2, cfg->arith) && N64 > ((t16 < t32) ? (int64_t)t32 + t16 : t32);
  *ordered = (host_on && step_ordered(pad_to(prev, 16), pad_to(prev, 64), t16, t32)) ? 1 : 0;
  // (the step read one of the two buffers and wrote the other: both lists are still there)
  if (std::min(c0, cap) > 0) HIP_TRY(hipMemcpyAsync(read, V.live[step & 1], (size_t)std::min(c0, cap) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (std::min(c, cap) > 0) HIP_TRY(hipMemcpyAsync(left, V.live[(step + 1) & 1], (size_t)std::min(c, cap) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DISTR_OK;
}

int distr_debug_xchg_ts(distr_ctx* ctx, void* stream, int64_t* out64) {
  if (!ctx || !out64) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  for (auto& r : ctx->xr)
    if (r.used && r.stream == (hipStream_t)stream) {
      HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
      HIP_TRY(hipMemcpy(out64, r.flags + 256 * 128, 64 * sizeof(long long), hipMemcpyDeviceToHost));
      return DISTR_OK;
    }
  return fail(ctx, DISTR_ERR_INVALID_ARG, "no exchange region for this stream");
}

// ------------------------------------------------------------------------------------------ f2 / f3: fused losses
size_t distr_loss_workspace_bytes(int32_t H, int32_t W) {
  const size_t nblk = ((size_t)H * W + 255) / 256;
  return nblk * 24 * sizeof(float) + 256;
}

static int loss_args(distr_ctx* ctx, int32_t H, int32_t W, const void* ws, size_t ws_bytes) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  if (H < 1 || W < 1 || (int64_t)H * W >= (1 << 26)) return fail(ctx, DISTR_ERR_INVALID_ARG, "bad image size %dx%d", H, W);
  if (ws_bytes < distr_loss_workspace_bytes(H, W) || !ws) return fail(ctx, DISTR_ERR_WORKSPACE, "loss workspace too small");
  return DISTR_OK;
}

int distr_single_loss_forward(distr_ctx* ctx, int32_t H, int32_t W, const float* depth, const float* normal, const uint8_t* mask,
                              const float* min_sdf, const float* gt_depth, const float* gt_normal, const uint8_t* gt_mask,
                              float threshold, float* out8, void* ws, size_t ws_bytes, void* stream) {
  int rc = loss_args(ctx, H, W, ws, ws_bytes);
  if (rc) return rc;
  EntryGuard guard_(ctx);
  if (!mask || !min_sdf || !gt_mask || !out8 || (gt_depth && !depth) || (gt_normal && !normal))
    return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  hipStream_t s = (hipStream_t)stream;
  SingleLossArgs A{H * W, depth, normal, mask, min_sdf, gt_depth, gt_normal, gt_mask, threshold};
  const int nblk = (A.P + 255) / 256;
  hipLaunchKernelGGL(k_single_loss_partial, dim3(nblk), dim3(256), 0, s, A, (float*)ws);
  LAUNCH_CHECK("k_single_loss_partial");
  hipLaunchKernelGGL(k_single_loss_final, dim3(1), dim3(64), 0, s, (const float*)ws, nblk, out8);
  LAUNCH_CHECK("k_single_loss_final");
  return DISTR_OK;
}

int distr_single_loss_backward(distr_ctx* ctx, int32_t H, int32_t W, const float* depth, const float* normal, const uint8_t* mask,
                               const float* min_sdf, const float* gt_depth, const float* gt_normal, const uint8_t* gt_mask,
                               float threshold, const float* out8, const float* g4, float* g_depth, float* g_normal,
                               float* g_min_sdf, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  if (H < 1 || W < 1 || (int64_t)H * W >= (1 << 26)) return fail(ctx, DISTR_ERR_INVALID_ARG, "bad image size %dx%d", H, W);
  if (!mask || !min_sdf || !gt_mask || !out8 || !g4 || (gt_depth && !depth) || (gt_normal && !normal))
    return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  hipStream_t s = (hipStream_t)stream;
  SingleLossArgs A{H * W, depth, normal, mask, min_sdf, gt_depth, gt_normal, gt_mask, threshold};
  hipLaunchKernelGGL(k_single_loss_bwd, grid1(A.P), dim3(256), 0, s, A, out8, g4, g_depth, g_normal, g_min_sdf);
  LAUNCH_CHECK("k_single_loss_bwd");
  return DISTR_OK;
}

static WarpArgs warp_args(const distr_warp_cfg* c, const float* z1, const uint8_t* m1, const float* z2, const float* img1,
                          const float* img2, const float* R1, const float* T1, const float* R2, const float* T2) {
  WarpArgs A;
  A.H = c->H; A.W = c->W;
  memcpy(A.K, c->K, sizeof(A.K));
  memcpy(A.K_inv, c->K_inv, sizeof(A.K_inv));
  A.thres_depth = c->thres_depth;
  A.z1 = z1; A.m1 = m1; A.z2 = z2; A.img1 = img1; A.img2 = img2;
  A.R1 = R1; A.T1 = T1; A.R2 = R2; A.T2 = T2;
  return A;
}

int distr_warp_loss_forward(distr_ctx* ctx, const distr_warp_cfg* cfg, const float* zdepth1, const uint8_t* mask1,
                            const float* zdepth2, const float* img1, const float* img2, const float* R1, const float* T1,
                            const float* R2, const float* T2, float* out3, uint8_t* keep, float* color1, float* color2,
                            void* ws, size_t ws_bytes, void* stream) {
  if (!ctx || !cfg) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  if (cfg->struct_size != sizeof(distr_warp_cfg)) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_warp_cfg.struct_size is %u, expected %zu", cfg->struct_size, sizeof(distr_warp_cfg));
  int rc = loss_args(ctx, cfg->H, cfg->W, ws, ws_bytes);
  if (rc) return rc;
  if (!zdepth1 || !mask1 || !zdepth2 || !img1 || !img2 || !R1 || !T1 || !R2 || !T2 || !out3)
    return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  hipStream_t s = (hipStream_t)stream;
  const WarpArgs A = warp_args(cfg, zdepth1, mask1, zdepth2, img1, img2, R1, T1, R2, T2);
  const int nblk = (A.H * A.W + 255) / 256;
  hipLaunchKernelGGL(k_warp_fwd, dim3(nblk), dim3(256), 0, s, A, keep, color1, color2, (float*)ws);
  LAUNCH_CHECK("k_warp_fwd");
  hipLaunchKernelGGL(k_warp_final, dim3(1), dim3(64), 0, s, (const float*)ws, nblk, out3);
  LAUNCH_CHECK("k_warp_final");
  return DISTR_OK;
}

int distr_warp_loss_backward(distr_ctx* ctx, const distr_warp_cfg* cfg, const float* zdepth1, const uint8_t* mask1,
                             const float* zdepth2, const float* img1, const float* img2, const float* R1, const float* T1,
                             const float* R2, const float* T2, const float* out3, const float* g_loss, float* g_zdepth1,
                             float* g_cam, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx || !cfg) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  if (cfg->struct_size != sizeof(distr_warp_cfg)) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_warp_cfg.struct_size is %u, expected %zu", cfg->struct_size, sizeof(distr_warp_cfg));
  int rc = loss_args(ctx, cfg->H, cfg->W, ws, ws_bytes);
  if (rc) return rc;
  if (!zdepth1 || !mask1 || !zdepth2 || !img1 || !img2 || !R1 || !T1 || !R2 || !T2 || !out3 || !g_loss || !g_cam)
    return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  hipStream_t s = (hipStream_t)stream;
  const WarpArgs A = warp_args(cfg, zdepth1, mask1, zdepth2, img1, img2, R1, T1, R2, T2);
  const int nblk = (A.H * A.W + 255) / 256;
  hipLaunchKernelGGL(k_warp_bwd, dim3(nblk), dim3(256), 0, s, A, out3, g_loss, g_zdepth1, (float*)ws);
  LAUNCH_CHECK("k_warp_bwd");
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(64), 0, s, (const float*)ws, nblk, 24, g_cam);
  LAUNCH_CHECK("k_sum_partials");
  return DISTR_OK;
}

}  // extern "C"

// ---- shape evaluation (include/distr_mesh.h, kernels: distr_mesh.hpp)
namespace {

bool mc_grid_ok(int32_t nx, int32_t ny, int32_t nz) {
  return nx >= 2 && ny >= 2 && nz >= 2 && (int64_t)nx * ny * nz < ((int64_t)1 << 31);
}

struct McWs {
  uint16_t* info;
  int *vbase, *act, *afb;
  mesh::C3 *btot, *boff, *totals;
  size_t bytes;
};

McWs mc_ws(void* base, int64_t P) {
  const int64_t nb = (P + mesh::MTILE - 1) / mesh::MTILE;
  WsCarve c(base);
  McWs w;
  w.info = c.take<uint16_t>(P);
  w.vbase = c.take<int>(P);
  w.act = c.take<int>(P);
  w.afb = c.take<int>(P);
  w.btot = c.take<mesh::C3>(nb);
  w.boff = c.take<mesh::C3>(nb);
  w.totals = c.take<mesh::C3>(1);
  w.bytes = c.bytes();
  return w;
}

int mc_args(distr_ctx* ctx, const float* grid, int32_t nx, int32_t ny, int32_t nz, const void* ws, size_t ws_bytes) {
  if (!mc_grid_ok(nx, ny, nz))
    return fail(ctx, DISTR_ERR_INVALID_ARG, "grid %d x %d x %d: marching cubes needs at least 2 values per axis and fewer than 2^31 values", nx, ny, nz);
  if (!grid || !ws) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  if (ws_bytes < distr_mc_workspace_bytes(nx, ny, nz))
    return fail(ctx, DISTR_ERR_WORKSPACE, "marching-cubes workspace too small: %zu < %zu", ws_bytes, distr_mc_workspace_bytes(nx, ny, nz));
  return DISTR_OK;
}

}  // namespace

extern "C" {

size_t distr_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
  return mc_grid_ok(nx, ny, nz) ? mc_ws(nullptr, (int64_t)nx * ny * nz).bytes : 0;
}

int distr_mc_count(distr_ctx* ctx, const float* grid, int32_t nx, int32_t ny, int32_t nz, float level, int64_t* nverts, int64_t* nfaces,
                   void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  if (int rc = mc_args(ctx, grid, nx, ny, nz, ws, ws_bytes)) return rc;
  if (!nverts || !nfaces) return fail(ctx, DISTR_ERR_INVALID_ARG, "null count pointer");
  hipStream_t s = (hipStream_t)stream;
  const mesh::McGrid g{grid, nx, ny, nz, level, (long long)nx * ny * nz};
  const McWs w = mc_ws(ws, g.P);
  const long long nb = (g.P + mesh::MTILE - 1) / mesh::MTILE;
  hipLaunchKernelGGL(mesh::k_mc_classify, dim3((unsigned)nb), dim3(mesh::MB), 0, s, g, w.info, w.btot);
  LAUNCH_CHECK("k_mc_classify");
  hipLaunchKernelGGL(mesh::k_mesh_top_scan<mesh::C3>, dim3(1), dim3(mesh::MB), 0, s, (const mesh::C3*)w.btot, nb, w.boff, w.totals);
  LAUNCH_CHECK("k_mesh_top_scan");
  mesh::C3 tot;
  HIP_TRY(hipMemcpyAsync(&tot, w.totals, sizeof(tot), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (tot.v > INT32_MAX || tot.f > INT32_MAX)
    return fail(ctx, DISTR_ERR_UNSUPPORTED, "mesh of %lld vertices / %lld triangles: int32 indices cannot hold it", tot.v, tot.f);
  *nverts = tot.v;
  *nfaces = tot.f;
  return DISTR_OK;
}

int distr_mc_emit(distr_ctx* ctx, const float* grid, int32_t nx, int32_t ny, int32_t nz, float level, const float* origin,
                  const float* voxel_size, float* verts, int64_t nverts, int32_t* faces, int64_t nfaces, void* ws, size_t ws_bytes,
                  void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  if (int rc = mc_args(ctx, grid, nx, ny, nz, ws, ws_bytes)) return rc;
  if (!origin || !voxel_size) return fail(ctx, DISTR_ERR_INVALID_ARG, "origin / voxel_size (host arrays of 3) are null");
  if (nverts < 0 || nfaces < 0 || nverts > INT32_MAX || nfaces > INT32_MAX || (nverts > 0 && !verts) || (nfaces > 0 && !faces))
    return fail(ctx, DISTR_ERR_INVALID_ARG, "bad vertex / triangle buffers (%lld, %lld)", (long long)nverts, (long long)nfaces);
  hipStream_t s = (hipStream_t)stream;
  const mesh::McGrid g{grid, nx, ny, nz, level, (long long)nx * ny * nz};
  const McWs w = mc_ws(ws, g.P);
  const long long nb = (g.P + mesh::MTILE - 1) / mesh::MTILE;
  const mesh::McOut o{origin[0], origin[1], origin[2], voxel_size[0], voxel_size[1], voxel_size[2], verts, nverts, faces, nfaces};
  hipLaunchKernelGGL(mesh::k_mc_compact, dim3((unsigned)nb), dim3(mesh::MB), 0, s, g, (const uint16_t*)w.info, (const mesh::C3*)w.boff,
                     w.act, w.afb, w.vbase, o);
  LAUNCH_CHECK("k_mc_compact");
  const long long fblocks = std::min<long long>((g.P + mesh::MB - 1) / mesh::MB, 4096);
  hipLaunchKernelGGL(mesh::k_mc_faces, dim3((unsigned)fblocks), dim3(mesh::MB), 0, s, g, (const uint16_t*)w.info, (const int*)w.act,
                     (const int*)w.afb, (const int*)w.vbase, (const mesh::C3*)w.totals, o);
  LAUNCH_CHECK("k_mc_faces");
  return DISTR_OK;
}

size_t distr_sample_workspace_bytes(int64_t nfaces) {
  if (nfaces < 1) return 0;
  const int64_t nb = (nfaces + mesh::MTILE - 1) / mesh::MTILE;
  WsCarve c(nullptr);
  c.take<double>(nfaces);
  c.take<double>(nb);
  c.take<double>(nb);
  c.take<double>(1);
  return c.bytes();
}

int distr_sample_surface(distr_ctx* ctx, const float* verts, int64_t nverts, const int32_t* faces, int64_t nfaces, int64_t n, uint64_t seed,
                         float* points, int32_t* face_index, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  if (nverts < 1 || nfaces < 1 || nfaces > INT32_MAX || n < 0) return fail(ctx, DISTR_ERR_INVALID_ARG, "sampling needs a mesh with vertices and triangles (%lld, %lld) and n >= 0", (long long)nverts, (long long)nfaces);
  if (!verts || !faces || !ws || (n > 0 && (!points || !face_index))) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  if (ws_bytes < distr_sample_workspace_bytes(nfaces)) return fail(ctx, DISTR_ERR_WORKSPACE, "sampling workspace too small");
  if (n == 0) return DISTR_OK;
  hipStream_t s = (hipStream_t)stream;
  const long long nb = (nfaces + mesh::MTILE - 1) / mesh::MTILE;
  WsCarve c(ws);
  double* cdf = c.take<double>(nfaces);
  double* btot = c.take<double>(nb);
  double* boff = c.take<double>(nb);
  double* total = c.take<double>(1);
  const mesh::SurfMesh m{verts, nverts, faces, nfaces};
  hipLaunchKernelGGL(mesh::k_area_scan<false>, dim3((unsigned)nb), dim3(mesh::MB), 0, s, m, btot, (const double*)nullptr, (double*)nullptr);
  LAUNCH_CHECK("k_area_scan<false>");
  hipLaunchKernelGGL(mesh::k_mesh_top_scan<double>, dim3(1), dim3(mesh::MB), 0, s, (const double*)btot, nb, boff, total);
  LAUNCH_CHECK("k_mesh_top_scan");
  hipLaunchKernelGGL(mesh::k_area_scan<true>, dim3((unsigned)nb), dim3(mesh::MB), 0, s, m, (double*)nullptr, (const double*)boff, cdf);
  LAUNCH_CHECK("k_area_scan<true>");
  hipLaunchKernelGGL(mesh::k_sample, dim3((unsigned)((n + mesh::MB - 1) / mesh::MB)), dim3(mesh::MB), 0, s, m, (const double*)cdf, n, seed,
                     points, face_index);
  LAUNCH_CHECK("k_sample");
  return DISTR_OK;
}

size_t distr_nearest_workspace_bytes(int64_t na) {
  const int64_t nb = std::max<int64_t>(1, (na + mesh::MTILE - 1) / mesh::MTILE);
  WsCarve c(nullptr);
  c.take<mesh::D2>(nb);
  c.take<mesh::D2>(nb);
  return c.bytes();
}

int distr_nearest_sqdist(distr_ctx* ctx, const float* a, int64_t na, const float* b, int64_t nb, float* d2, double* sums, void* ws,
                         size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  if (na < 0 || nb < 1 || na > INT32_MAX || nb > INT32_MAX) return fail(ctx, DISTR_ERR_INVALID_ARG, "point counts %lld, %lld (need na >= 0, nb >= 1)", (long long)na, (long long)nb);
  if (!b || !ws || (na > 0 && (!a || !d2))) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  if (ws_bytes < distr_nearest_workspace_bytes(na)) return fail(ctx, DISTR_ERR_WORKSPACE, "nearest-distance workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const long long ablocks = (na + mesh::MB - 1) / mesh::MB;
  if (na > 0) {
    hipLaunchKernelGGL(mesh::k_fill_inf, dim3((unsigned)ablocks), dim3(mesh::MB), 0, s, (unsigned*)d2, (long long)na);
    LAUNCH_CHECK("k_fill_inf");
    // B is split into chunks (grid.y) until about 2048 workgroups are in flight: 30 000 points of A alone fill only 118
    const long long tiles = (nb + mesh::NN_TILE - 1) / mesh::NN_TILE;
    const long long split = std::max<long long>(1, std::min<long long>({tiles, (2048 + ablocks - 1) / ablocks, 1024}));
    const long long chunk = (tiles + split - 1) / split * mesh::NN_TILE;
    const long long ysz = (nb + chunk - 1) / chunk;
    hipLaunchKernelGGL(mesh::k_nearest, dim3((unsigned)ablocks, (unsigned)ysz), dim3(mesh::MB), 0, s, a, (long long)na, b, (long long)nb,
                       chunk, (unsigned*)d2);
    LAUNCH_CHECK("k_nearest");
  }
  if (sums) {
    const long long nblk = std::max<long long>(1, (na + mesh::MTILE - 1) / mesh::MTILE);
    WsCarve c(ws);
    mesh::D2* btot = c.take<mesh::D2>(nblk);
    mesh::D2* boff = c.take<mesh::D2>(nblk);
    hipLaunchKernelGGL(mesh::k_dist_sums, dim3((unsigned)nblk), dim3(mesh::MB), 0, s, (const float*)d2, (long long)na, btot);
    LAUNCH_CHECK("k_dist_sums");
    hipLaunchKernelGGL(mesh::k_mesh_top_scan<mesh::D2>, dim3(1), dim3(mesh::MB), 0, s, (const mesh::D2*)btot, nblk, boff, (mesh::D2*)sums);
    LAUNCH_CHECK("k_mesh_top_scan");
  }
  return DISTR_OK;
}

size_t distr_mesh_sdf_workspace_bytes(int64_t nq, int64_t nfaces) {
  if (nq < 1 || nfaces < 1) return 0;
  const int64_t nchunks = (nfaces + mesh::SDF_CHUNK - 1) / mesh::SDF_CHUNK;
  WsCarve c(nullptr);
  c.take<unsigned long long>(nq);
  c.take<double>(nchunks * nq);
  return c.bytes();
}

int distr_mesh_sdf(distr_ctx* ctx, const float* verts, int64_t nverts, const int32_t* faces, int64_t nfaces, const float* q, int64_t nq,
                   float* sdf, float* d2, float* winding, int32_t* face, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  const int64_t nchunks = (nfaces + mesh::SDF_CHUNK - 1) / mesh::SDF_CHUNK;
  if (nverts < 1 || nfaces < 1 || nfaces > INT32_MAX || nchunks > 65535 || nq < 0 || nq > INT32_MAX)
    return fail(ctx, DISTR_ERR_INVALID_ARG, "signed distance needs a mesh with vertices and 1 .. %d triangles (%lld, %lld) and 0 <= nq < 2^31 (%lld)",
                65535 * mesh::SDF_CHUNK, (long long)nverts, (long long)nfaces, (long long)nq);
  if (!verts || !faces || (nq > 0 && (!q || !sdf || !ws))) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  if (ws_bytes < distr_mesh_sdf_workspace_bytes(nq, nfaces)) return fail(ctx, DISTR_ERR_WORKSPACE, "signed-distance workspace too small");
  if (nq == 0) return DISTR_OK;
  hipStream_t s = (hipStream_t)stream;
  WsCarve c(ws);
  unsigned long long* best = c.take<unsigned long long>(nq);
  double* wsum = c.take<double>(nchunks * nq);
  const unsigned qblocks = (unsigned)((nq + mesh::MB - 1) / mesh::MB);
  const mesh::SurfMesh m{verts, nverts, faces, nfaces};
  hipLaunchKernelGGL(mesh::k_sdf_init, dim3(qblocks), dim3(mesh::MB), 0, s, best, (long long)nq);
  LAUNCH_CHECK("k_sdf_init");
  hipLaunchKernelGGL(mesh::k_sdf_pairs, dim3(qblocks, (unsigned)nchunks), dim3(mesh::MB), 0, s, m, q, (long long)nq, best, wsum);
  LAUNCH_CHECK("k_sdf_pairs");
  hipLaunchKernelGGL(mesh::k_sdf_finish, dim3(qblocks), dim3(mesh::MB), 0, s, q, (long long)nq, (const unsigned long long*)best,
                     (const double*)wsum, (long long)nchunks, sdf, d2, winding, face);
  LAUNCH_CHECK("k_sdf_finish");
  return DISTR_OK;
}

int distr_sdf_queries(distr_ctx* ctx, const float* surf, int64_t ns, float sigma_a, float sigma_b, int64_t n_uniform, float half_extent,
                      uint64_t seed, float* q_out, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  if (ns < 0 || n_uniform < 0 || ns > INT32_MAX || n_uniform > INT32_MAX)
    return fail(ctx, DISTR_ERR_INVALID_ARG, "query counts %lld, %lld (need 0 <= count < 2^31)", (long long)ns, (long long)n_uniform);
  const int64_t n = std::max(ns, n_uniform);
  if ((ns > 0 && !surf) || (n > 0 && !q_out)) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  if (n == 0) return DISTR_OK;
  hipLaunchKernelGGL(mesh::k_sdf_queries, dim3((unsigned)((n + mesh::MB - 1) / mesh::MB)), dim3(mesh::MB), 0, (hipStream_t)stream, surf,
                     (long long)ns, sigma_a, sigma_b, (long long)n_uniform, half_extent, seed, q_out);
  LAUNCH_CHECK("k_sdf_queries");
  return DISTR_OK;
}

size_t distr_mesh_render_workspace_bytes(int32_t H, int32_t W, int32_t nviews) {
  if (H < 1 || W < 1 || nviews < 1 || nviews > DISTR_MAX_VIEWS || (int64_t)H * W * nviews > INT32_MAX) return 0;
  WsCarve c(nullptr);
  c.take<unsigned long long>((size_t)H * W * nviews);
  return c.bytes();
}

int distr_mesh_render(distr_ctx* ctx, const distr_mesh_render_cfg* cfg, const float* verts, int64_t nverts, const int32_t* faces,
                      int64_t nfaces, int32_t nviews, const float* RT, float* depth, float* zdepth, float* normal, uint8_t* mask,
                      int32_t* face, float* bary, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  if (!cfg) return fail(ctx, DISTR_ERR_INVALID_ARG, "null mesh render cfg");
  if (cfg->struct_size != sizeof(distr_mesh_render_cfg))
    return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_mesh_render_cfg.struct_size %u: this library expects %zu (set it with DISTR_INIT)", cfg->struct_size, sizeof(distr_mesh_render_cfg));
  if (nviews < 1 || nviews > DISTR_MAX_VIEWS) return fail(ctx, DISTR_ERR_INVALID_ARG, "nviews %d not in [1, %d]", nviews, DISTR_MAX_VIEWS);
  if (cfg->H < 1 || cfg->W < 1 || (int64_t)cfg->H * cfg->W * nviews > INT32_MAX)
    return fail(ctx, DISTR_ERR_INVALID_ARG, "image size %d x %d, %d views: need H * W * nviews < 2^31", cfg->H, cfg->W, nviews);
  if (cfg->normal_frame != DISTR_MESH_NORMAL_WORLD && cfg->normal_frame != DISTR_MESH_NORMAL_IMAGE)
    return fail(ctx, DISTR_ERR_INVALID_ARG, "normal_frame %d", cfg->normal_frame);
  const int64_t nchunks = (nfaces + mesh::RC_CHUNK - 1) / mesh::RC_CHUNK;
  if (nverts < 1 || nfaces < 1 || nfaces > INT32_MAX || nchunks > 65535)
    return fail(ctx, DISTR_ERR_INVALID_ARG, "mesh render needs a mesh with vertices and 1 .. %d triangles (%lld, %lld)", 65535 * mesh::RC_CHUNK,
                (long long)nverts, (long long)nfaces);
  if (!verts || !faces || !RT || !ws) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  if (ws_bytes < distr_mesh_render_workspace_bytes(cfg->H, cfg->W, nviews)) return fail(ctx, DISTR_ERR_WORKSPACE, "mesh render workspace too small");
  hipStream_t s = (hipStream_t)stream;
  mesh::CastGeo G;
  G.H = cfg->H; G.W = cfg->W; G.P = cfg->H * cfg->W;
  for (int i = 0; i < 9; ++i) { G.Ki[i] = cfg->K_inv[i]; G.M[i] = cfg->M[i]; }
  G.frame = cfg->normal_frame;
  WsCarve c(ws);
  const long long n = (long long)G.P * nviews;
  unsigned long long* best = c.take<unsigned long long>(n);
  const mesh::SurfMesh m{verts, nverts, faces, nfaces};
  const int per = mesh::MB * mesh::RC_PPT;
  hipLaunchKernelGGL(mesh::k_sdf_init, dim3((unsigned)((n + mesh::MB - 1) / mesh::MB)), dim3(mesh::MB), 0, s, best, n);
  LAUNCH_CHECK("k_sdf_init");
  hipLaunchKernelGGL(mesh::k_mesh_cast, dim3((unsigned)((G.P + per - 1) / per), (unsigned)nchunks, (unsigned)nviews), dim3(mesh::MB), 0, s, m, G,
                     RT, best);
  LAUNCH_CHECK("k_mesh_cast");
  const mesh::CastOut o{depth, zdepth, normal, mask, face, bary};
  hipLaunchKernelGGL(mesh::k_mesh_finish, dim3((unsigned)((G.P + mesh::MB - 1) / mesh::MB), (unsigned)nviews), dim3(mesh::MB), 0, s, m, G, RT,
                     (const unsigned long long*)best, o);
  LAUNCH_CHECK("k_mesh_finish");
  return DISTR_OK;
}

}  // extern "C"

// ---- depth maps back-projected into SDF samples (include/distr_samples.h, kernels: distr_samples.hpp)
namespace {

struct SampPlan {
  samples::Geo G;
  samples::Views VW;
  int nviews;
  int64_t ntot, nmax;        // valid pixels of all views, of the largest view
  int nblk_px;               // blocks of MTILE pixels per view (count / compact)
  int nblk_cam;              // blocks of MTILE valid pixels of the largest view (camera gradient)
  int64_t seg[DISTR_MAX_VIEWS];   // entries of the point list per view (m per valid pixel): the segments of the decoder calls
};

int samp_cfg(distr_ctx* ctx, const distr_samples_cfg* c, int32_t nviews, SampPlan& p) {
  if (!c) return fail(ctx, DISTR_ERR_INVALID_ARG, "null samples cfg");
  if (c->struct_size != sizeof(distr_samples_cfg))
    return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_samples_cfg.struct_size %u: this library expects %zu (set it with DISTR_INIT)", c->struct_size, sizeof(distr_samples_cfg));
  if (c->H < 1 || c->W < 1 || (int64_t)c->H * c->W > ((int64_t)1 << 26)) return fail(ctx, DISTR_ERR_INVALID_ARG, "image size %d x %d", c->H, c->W);
  if (nviews < 1 || nviews > DISTR_MAX_VIEWS) return fail(ctx, DISTR_ERR_INVALID_ARG, "nviews %d: 1..%d", nviews, DISTR_MAX_VIEWS);
  if (c->mode != DISTR_SAMPLES_SURFACE && c->mode != DISTR_SAMPLES_FREESPACE) return fail(ctx, DISTR_ERR_INVALID_ARG, "samples mode %d", c->mode);
  if (c->mode == DISTR_SAMPLES_FREESPACE && (c->number < 1 || c->number > DISTR_SAMPLES_MAX_NUMBER))
    return fail(ctx, DISTR_ERR_INVALID_ARG, "free-space samples: number %d (1..%d)", c->number, DISTR_SAMPLES_MAX_NUMBER);
  memset(&p, 0, sizeof(p));
  p.G.H = c->H; p.G.W = c->W; p.G.P = c->H * c->W;
  memcpy(p.G.Ki, c->K_inv, sizeof(p.G.Ki));
  memcpy(p.G.M, c->M, sizeof(p.G.M));
  p.G.mode = c->mode;
  p.G.m = c->mode == DISTR_SAMPLES_SURFACE ? 2 : c->number;
  p.nviews = nviews;
  p.nblk_px = (p.G.P + samples::MTILE - 1) / samples::MTILE;
  return DISTR_OK;
}

int samp_counts(distr_ctx* ctx, const int64_t* counts, SampPlan& p) {
  if (!counts) return fail(ctx, DISTR_ERR_INVALID_ARG, "null counts (host array of nviews, from distr_depth_samples_count)");
  for (int v = 0; v < p.nviews; ++v) {
    if (counts[v] < 0 || counts[v] > p.G.P) return fail(ctx, DISTR_ERR_INVALID_ARG, "counts[%d] = %lld: outside 0..H*W", v, (long long)counts[v]);
    p.VW.n[v] = (int32_t)counts[v];
    p.VW.off[v] = (int32_t)p.ntot;
    p.ntot += counts[v];
    p.nmax = std::max(p.nmax, (int64_t)counts[v]);
    p.seg[v] = counts[v] * p.G.m;
  }
  if (p.ntot * p.G.m > ((int64_t)1 << 29)) return fail(ctx, DISTR_ERR_UNSUPPORTED, "point list of %lld entries: too long", (long long)(p.ntot * p.G.m));
  p.nblk_cam = (int)std::max<int64_t>(1, (p.nmax + samples::MTILE - 1) / samples::MTILE);
  return DISTR_OK;
}

struct SampCountWs { int *btot, *boff, *totals; size_t bytes; };
SampCountWs samp_count_ws(void* base, const SampPlan& p) {
  WsCarve c(base);
  SampCountWs w;
  w.btot = c.take<int>((size_t)p.nviews * p.nblk_px);
  w.boff = c.take<int>((size_t)p.nviews * p.nblk_px);
  w.totals = c.take<int>(DISTR_MAX_VIEWS);
  w.bytes = c.bytes();
  return w;
}

// forward: one plain evaluation (shared code) or one segmented one (a code per view); sized for either
size_t samp_fwd_bytes(const SampPlan& p) { return std::max(distr_mlp_workspace_bytes(p.ntot * p.G.m), distr_mlp_multi_workspace_bytes(p.nviews, p.seg)); }

struct SampBwdWs { float *g_xyz, *part; void* mlp; size_t mlp_bytes, bytes; };
SampBwdWs samp_bwd_ws(void* base, const SampPlan& p) {
  WsCarve c(base);
  SampBwdWs w;
  w.g_xyz = c.take<float>((size_t)(3 * p.ntot * p.G.m));
  w.part = c.take<float>((size_t)p.nviews * p.nblk_cam * 12);
  w.mlp_bytes = distr_mlp_backward_multi_workspace_bytes(p.nviews, p.seg);      // one segmented backward: a segment per view
  w.mlp = c.take<char>(w.mlp_bytes);
  w.bytes = c.bytes();
  return w;
}

}  // namespace

extern "C" {

int distr_depth_samples_workspace_bytes(distr_ctx* ctx, const distr_samples_cfg* cfg, int32_t nviews, const int64_t* counts,
                                        size_t* count_bytes, size_t* forward_bytes, size_t* backward_bytes) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  SampPlan p;
  if (int rc = samp_cfg(ctx, cfg, nviews, p)) return rc;
  if (count_bytes) *count_bytes = samp_count_ws(nullptr, p).bytes;
  if (!counts) {
    if (forward_bytes || backward_bytes) return fail(ctx, DISTR_ERR_INVALID_ARG, "forward / backward workspace sizes need the counts");
    return DISTR_OK;
  }
  if (int rc = samp_counts(ctx, counts, p)) return rc;
  if (forward_bytes) *forward_bytes = samp_fwd_bytes(p);
  if (backward_bytes) *backward_bytes = samp_bwd_ws(nullptr, p).bytes;
  return DISTR_OK;
}

int distr_depth_samples_count(distr_ctx* ctx, const distr_samples_cfg* cfg, int32_t nviews, const float* depth, int32_t* index,
                              int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  SampPlan p;
  if (int rc = samp_cfg(ctx, cfg, nviews, p)) return rc;
  if (!depth || !index || !counts || !ws) return fail(ctx, DISTR_ERR_INVALID_ARG, "null pointer");
  if (ws_bytes < samp_count_ws(nullptr, p).bytes) return fail(ctx, DISTR_ERR_WORKSPACE, "depth-samples count workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const SampCountWs w = samp_count_ws(ws, p);
  const dim3 grid((unsigned)p.nblk_px, (unsigned)nviews);
  hipLaunchKernelGGL(samples::k_samp_count, grid, dim3(samples::MB), 0, s, depth, p.G.P, p.nblk_px, w.btot);
  LAUNCH_CHECK("k_samp_count");
  hipLaunchKernelGGL(samples::k_samp_top_scan, dim3((unsigned)nviews), dim3(samples::MB), 0, s, (const int*)w.btot, p.nblk_px, w.boff, w.totals);
  LAUNCH_CHECK("k_samp_top_scan");
  hipLaunchKernelGGL(samples::k_samp_compact, grid, dim3(samples::MB), 0, s, depth, p.G.P, p.nblk_px, (const int*)w.boff, index);
  LAUNCH_CHECK("k_samp_compact");
  int tot[DISTR_MAX_VIEWS];
  HIP_TRY(hipMemcpyAsync(tot, w.totals, sizeof(int) * nviews, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int v = 0; v < nviews; ++v) counts[v] = tot[v];
  return DISTR_OK;
}

int distr_depth_samples_forward(distr_ctx* ctx, const distr_samples_cfg* cfg, int32_t nviews, const int64_t* counts, const int32_t* index,
                                const float* latent, int64_t latent_stride, const float* RT, const float* depth, const float* normal,
                                const float* draws, float* xyz, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  SampPlan p;
  if (int rc = samp_cfg(ctx, cfg, nviews, p)) return rc;
  if (int rc = samp_counts(ctx, counts, p)) return rc;
  if (!ctx->has_decoder) return fail(ctx, DISTR_ERR_NO_DECODER, "distr_set_decoder has not been called");
  if (latent_stride != 0 && latent_stride < ctx->D.nlat) return fail(ctx, DISTR_ERR_INVALID_ARG, "latent_stride %lld: 0 (shared code) or >= %d", (long long)latent_stride, ctx->D.nlat);
  if (!index || !latent || !RT || !depth || !draws || !ws || (p.G.mode == DISTR_SAMPLES_SURFACE && !normal) || (p.ntot > 0 && (!xyz || !out)))
    return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  const int64_t L = p.ntot * p.G.m;
  if (ws_bytes < samp_fwd_bytes(p)) return fail(ctx, DISTR_ERR_WORKSPACE, "depth-samples forward workspace too small");
  if (L == 0) return DISTR_OK;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((p.nmax + samples::MB - 1) / samples::MB), (unsigned)nviews);
  hipLaunchKernelGGL(samples::k_samp_points, grid, dim3(samples::MB), 0, s, p.G, p.VW, index, RT, depth, normal, draws, xyz);
  LAUNCH_CHECK("k_samp_points");
  PointList pl = plain_list(L);
  if (latent_stride != 0 && nviews > 1) {           // a code per view: one segmented evaluation, a segment (with tiles of its own) per view
    if (int rc = seg_list(ctx, nviews, p.seg, pl)) return rc;
  }
  if (int rc = mlp_eval_list(ctx, pl, latent, pl.nseg ? latent_stride : 0, xyz, cfg->clamp_dist, out, ws, ws_bytes, s)) return rc;
  if (p.G.mode == DISTR_SAMPLES_SURFACE) {
    hipLaunchKernelGGL(samples::k_samp_epilogue, grid, dim3(samples::MB), 0, s, p.VW, draws, out);
    LAUNCH_CHECK("k_samp_epilogue");
  }
  return DISTR_OK;
}

int distr_depth_samples_backward(distr_ctx* ctx, const distr_samples_cfg* cfg, int32_t nviews, const int64_t* counts, const int32_t* index,
                                 const float* latent, int64_t latent_stride, const float* RT, const float* depth, const float* draws,
                                 const float* xyz, const float* g_out, float* g_latent, float* g_RT, void* ws, size_t ws_bytes,
                                 void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  SampPlan p;
  if (int rc = samp_cfg(ctx, cfg, nviews, p)) return rc;
  if (int rc = samp_counts(ctx, counts, p)) return rc;
  if (!ctx->has_decoder) return fail(ctx, DISTR_ERR_NO_DECODER, "distr_set_decoder has not been called");
  if (latent_stride != 0 && latent_stride < ctx->D.nlat) return fail(ctx, DISTR_ERR_INVALID_ARG, "latent_stride %lld: 0 (shared code) or >= %d", (long long)latent_stride, ctx->D.nlat);
  if (!index || !latent || !RT || !depth || !draws || !ws || (p.ntot > 0 && (!xyz || !g_out))) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  if (ws_bytes < samp_bwd_ws(nullptr, p).bytes) return fail(ctx, DISTR_ERR_WORKSPACE, "depth-samples backward workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const SampBwdWs w = samp_bwd_ws(ws, p);
  // one segmented point-list backward, a segment per view: every view keeps the tiles and the reduction order of its stand-alone call
  if (p.ntot > 0 || g_latent) {
    PointList pl;
    if (int rc = seg_list(ctx, nviews, p.seg, pl)) return rc;
    if (int rc = mlp_backward_list(ctx, pl, latent, latent_stride, xyz, g_out, cfg->clamp_dist, g_RT ? w.g_xyz : nullptr, g_latent, w.mlp, w.mlp_bytes, s))
      return rc;
  }
  if (g_RT) {
    hipLaunchKernelGGL(samples::k_samp_cam_bwd, dim3((unsigned)p.nblk_cam, (unsigned)nviews), dim3(samples::MB), 0, s, p.G, p.VW, index, RT, depth,
                       draws, (const float*)w.g_xyz, p.nblk_cam, w.part);
    LAUNCH_CHECK("k_samp_cam_bwd");
    hipLaunchKernelGGL(samples::k_samp_cam_fin, dim3((unsigned)nviews), dim3(samples::MB), 0, s, p.VW, RT, (const float*)w.part, p.nblk_cam, g_RT);
    LAUNCH_CHECK("k_samp_cam_fin");
  }
  return DISTR_OK;
}

}  // extern "C"

// ---- normal-map losses through the decoder's second path (include/distr_normal_grad.h, kernels: distr_normal_grad.hpp)
namespace {

struct NgWs {
  int *btot, *boff, *totals;
  int32_t* index;
  double* c64;               // [nviews][1024] lin0 / lin4 start values in float64 (k_ng_consts64)
  float *xyz, *gf, *g_xyz, *part;
  void* mlp;
  size_t mlp_bytes, bytes;
};

struct NgPlan {
  int nviews, P, nblk;       // nblk: blocks of MTILE pixels per view (count / compact / camera sums)
  PointList pl;              // the segmented list at its capacity: a segment of P points per view (the table holds the real counts)
};

// what the term is defined for, before any pointer is looked at (the workspace size and the call refuse alike)
int ng_plan(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, NgPlan& p) {
  if (int rc = check_cfg(ctx, cfg)) return rc;
  if (nviews < 1 || nviews > DISTR_MAX_VIEWS) return fail(ctx, DISTR_ERR_INVALID_ARG, "nviews %d not in [1, %d]", nviews, DISTR_MAX_VIEWS);
  if (cfg->use_depth2normal) return fail(ctx, DISTR_ERR_INVALID_ARG, "normal decoder gradient: use_depth2normal renders have no autograd normals, the term does not exist");
  if (!cfg->want_normal) return fail(ctx, DISTR_ERR_INVALID_ARG, "normal decoder gradient: the forward was run with want_normal=0");
  if (!cfg->save_for_backward) return fail(ctx, DISTR_ERR_INVALID_ARG, "normal decoder gradient: the forward was run with save_for_backward=0");
  if (cfg->rows != 0) return fail(ctx, DISTR_ERR_UNSUPPORTED, "normal decoder gradient: row bands (rows != 0) are not implemented");
  if (cfg->arith != DISTR_ARITH_F32) return fail(ctx, DISTR_ERR_UNSUPPORTED, "normal decoder gradient: arith f32 only");
  memset(&p, 0, sizeof(p));
  p.nviews = nviews;
  p.P = cfg->H * cfg->W;
  p.nblk = (p.P + ngrad::MTILE - 1) / ngrad::MTILE;
  int64_t cap[DISTR_MAX_VIEWS];
  for (int v = 0; v < nviews; ++v) cap[v] = p.P;
  return seg_list(ctx, nviews, cap, p.pl);         // (refuses more than 2^30 pixels in all)
}

NgWs ng_ws(void* base, NgPlan& p) {
  WsCarve c(base);
  NgWs w;
  const size_t NP = (size_t)p.nviews * p.P;
  w.btot = c.take<int>((size_t)p.nviews * p.nblk);
  w.boff = c.take<int>((size_t)p.nviews * p.nblk);
  w.totals = c.take<int>(DISTR_MAX_VIEWS);
  w.index = c.take<int32_t>(NP);
  w.c64 = c.take<double>((size_t)p.nviews * 2 * HID);
  w.xyz = c.take<float>(3 * NP);
  w.gf = c.take<float>(NP);
  w.g_xyz = c.take<float>(3 * NP);
  w.part = c.take<float>((size_t)p.nviews * p.nblk * 12);
  w.mlp_bytes = carve_list(nullptr, p.pl, true);
  w.mlp = c.take<char>(w.mlp_bytes);
  w.bytes = c.bytes();
  return w;
}

}  // namespace

extern "C" {

int distr_render_normal_grad_workspace_bytes(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, size_t* bytes) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  NgPlan p;
  if (int rc = ng_plan(ctx, cfg, nviews, p)) return rc;
  if (!bytes) return fail(ctx, DISTR_ERR_INVALID_ARG, "null pointer");
  *bytes = ng_ws(nullptr, p).bytes;
  return DISTR_OK;
}

int distr_render_normal_grad_backward_batch(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, const int32_t* view_flags,
                                            const void* ws_fwd, size_t ws_fwd_bytes, const float* g_normal, float* g_latent, float* g_R,
                                            float* g_T, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  NgPlan p;
  if (int rc = ng_plan(ctx, cfg, nviews, p)) return rc;
  ViewFlags vf;      // checked, not used: render_normal takes no no_grad_camera (renderer.py:881-882, 977)
  if (int rc = make_view_flags(ctx, *cfg, nviews, view_flags, vf)) return rc;
  if (!ctx->has_decoder) return fail(ctx, DISTR_ERR_NO_DECODER, "distr_set_decoder has not been called");
  if (!ws_fwd || !g_normal || !ws) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  View V;
  const size_t single = make_view(*cfg, const_cast<void*>(ws_fwd), V, ctx->save_masks, nviews);
  if (ws_fwd_bytes < single * nviews) return fail(ctx, DISTR_ERR_WORKSPACE, "forward workspace too small: %zu < %zu", ws_fwd_bytes, single * nviews);
  if (ws_bytes < ng_ws(nullptr, p).bytes) return fail(ctx, DISTR_ERR_WORKSPACE, "normal decoder gradient: workspace too small: %zu < %zu", ws_bytes, ng_ws(nullptr, p).bytes);
  hipStream_t s = (hipStream_t)stream;
  const DecoderDev& D = ctx->D;
  const unsigned NV = (unsigned)nviews;
  if (cfg->normalize_normal) {      // unit normals are scale invariant: no term
    if (g_latent) HIP_TRY(hipMemsetAsync(g_latent, 0, (size_t)nviews * D.nlat * sizeof(float), s));
    if (g_R) HIP_TRY(hipMemsetAsync(g_R, 0, (size_t)nviews * 9 * sizeof(float), s));
    if (g_T) HIP_TRY(hipMemsetAsync(g_T, 0, (size_t)nviews * 3 * sizeof(float), s));
    return DISTR_OK;
  }
  const NgWs w = ng_ws(ws, p);
  carve_list(w.mlp, p.pl, true);
  const dim3 gpx((unsigned)p.nblk, NV), gpt((unsigned)((p.P + ngrad::MB - 1) / ngrad::MB), NV), blk(ngrad::MB);
  hipLaunchKernelGGL(ngrad::k_ng_count, gpx, blk, 0, s, V, p.nblk, w.btot);
  LAUNCH_CHECK("k_ng_count");
  hipLaunchKernelGGL(samples::k_samp_top_scan, dim3(NV), blk, 0, s, (const int*)w.btot, p.nblk, w.boff, w.totals);
  LAUNCH_CHECK("k_samp_top_scan");
  hipLaunchKernelGGL(ngrad::k_ng_compact, gpx, blk, 0, s, V, p.nblk, (const int*)w.boff, w.index);
  LAUNCH_CHECK("k_ng_compact");
  const ngrad::Lists L{w.index, w.totals, w.xyz, w.gf, w.g_xyz};
  hipLaunchKernelGGL(ngrad::k_ng_gather, gpt, blk, 0, s, V, L, g_normal);
  LAUNCH_CHECK("k_ng_gather");
  hipLaunchKernelGGL(ngrad::k_ng_consts64, dim3(4, NV), dim3(256), 0, s, V, D, w.c64);
  LAUNCH_CHECK("k_ng_consts64");
  hipLaunchKernelGGL(ngrad::k_ng_f64, dim3((unsigned)((p.P + ngrad::FP - 1) / ngrad::FP), NV), dim3(256), 0, s, V, L, D, (const double*)w.c64,
                     (int)wide_decoder(ctx));
  LAUNCH_CHECK("k_ng_f64");
  // one segmented point-list backward, a segment per view (also for one view: the same tiles either way). The latent constants come
  // from the codes the forward saved (Consts::latent, a view every vstride bytes); the tile table from the counts on the device.
  const float* codes = reinterpret_cast<const float*>(reinterpret_cast<const char*>(V.C) + offsetof(Consts, latent));
  hipLaunchKernelGGL(k_latent_consts, dim3(4, NV), dim3(256), 0, s, p.pl.c0c4, D, codes, (int64_t)(V.vstride / (int64_t)sizeof(float)), (SegTable*)nullptr, p.pl.cnt);
  LAUNCH_CHECK("k_latent_consts");
  hipLaunchKernelGGL(ngrad::k_ng_seg_table, dim3(1), dim3(64), 0, s, (const int*)w.totals, nviews, p.P, p.pl.tab);
  LAUNCH_CHECK("k_ng_seg_table");
  BwdArgs B;
  memset(&B, 0, sizeof(B));
  B.xyz = w.xyz; B.c0c4 = p.pl.c0c4; B.seg = p.pl.tab; B.coef = w.gf; B.clamp = -1.0f; B.partial = p.pl.partial;
  B.out_g = (g_R || g_T) ? w.g_xyz : nullptr;
  if (int rc = launch_bwd(ctx, "k_bwd<pointgrad+latent>", BWD_POINTGRAD, 2, 0, wide_decoder(ctx), p.pl.tiles, s, B)) return rc;
  if (int rc = list_latent_grad(ctx, D, p.pl, g_latent, s)) return rc;
  if (g_R || g_T) {
    hipLaunchKernelGGL(ngrad::k_ng_cam_bwd, gpx, blk, 0, s, V, L, p.nblk, w.part);
    LAUNCH_CHECK("k_ng_cam_bwd");
    hipLaunchKernelGGL(ngrad::k_ng_cam_fin, dim3(NV), blk, 0, s, V, (const int*)w.totals, (const float*)w.part, p.nblk, g_R, g_T);
    LAUNCH_CHECK("k_ng_cam_fin");
  }
  return DISTR_OK;
}

}  // extern "C"

// ---- the colour stage of a batch of rendered views (include/distr_color_batch.h, kernels: distr_color_batch.hpp)
namespace {

struct CbPlan {
  int nviews, P, nblk;       // nblk: blocks of MTILE pixels per view (count / compact / camera sums)
  cbatch::Geo G;
  PointList pl;              // the segmented list at its capacity: a segment of P points per view (the table holds the real counts)
};

struct CbFwdWs {             // what the forward leaves for the backward
  int *btot, *boff, *totals;
  int32_t *index, *pos;      // [nviews][P] compacted valid pixels; list position of every pixel (-1 off the mask)
  float *xyz, *col;          // [nviews * P][3] surface points and their unshaded colours, view v from v * P on
  void* mlp;
  size_t mlp_bytes, bytes;
};

struct CbBwdWs {
  float *g_col, *g_xyz, *part;
  void* mlp;
  size_t mlp_bytes, bytes;
};

int cb_plan(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, CbPlan& p) {
  if (int rc = check_cfg(ctx, cfg)) return rc;
  if (nviews < 1 || nviews > DISTR_MAX_VIEWS) return fail(ctx, DISTR_ERR_INVALID_ARG, "nviews %d not in [1, %d]", nviews, DISTR_MAX_VIEWS);
  if (cfg->rows != 0) return fail(ctx, DISTR_ERR_UNSUPPORTED, "colour stage: row bands (rows != 0) are not implemented");
  memset(&p, 0, sizeof(p));
  p.nviews = nviews;
  p.P = cfg->H * cfg->W;
  p.nblk = (p.P + cbatch::MTILE - 1) / cbatch::MTILE;
  p.G.H = cfg->H; p.G.W = cfg->W; p.G.P = p.P;
  memcpy(p.G.Ki, cfg->K_inv, sizeof(p.G.Ki));
  memcpy(p.G.M, cfg->M, sizeof(p.G.M));
  int64_t cap[DISTR_MAX_VIEWS];
  for (int v = 0; v < nviews; ++v) cap[v] = p.P;
  return seg_list(ctx, nviews, cap, p.pl);         // (refuses more than 2^30 pixels in all)
}

CbFwdWs cb_fwd_ws(void* base, CbPlan& p) {
  WsCarve c(base);
  CbFwdWs w;
  const size_t NP = (size_t)p.nviews * p.P;
  w.btot = c.take<int>((size_t)p.nviews * p.nblk);
  w.boff = c.take<int>((size_t)p.nviews * p.nblk);
  w.totals = c.take<int>(DISTR_MAX_VIEWS);
  w.index = c.take<int32_t>(NP);
  w.pos = c.take<int32_t>(NP);
  w.xyz = c.take<float>(3 * NP);
  w.col = c.take<float>(3 * NP);
  w.mlp_bytes = carve_list(nullptr, p.pl, false);
  w.mlp = c.take<char>(w.mlp_bytes);
  w.bytes = c.bytes();
  return w;
}

CbBwdWs cb_bwd_ws(void* base, CbPlan& p) {
  WsCarve c(base);
  CbBwdWs w;
  const size_t NP = (size_t)p.nviews * p.P;
  w.g_col = c.take<float>(3 * NP);
  w.g_xyz = c.take<float>(3 * NP);
  w.part = c.take<float>((size_t)p.nviews * p.nblk * 12);
  w.mlp_bytes = carve_list(nullptr, p.pl, true);
  w.mlp = c.take<char>(w.mlp_bytes);
  w.bytes = c.bytes();
  return w;
}

// the lights of a call as the kernels take them, or why they are refused; `sets`: views (or frames) that index the strides
int cb_lights(distr_ctx* ctx, const distr_color_lights* in, bool have_normal, cbatch::Lights& L) {
  memset(&L, 0, sizeof(L));
  if (!in) return DISTR_OK;
  if (in->struct_size != sizeof(distr_color_lights)) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_color_lights.struct_size is %u, expected %zu", in->struct_size, sizeof(distr_color_lights));
  if (in->nlights < 0 || in->nlights > 4096) return fail(ctx, DISTR_ERR_INVALID_ARG, "nlights %d: 0..4096", in->nlights);
  if (in->nlights == 0) return DISTR_OK;
  if (!in->locations_dev || !in->energies_dev || !have_normal) return fail(ctx, DISTR_ERR_INVALID_ARG, "lights need locations, energies and the normal image");
  if ((in->location_stride != 0 && in->location_stride < 3 * (int64_t)in->nlights) || (in->energy_stride != 0 && in->energy_stride < in->nlights))
    return fail(ctx, DISTR_ERR_INVALID_ARG, "light strides: 0 (shared) or >= 3 M / M floats");
  L.loc = in->locations_dev; L.en = in->energies_dev; L.lstride = in->location_stride; L.estride = in->energy_stride; L.M = in->nlights;
  return DISTR_OK;
}

// the latent constants of every view's [shape | colour] code and the tile table from the counts on the device
int cb_list_setup(distr_ctx* ctx, CbPlan& p, const float* latent_cat, int64_t latent_stride, const int* totals, hipStream_t s) {
  hipLaunchKernelGGL(k_latent_consts, dim3(4, (unsigned)p.nviews), dim3(256), 0, s, p.pl.c0c4, ctx->DC, latent_cat, latent_stride, (SegTable*)nullptr, p.pl.cnt);
  LAUNCH_CHECK("k_latent_consts");
  hipLaunchKernelGGL(ngrad::k_ng_seg_table, dim3(1), dim3(64), 0, s, totals, p.nviews, p.P, p.pl.tab);
  LAUNCH_CHECK("k_ng_seg_table");
  return DISTR_OK;
}

int cb_common(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, int64_t latent_stride, CbPlan& p) {
  if (int rc = cb_plan(ctx, cfg, nviews, p)) return rc;
  if (!ctx->has_color) return fail(ctx, DISTR_ERR_NO_DECODER, "distr_set_color_decoder has not been called");
  if (latent_stride != 0 && latent_stride < ctx->DC.nlat) return fail(ctx, DISTR_ERR_INVALID_ARG, "latent_stride %lld: 0 (shared code) or >= %d", (long long)latent_stride, ctx->DC.nlat);
  return DISTR_OK;
}

}  // namespace

extern "C" {

int distr_color_stage_workspace_bytes(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, size_t* forward_bytes, size_t* backward_bytes) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  CbPlan p;
  if (int rc = cb_plan(ctx, cfg, nviews, p)) return rc;
  if (forward_bytes) *forward_bytes = cb_fwd_ws(nullptr, p).bytes;
  if (backward_bytes) *backward_bytes = cb_bwd_ws(nullptr, p).bytes;
  return DISTR_OK;
}

int distr_color_stage_forward_batch(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, const float* R, const float* T, const float* zdepth,
                                    const uint8_t* mask, const float* normal, const float* latent_cat, int64_t latent_stride,
                                    const distr_color_lights* lights, float* rgb, void* ws, size_t ws_bytes, int32_t* index_out, float* xyz_out,
                                    int32_t* totals_out, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  CbPlan p;
  if (int rc = cb_common(ctx, cfg, nviews, latent_stride, p)) return rc;
  if (!R || !T || !zdepth || !mask || !latent_cat || !rgb || !ws) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  cbatch::Lights L;
  if (int rc = cb_lights(ctx, lights, normal != nullptr, L)) return rc;
  if (ws_bytes < cb_fwd_ws(nullptr, p).bytes) return fail(ctx, DISTR_ERR_WORKSPACE, "colour stage: forward workspace too small: %zu < %zu", ws_bytes, cb_fwd_ws(nullptr, p).bytes);
  hipStream_t s = (hipStream_t)stream;
  const CbFwdWs w = cb_fwd_ws(ws, p);
  carve_list(w.mlp, p.pl, false);
  const unsigned NV = (unsigned)nviews;
  const dim3 gblk((unsigned)p.nblk, NV), gpx((unsigned)((p.P + cbatch::MB - 1) / cbatch::MB), NV), blk(cbatch::MB);
  const cbatch::Cams C{R, T, zdepth, normal, (int64_t)p.P};
  hipLaunchKernelGGL(cbatch::k_cb_count, gblk, blk, 0, s, mask, p.P, p.nblk, w.btot);
  LAUNCH_CHECK("k_cb_count");
  hipLaunchKernelGGL(samples::k_samp_top_scan, dim3(NV), blk, 0, s, (const int*)w.btot, p.nblk, w.boff, w.totals);
  LAUNCH_CHECK("k_samp_top_scan");
  hipLaunchKernelGGL(cbatch::k_cb_compact, gblk, blk, 0, s, mask, p.P, p.nblk, (const int*)w.boff, w.index, w.pos);
  LAUNCH_CHECK("k_cb_compact");
  hipLaunchKernelGGL(cbatch::k_cb_points, gpx, blk, 0, s, p.G, C, (const int32_t*)w.index, (const int*)w.totals, w.xyz);
  LAUNCH_CHECK("k_cb_points");
  if (int rc = cb_list_setup(ctx, p, latent_cat, latent_stride, w.totals, s)) return rc;
  if (int rc = color_eval_launch(ctx, p.pl, w.xyz, w.col, s)) return rc;
  hipLaunchKernelGGL(cbatch::k_cb_epilogue<true>, gpx, blk, 0, s, p.G, C, L, mask, (const int32_t*)w.pos, (const float*)w.col, rgb);
  LAUNCH_CHECK("k_cb_epilogue");
  const size_t NP = (size_t)nviews * p.P;
  if (index_out) HIP_TRY(hipMemcpyAsync(index_out, w.index, NP * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (xyz_out) HIP_TRY(hipMemcpyAsync(xyz_out, w.xyz, 3 * NP * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (totals_out) HIP_TRY(hipMemcpyAsync(totals_out, w.totals, (size_t)nviews * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  return DISTR_OK;
}

int distr_color_stage_backward_batch(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, const float* R, const float* T, const float* zdepth,
                                     const float* normal, const float* latent_cat, int64_t latent_stride, const distr_color_lights* lights,
                                     const void* ws_fwd, size_t ws_fwd_bytes, const float* g_rgb, float* g_latent_cat, float* g_R, float* g_T,
                                     float* g_normal, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  CbPlan p;
  if (int rc = cb_common(ctx, cfg, nviews, latent_stride, p)) return rc;
  if (!R || !T || !zdepth || !latent_cat || !ws_fwd || !g_rgb || !ws) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  cbatch::Lights L;
  if (int rc = cb_lights(ctx, lights, normal != nullptr, L)) return rc;
  if (ws_fwd_bytes < cb_fwd_ws(nullptr, p).bytes) return fail(ctx, DISTR_ERR_WORKSPACE, "colour stage: forward workspace too small: %zu < %zu", ws_fwd_bytes, cb_fwd_ws(nullptr, p).bytes);
  if (ws_bytes < cb_bwd_ws(nullptr, p).bytes) return fail(ctx, DISTR_ERR_WORKSPACE, "colour stage: backward workspace too small: %zu < %zu", ws_bytes, cb_bwd_ws(nullptr, p).bytes);
  hipStream_t s = (hipStream_t)stream;
  const CbFwdWs f = cb_fwd_ws(const_cast<void*>(ws_fwd), p);
  const CbBwdWs w = cb_bwd_ws(ws, p);
  carve_list(w.mlp, p.pl, true);
  const unsigned NV = (unsigned)nviews;
  const dim3 gblk((unsigned)p.nblk, NV), gpx((unsigned)((p.P + cbatch::MB - 1) / cbatch::MB), NV), blk(cbatch::MB);
  const cbatch::Cams C{R, T, zdepth, normal, (int64_t)p.P};
  const bool decoder = g_latent_cat != nullptr;      // null: the colours are constants, only the shading terms are left
  const bool camera = g_R || g_T;
  if (!L.M) g_normal = nullptr;                      // written with lights only
  if (decoder || g_normal) {
    hipLaunchKernelGGL(cbatch::k_cb_bwd_pre, gpx, blk, 0, s, p.G, C, L, (const int32_t*)f.pos, (const float*)f.col, g_rgb, decoder ? w.g_col : (float*)nullptr,
                       g_normal);
    LAUNCH_CHECK("k_cb_bwd_pre");
  }
  if (decoder) {
    if (int rc = cb_list_setup(ctx, p, latent_cat, latent_stride, f.totals, s)) return rc;
    if (int rc = color_bwd_launch(ctx, p.pl, f.xyz, w.g_col, camera ? w.g_xyz : (float*)nullptr, s)) return rc;
    if (int rc = list_latent_grad(ctx, ctx->DC, p.pl, g_latent_cat, s)) return rc;
  }
  if (camera) {
    if (!decoder && !L.M) {      // nothing reaches the camera
      if (g_R) HIP_TRY(hipMemsetAsync(g_R, 0, (size_t)nviews * 9 * sizeof(float), s));
      if (g_T) HIP_TRY(hipMemsetAsync(g_T, 0, (size_t)nviews * 3 * sizeof(float), s));
      return DISTR_OK;
    }
    hipLaunchKernelGGL(cbatch::k_cb_cam_bwd, gblk, blk, 0, s, p.G, C, L, (const int32_t*)f.index, (const int*)f.totals, (const float*)f.col, g_rgb,
                       decoder ? (const float*)w.g_xyz : (const float*)nullptr, p.nblk, w.part);
    LAUNCH_CHECK("k_cb_cam_bwd");
    hipLaunchKernelGGL(cbatch::k_cb_cam_fin, dim3(NV), blk, 0, s, p.G, C, (const int*)f.totals, (const float*)w.part, p.nblk, g_R, g_T);
    LAUNCH_CHECK("k_cb_cam_fin");
  }
  return DISTR_OK;
}

// ---- the decoder list of the stage's backward, written out (include/distr_color_train.h). The same two carves as the stage: f.totals,
// f.index and f.xyz are the forward's, w.g_col is what k_cb_bwd_pre wrote -- k_color_bwd reads it (const) and writes g_xyz and the tile
// partials, k_points_latent_grad and the camera kernels write regions of their own, so it is intact when the backward returns.
int distr_color_stage_samples_export_batch(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nviews, const void* ws_fwd, size_t ws_fwd_bytes,
                                           const void* ws_bwd, size_t ws_bwd_bytes, float* xyz_out, float* up_out, int32_t* index_out, int64_t cap,
                                           int32_t* counts_dev, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  CbPlan p;
  if (int rc = cb_plan(ctx, cfg, nviews, p)) return rc;
  if (!ws_fwd || !ws_bwd) return fail(ctx, DISTR_ERR_INVALID_ARG, "null workspace");
  if (!xyz_out || !up_out || !counts_dev) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  if (cap < (int64_t)p.P) return fail(ctx, DISTR_ERR_INVALID_ARG, "colour stage export: cap %lld is below the %d rows a view's list can hold", (long long)cap, p.P);
  if (ws_fwd_bytes < cb_fwd_ws(nullptr, p).bytes) return fail(ctx, DISTR_ERR_WORKSPACE, "colour stage: forward workspace too small: %zu < %zu", ws_fwd_bytes, cb_fwd_ws(nullptr, p).bytes);
  if (ws_bwd_bytes < cb_bwd_ws(nullptr, p).bytes) return fail(ctx, DISTR_ERR_WORKSPACE, "colour stage: backward workspace too small: %zu < %zu", ws_bwd_bytes, cb_bwd_ws(nullptr, p).bytes);
  const CbFwdWs f = cb_fwd_ws(const_cast<void*>(ws_fwd), p);
  const CbBwdWs w = cb_bwd_ws(const_cast<void*>(ws_bwd), p);
  hipLaunchKernelGGL(cbatch::k_cb_export, dim3((unsigned)((p.P + cbatch::MB - 1) / cbatch::MB), (unsigned)nviews), dim3(cbatch::MB), 0, (hipStream_t)stream, p.P,
                     (const int*)f.totals, (const int32_t*)f.index, (const float*)f.xyz, (const float*)w.g_col, xyz_out, up_out, index_out, cap, counts_dev);
  LAUNCH_CHECK("k_cb_export");
  return DISTR_OK;
}

// ---- the photometric loss of a batch of colour images (include/distr_color_train.h, kernels: distr_color_loss.hpp)
size_t distr_color_loss_workspace_bytes(int32_t H, int32_t W, int32_t nviews, int32_t backward) {
  if (H < 1 || W < 1 || (int64_t)H * W > ((int64_t)1 << 24) || nviews < 1 || nviews > DISTR_MAX_VIEWS) return 0;
  const size_t P = (size_t)H * W, nblk = (P + closs::CB - 1) / closs::CB;
  return (backward ? (size_t)nviews * P * 9 : (size_t)nviews * nblk * 3) * sizeof(float) + 256;
}

static int color_loss_args(distr_ctx* ctx, int32_t H, int32_t W, int32_t nviews, const void* ws, size_t ws_bytes, bool backward) {
  if (H < 1 || W < 1 || (int64_t)H * W > ((int64_t)1 << 24)) return fail(ctx, DISTR_ERR_INVALID_ARG, "colour loss: image size %d x %d: at least 1 x 1, at most 2^24 pixels", H, W);
  if (nviews < 1 || nviews > DISTR_MAX_VIEWS) return fail(ctx, DISTR_ERR_INVALID_ARG, "nviews %d not in [1, %d]", nviews, DISTR_MAX_VIEWS);
  const size_t need = distr_color_loss_workspace_bytes(H, W, nviews, backward ? 1 : 0);
  if (!ws || ws_bytes < need) return fail(ctx, DISTR_ERR_WORKSPACE, "colour loss: %s workspace too small: %zu < %zu", backward ? "backward" : "forward", ws ? ws_bytes : (size_t)0, need);
  return DISTR_OK;
}

int distr_color_loss_forward_batch(distr_ctx* ctx, int32_t H, int32_t W, int32_t nviews, const float* rgb, const uint8_t* mask, const float* gt,
                                   const uint8_t* gt_mask, int32_t want_ssim, float* l1_out, float* ssim_out, int32_t* overlap_out, void* ws,
                                   size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  if (!rgb || !mask || !gt || !gt_mask || !l1_out || !overlap_out || (want_ssim && !ssim_out)) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  if (int rc = color_loss_args(ctx, H, W, nviews, ws, ws_bytes, false)) return rc;
  const closs::Imgs I{H, W, H * W, rgb, gt, mask, gt_mask};
  const int nblk = (I.P + closs::CB - 1) / closs::CB;
  float* part = WsCarve(ws).take<float>((size_t)nviews * nblk * 3);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(closs::k_cl_fwd, dim3((unsigned)nblk, (unsigned)nviews), dim3(closs::CB), 0, s, I, want_ssim ? 1 : 0, nblk, part);
  LAUNCH_CHECK("k_cl_fwd");
  hipLaunchKernelGGL(closs::k_cl_fin, dim3((unsigned)nviews), dim3(closs::CB), 0, s, I.P, nblk, (const float*)part, l1_out, want_ssim ? ssim_out : (float*)nullptr, overlap_out);
  LAUNCH_CHECK("k_cl_fin");
  return DISTR_OK;
}

int distr_color_loss_backward_batch(distr_ctx* ctx, int32_t H, int32_t W, int32_t nviews, const float* rgb, const uint8_t* mask, const float* gt,
                                    const uint8_t* gt_mask, const int32_t* overlap_dev, const float* g_l1, const float* g_ssim, float* g_rgb_out,
                                    void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  if (!rgb || !mask || !gt || !gt_mask || !overlap_dev || !g_rgb_out) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  if (int rc = color_loss_args(ctx, H, W, nviews, ws, ws_bytes, true)) return rc;
  const closs::Imgs I{H, W, H * W, rgb, gt, mask, gt_mask};
  const dim3 grid((unsigned)((I.P + closs::CB - 1) / closs::CB), (unsigned)nviews);
  float* dpart = WsCarve(ws).take<float>((size_t)nviews * I.P * 9);
  hipStream_t s = (hipStream_t)stream;
  if (g_ssim) {
    hipLaunchKernelGGL(closs::k_cl_bwd_part, grid, dim3(closs::CB), 0, s, I, g_ssim, dpart);
    LAUNCH_CHECK("k_cl_bwd_part");
  }
  hipLaunchKernelGGL(closs::k_cl_bwd, grid, dim3(closs::CB), 0, s, I, g_l1, overlap_dev, g_ssim ? (const float*)dpart : (const float*)nullptr, g_rgb_out);
  LAUNCH_CHECK("k_cl_bwd");
  return DISTR_OK;
}

int distr_color_relight(distr_ctx* ctx, const distr_render_cfg* cfg, int32_t nframes, const float* R, const float* T, const float* zdepth,
                        const uint8_t* mask, const float* normal, const float* color, const distr_color_lights* lights, float* out, void* stream) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  CbPlan p;
  if (int rc = cb_plan(ctx, cfg, 1, p)) return rc;
  if (nframes < 1 || (int64_t)nframes * p.P > ((int64_t)1 << 30)) return fail(ctx, DISTR_ERR_INVALID_ARG, "nframes %d: at least 1, at most 2^30 pixels in all", nframes);
  if (nframes > 65535) return fail(ctx, DISTR_ERR_INVALID_ARG, "nframes %d: at most 65535 per call", nframes);
  if (!R || !T || !zdepth || !mask || !normal || !color || !out) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  cbatch::Lights L;
  if (int rc = cb_lights(ctx, lights, true, L)) return rc;
  if (!L.M) return fail(ctx, DISTR_ERR_INVALID_ARG, "relight needs at least one light");
  const cbatch::Cams C{R, T, zdepth, normal, (int64_t)0};
  const dim3 gpx((unsigned)((p.P + cbatch::MB - 1) / cbatch::MB), (unsigned)nframes), blk(cbatch::MB);
  hipLaunchKernelGGL(cbatch::k_cb_epilogue<false>, gpx, blk, 0, (hipStream_t)stream, p.G, C, L, mask, (const int32_t*)nullptr, color, out);
  LAUNCH_CHECK("k_cb_epilogue<relight>");
  return DISTR_OK;
}

}  // extern "C"

// ---- the layer-wise decoder path: weight gradients for decode_sdf (include/distr_train.h, distr_train.hpp)
namespace {

struct TrainPlan {
  int C, nseg;               // C: the code length L of the described net (section 8i)
  int n3, ld4, nout;         // lin3's rows, W4's row stride n3 + L + 3 (columns [lin3 outputs | code | xyz]), lin8's rows (1 or 3)
  int64_t n;                 // points
  int rows, blocks;          // padded rows, 64-row blocks
  int64_t slab_len; int nslab;
  train::Segs sg;
  int32_t seg_row[DISTR_MAX_VIEWS + 1];
  // workspace
  int32_t *rowpt, *blkseg, *blkpt0;
  float *c0c4, *xyz4, *X[9] /* 1..8 */, *z, *th, *dz, *D[2], *colpart, *colseg[3] /* lin0, lin4, the others */, *slabs;
  int out_w[9], in_w[9];     // GEMM widths: rows of W_l, and the columns of W_l that multiply the saved activation (lin4: n3)
  size_t bytes;              // what the carve takes
  train::DropArgs da;        // the call's dropout as the kernels take it (train_call)
  uint32_t drop_mask;
  // the carve of the grad_x f calls (section 8m), behind everything above: the padded upstream u4, the row scalars c1 / c2 / Q, the
  // row weights of k_train_colsum_w, the tangents tau_1..tau_8 (T[1] holds Delta_4 during the forward)
  bool grad;
  float *u4, *c1, *c2, *q, *rw, *T[9] /* 1..8 */;
};

void train_slab_plan(int64_t rows, int64_t* len, int* count) {
  // slab length: a multiple of 64 rows, at least SLAB_MIN, and long enough for MAX_SLABS slabs to cover the list
  const int64_t per = (rows + train::MAX_SLABS - 1) / train::MAX_SLABS;
  const int64_t L = std::max<int64_t>(train::SLAB_MIN, (per + train::TROW - 1) / train::TROW * train::TROW);
  *len = L;
  *count = (int)((rows + L - 1) / L);
}

constexpr int TRAIN_MAX_L = 65536;      // code length of a described net: keeps every index of W0 / W4 far inside an int

// L, n3, nout: the described net (distr_train_net); the SDF decoder of code length C is (C, 509 - C, 1)
int train_plan(distr_ctx* ctx, int32_t L, int32_t n3, int32_t nout, int32_t nseg, const int64_t* counts, TrainPlan& p) {
  memset(&p, 0, sizeof(p));
  PointList pl;
  if (int rc = seg_list(ctx, nseg, counts, pl)) return rc;
  if (nout != 1 && nout != 3) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_train_net: out_dim %d: 1 or 3", nout);
  if (n3 < 1 || n3 > HID - 3) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_train_net: lin3_rows %d: 1..%d", n3, HID - 3);
  if (L < 1 || L > TRAIN_MAX_L) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_train_net: latent_size %d: 1..%d", L, TRAIN_MAX_L);
  p.C = L; p.n3 = n3; p.ld4 = n3 + L + 3; p.nout = nout; p.nseg = nseg; p.n = pl.n;
  int64_t rows = 0;
  for (int s = 0; s < nseg; ++s) {
    p.sg.n[s] = (int32_t)counts[s];
    p.seg_row[s] = (int32_t)rows;
    rows += (counts[s] + train::TROW - 1) / train::TROW * train::TROW;
  }
  p.seg_row[nseg] = (int32_t)rows;
  p.rows = (int)rows; p.blocks = (int)(rows / train::TROW);
  train_slab_plan(rows, &p.slab_len, &p.nslab);
  for (int l = 0; l < 9; ++l) { p.out_w[l] = HID; p.in_w[l] = HID; }
  p.out_w[3] = n3; p.in_w[4] = n3; p.out_w[8] = nout; p.in_w[0] = 3;
  return DISTR_OK;
}

size_t train_carve(void* base, TrainPlan& p) {
  WsCarve c(base);
  const size_t R = (size_t)p.rows;
  p.rowpt = c.take<int32_t>(R); p.blkseg = c.take<int32_t>((size_t)p.blocks);
  p.c0c4 = c.take<float>((size_t)p.nseg * 2 * HID);
  p.xyz4 = c.take<float>(R * 4);
  for (int l = 1; l <= 8; ++l) p.X[l] = c.take<float>(R * HID);
  p.z = c.take<float>(R * p.nout); p.th = c.take<float>(R * p.nout); p.dz = c.take<float>(R * p.nout);
  p.D[0] = c.take<float>(R * HID); p.D[1] = c.take<float>(R * HID);
  p.colpart = c.take<float>((size_t)p.blocks * 4 * HID);
  for (int i = 0; i < 3; ++i) p.colseg[i] = c.take<float>((size_t)p.nseg * 4 * HID);
  p.slabs = c.take<float>((size_t)p.nslab * HID * HID);
  p.blkpt0 = c.take<int32_t>((size_t)p.blocks);      // (last: the offsets of everything above are those of the path without dropout)
  if (p.grad) {
    p.u4 = c.take<float>(R * 4); p.rw = c.take<float>(R * 4);
    p.c1 = c.take<float>(R); p.c2 = c.take<float>(R); p.q = c.take<float>(R);
    for (int l = 1; l <= 8; ++l) p.T[l] = c.take<float>(R * HID);
  }
  return c.bytes();
}

// plan and carve of a description (its pointers are not looked at): every size, offset and train call goes through here.
// base == nullptr: sizes and offsets only. grad: the calls of section 8m (out_dim 1 only), with their larger carve.
int train_layout(distr_ctx* ctx, const distr_train_net* net, int32_t nseg, const int64_t* counts, void* base, TrainPlan& p, bool grad = false) {
  if (!net || net->struct_size != sizeof(distr_train_net)) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_train_net: struct_size (use DISTR_INIT)");
  if (int rc = train_plan(ctx, net->latent_size, net->lin3_rows, net->out_dim, nseg, counts, p)) return rc;
  if (grad && p.nout != 1) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_train_grad: out_dim %d: the spatial gradient belongs to out_dim 1", p.nout);
  p.grad = grad;
  p.bytes = train_carve(base, p);
  return DISTR_OK;
}

inline int vec_ok(const void* p, int ld) { return ((uintptr_t)p % 16 == 0 && ld % 4 == 0) ? 1 : 0; }

// drop: null = the kernel without dropout, the code of the plain calls
template <bool A_K, bool B_K, int EPI>
int train_gemm(distr_ctx* ctx, const char* name, train::GemmArgs& g, int nz, hipStream_t s, const train::DropArgs* drop = nullptr) {
  g.vecA = vec_ok(g.A, g.lda); g.vecB = vec_ok(g.B, g.ldb);
  const dim3 grid((unsigned)((g.M + train::TBM - 1) / train::TBM), (unsigned)((g.N + train::TBN - 1) / train::TBN), (unsigned)nz);
  if constexpr (EPI != train::EPI_PART) {      // (the weight-gradient form has no dropout variant)
    if (drop) {
      hipLaunchKernelGGL((train::k_train_gemm_drop<A_K, B_K, EPI>), grid, dim3(256), 0, s, g, *drop);
      LAUNCH_CHECK(name);
      return DISTR_OK;
    }
  }
  hipLaunchKernelGGL((train::k_train_gemm<A_K, B_K, EPI>), grid, dim3(256), 0, s, g);
  LAUNCH_CHECK(name);
  return DISTR_OK;
}

// distr_train_dropout -> the kernels' arguments; active = false for null / layer_mask 0 (the plain path)
int train_drop_args(distr_ctx* ctx, const distr_train_dropout* d, int32_t nseg, train::DropArgs& a, uint32_t& layer_mask) {
  memset(&a, 0, sizeof(a));
  layer_mask = 0;
  if (!d) return DISTR_OK;
  if (d->struct_size != sizeof(distr_train_dropout)) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_train_dropout: struct_size (use DISTR_INIT)");
  if (d->layer_mask > 0xffu) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_train_dropout: layer_mask 0x%x: bits 0..7 (lin0..lin7)", d->layer_mask);
  if (!std::isfinite(d->scale) || d->scale < 1.f) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_train_dropout: scale %g: finite and >= 1", (double)d->scale);
  if (d->segment_base < 0 || d->segment_base + (int64_t)nseg > ((int64_t)1 << 32))
    return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_train_dropout: segment_base %lld: 0 .. 2^32 - nseg", (long long)d->segment_base);
  a.key0 = (uint32_t)(d->seed & 0xffffffffu); a.key1 = (uint32_t)(d->seed >> 32);
  a.thr = d->threshold; a.scale = d->scale; a.seg_base = (uint32_t)d->segment_base;
  layer_mask = d->layer_mask;
  return DISTR_OK;
}

// the nine W / b pairs of a description; name: the struct the caller passed, for the message
int train_pointers_ok(distr_ctx* ctx, const distr_train_net* net, const char* name) {
  for (int l = 0; l < 9; ++l)
    if (!net->W[l] || !net->b[l]) return fail(ctx, DISTR_ERR_INVALID_ARG, "%s: null pointer for lin%d", name, l);
  return DISTR_OK;
}

// the SDF decoder of code length C as a description: (C, 509 - C, 1), no pointers yet; false for a C outside 1..508
bool train_sdf_net(int32_t C, distr_train_net& n) {
  memset(&n, 0, sizeof(n));
  n.struct_size = sizeof(n); n.latent_size = C; n.lin3_rows = HID - 3 - C; n.out_dim = 1;
  return C >= 1 && C <= HID - 4;
}

// distr_train_weights -> the description of its SDF decoder (the pointers are checked by the entry)
int train_net_of(distr_ctx* ctx, const distr_train_weights* w, distr_train_net& n) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(ctx->mu);      // (a refusal writes the context's message)
  if (!w || w->struct_size != sizeof(distr_train_weights)) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_train_weights: struct_size (use DISTR_INIT)");
  if (!train_sdf_net(w->latent_size, n)) return fail(ctx, DISTR_ERR_INVALID_ARG, "latent_size %d: 1..%d", w->latent_size, HID - 4);
  for (int l = 0; l < 9; ++l) { n.W[l] = w->W[l]; n.b[l] = w->b[l]; }
  return DISTR_OK;
}

// g_W of one layer's activation columns: Delta^T X over the K slabs, then the slabs in order
// (ldo: the row stride of g_W -- ld4 for lin4, whose activation columns are the first n3 of its rows, 512 elsewhere)
int train_weight_grad(distr_ctx* ctx, const TrainPlan& p, const float* delta, int ldd, int M, const float* X, int N, float* g_W, int ldo, hipStream_t s) {
  train::GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = delta; g.lda = ldd; g.B = X; g.ldb = HID; g.Cout = p.slabs; g.ldc = N; g.M = M; g.N = N; g.K = p.rows;
  g.slab_len = (int)p.slab_len; g.slab_stride = (size_t)M * N;
  if (int rc = train_gemm<false, false, train::EPI_PART>(ctx, "k_train_gemm<weights>", g, p.nslab, s)) return rc;
  hipLaunchKernelGGL(train::k_train_slab_sum, grid1((int64_t)M * N), dim3(256), 0, s, (const float*)p.slabs, p.nslab, M, N, g_W, ldo);
  LAUNCH_CHECK("k_train_slab_sum");
  return DISTR_OK;
}

// column sums of a delta per segment (slot of p.colseg), then g_b and (lin0 / lin4: g_W non-null) the xyz and latent columns of g_W
int train_bias_grad(distr_ctx* ctx, const TrainPlan& p, const float* delta, int ldd, int ncols, bool moments, float* seg, float* g_b, float* g_W, int ldw,
                    int lat_col, int xyz_col, const float* latent, int64_t latent_stride, hipStream_t s) {
  hipLaunchKernelGGL(train::k_train_colsum, dim3((unsigned)p.blocks), dim3(256), 0, s, delta, ldd, ncols, moments ? (const float*)p.xyz4 : (const float*)nullptr, p.colpart);
  LAUNCH_CHECK("k_train_colsum");
  hipLaunchKernelGGL(train::k_train_colsum_seg, dim3((unsigned)p.nseg, HID / 32, moments ? 4 : 1), dim3(256), 0, s, (const float*)p.colpart, p.sg, ncols, seg);
  LAUNCH_CHECK("k_train_colsum_seg");
  hipLaunchKernelGGL(train::k_train_bias, dim3((unsigned)ncols), dim3(256), 0, s, (const float*)seg, p.nseg, g_b, g_W, ldw, lat_col, xyz_col, g_W ? p.C : 0, latent,
                     latent_stride);
  LAUNCH_CHECK("k_train_bias");
  return DISTR_OK;
}

int train_grads_ok(distr_ctx* ctx, const distr_train_grads* gr) {
  if (!gr || gr->struct_size != sizeof(distr_train_grads)) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_train_grads: struct_size (use DISTR_INIT)");
  for (int l = 0; l < 9; ++l)
    if (!gr->g_W[l] || !gr->g_b[l]) return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_train_grads: null pointer for lin%d", l);
  return DISTR_OK;
}

// THE check of a train call's arguments, forward and backward alike (the caller holds the EntryGuard). name: the struct the caller
// passed its weights in. gr: the backward's gradients (backward = true). io: the per-point array, xyz or the upstream gradient.
// Leaves the plan carved on the caller's workspace, with the dropout as the kernels take it.
int train_call(distr_ctx* ctx, const distr_train_net* net, const char* name, int32_t nseg, const int64_t* counts, const float* latent, int64_t latent_stride,
               const float* io, float clamp, void* ws, const distr_train_dropout* drop, bool backward, const distr_train_grads* gr, TrainPlan& p,
               bool grad = false) {
  if (int rc = train_layout(ctx, net, nseg, counts, ws, p, grad)) return rc;
  if (int rc = train_pointers_ok(ctx, net, name)) return rc;
  if (int rc = train_drop_args(ctx, drop, nseg, p.da, p.drop_mask)) return rc;
  if (backward)
    if (int rc = train_grads_ok(ctx, gr)) return rc;
  if (p.nout != 1 && clamp >= 0.f)
    return fail(ctx, DISTR_ERR_INVALID_ARG, "distr_train_net: clamp_dist %g with out_dim %d: a clamp belongs to out_dim 1 (pass a negative value)", (double)clamp, p.nout);
  if (latent_stride != 0 && latent_stride < p.C) return fail(ctx, DISTR_ERR_INVALID_ARG, "latent_stride %lld: 0 (shared code) or >= %d", (long long)latent_stride, p.C);
  if (!latent || !ws || (p.n > 0 && !io)) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  return DISTR_OK;
}

// the forward's launch sequence on a checked call
int train_forward_launch(distr_ctx* ctx, const distr_train_net* w, TrainPlan& p, const float* latent, int64_t latent_stride, const float* xyz, float clamp,
                         float* sdf, void* stream) {
  const int C = p.C;
  if (p.rows == 0) return DISTR_OK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(train::k_train_rows, grid1(p.rows), dim3(256), 0, s, p.sg, p.nseg, p.rows, p.rowpt, p.blkseg, p.blkpt0);
  LAUNCH_CHECK("k_train_rows");
  p.da.blkseg = p.blkseg; p.da.blkpt0 = p.blkpt0;
  hipLaunchKernelGGL(train::k_train_consts, dim3(4, (unsigned)p.nseg), dim3(256), 0, s, p.c0c4, w->W[0], w->b[0], w->W[4], w->b[4], C, p.ld4, p.n3, latent, latent_stride);
  LAUNCH_CHECK("k_train_consts");
  if (p.drop_mask & 1u) {
    p.da.layer = 0;
    hipLaunchKernelGGL(train::k_train_lin0_drop, dim3((unsigned)p.blocks), dim3(256), 0, s, xyz, (const int32_t*)p.rowpt, (const int32_t*)p.blkseg, (const float*)p.c0c4,
                       w->W[0], C, p.X[1], p.xyz4, p.da);
  } else
    hipLaunchKernelGGL(train::k_train_lin0, dim3((unsigned)p.blocks), dim3(256), 0, s, xyz, (const int32_t*)p.rowpt, (const int32_t*)p.blkseg, (const float*)p.c0c4, w->W[0], C,
                       p.X[1], p.xyz4);
  LAUNCH_CHECK("k_train_lin0");
  for (int l = 1; l <= 8; ++l) {
    train::GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = p.X[l]; g.lda = HID; g.B = w->W[l]; g.ldb = l == 4 ? p.ld4 : HID; g.M = p.rows; g.N = p.out_w[l]; g.K = p.in_w[l];
    g.Cout = l < 8 ? p.X[l + 1] : p.z; g.ldc = l < 8 ? HID : p.nout; g.relu = l < 8;
    if (l == 4) {      // the accumulator starts from c4[segment]; xyz follows the lin3 outputs (and the code) in k order
      g.ctab = p.c0c4 + HID; g.ctab_stride = 2 * HID; g.blkseg = p.blkseg;
      g.tailW = w->W[4] + (p.ld4 - 3); g.tail_ld = p.ld4; g.xyz4 = p.xyz4;
    } else g.bias = w->b[l];
    p.da.layer = (uint32_t)l;
    if (int rc = train_gemm<true, true, train::EPI_FWD>(ctx, "k_train_gemm<forward>", g, 1, s, (l < 8 && (p.drop_mask >> l & 1u)) ? &p.da : nullptr)) return rc;
  }
  hipLaunchKernelGGL(train::k_train_out, grid1((int64_t)p.rows * p.nout), dim3(256), 0, s, (const float*)p.z, (const int32_t*)p.rowpt, p.rows, p.nout, clamp, p.th, sdf);
  LAUNCH_CHECK("k_train_out");
  return DISTR_OK;
}

// an empty list: every gradient is zero
int train_zero_grads(distr_ctx* ctx, const TrainPlan& p, const distr_train_grads* gr, float* g_latent, hipStream_t s) {
  for (int l = 0; l < 9; ++l) {
    const size_t in = l == 0 ? (size_t)p.C + 3 : l == 4 ? (size_t)p.ld4 : HID;
    HIP_TRY(hipMemsetAsync(gr->g_W[l], 0, (size_t)p.out_w[l] * in * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(gr->g_b[l], 0, (size_t)p.out_w[l] * sizeof(float), s));
  }
  if (g_latent) HIP_TRY(hipMemsetAsync(g_latent, 0, (size_t)p.nseg * p.C * sizeof(float), s));
  return DISTR_OK;
}

// the backward's launch sequence on a checked call
int train_backward_launch(distr_ctx* ctx, const distr_train_net* w, TrainPlan& p, const float* latent, int64_t latent_stride, const float* g_sdf, float clamp,
                          const distr_train_grads* gr, float* g_latent, void* stream) {
  const int C = p.C, nseg = p.nseg;
  hipStream_t s = (hipStream_t)stream;
  if (p.rows == 0) return train_zero_grads(ctx, p, gr, g_latent, s);
  hipLaunchKernelGGL(train::k_train_dz, grid1((int64_t)p.rows * p.nout), dim3(256), 0, s, g_sdf, (const float*)p.th, (const int32_t*)p.rowpt, p.rows, p.nout, clamp, p.dz);
  LAUNCH_CHECK("k_train_dz");
  // lin8: its delta is dz, nout columns
  if (int rc = train_weight_grad(ctx, p, p.dz, p.nout, p.nout, p.X[8], HID, gr->g_W[8], HID, s)) return rc;
  if (int rc = train_bias_grad(ctx, p, p.dz, p.nout, p.nout, false, p.colseg[2], gr->g_b[8], nullptr, 0, 0, 0, latent, latent_stride, s)) return rc;
  const float* delta = p.dz;
  int ldd = p.nout, cur = 0;
  for (int l = 8; l >= 1; --l) {
    // delta of lin(l-1) = (delta of lin_l) W_l, gated by the saved relu output X_l; lin4: its lin3 columns only
    train::GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = delta; g.lda = ldd; g.B = w->W[l]; g.ldb = l == 4 ? p.ld4 : HID; g.M = p.rows; g.N = p.in_w[l]; g.K = p.out_w[l];
    g.Cout = p.D[cur]; g.ldc = HID; g.gate = p.X[l]; g.ldg = HID;
    // X_l went through lin(l-1)'s dropout: a dropped unit is an exact zero there, a kept one carries the factor scale
    if (int rc = train_gemm<true, false, train::EPI_GATE>(ctx, "k_train_gemm<delta>", g, 1, s, (p.drop_mask >> (l - 1) & 1u) ? &p.da : nullptr)) return rc;
    delta = p.D[cur]; ldd = HID; cur ^= 1;
    const int m = l - 1;       // delta now belongs to lin m
    if (m >= 1) {
      if (int rc = train_weight_grad(ctx, p, delta, HID, p.out_w[m], p.X[m], p.in_w[m], gr->g_W[m], m == 4 ? p.ld4 : HID, s)) return rc;
      if (int rc = train_bias_grad(ctx, p, delta, HID, p.out_w[m], m == 4, p.colseg[m == 4 ? 1 : 2], gr->g_b[m], m == 4 ? gr->g_W[4] : nullptr, p.ld4, p.n3,
                                   p.ld4 - 3, latent, latent_stride, s))
        return rc;
    } else {
      if (int rc = train_bias_grad(ctx, p, delta, HID, HID, true, p.colseg[0], gr->g_b[0], gr->g_W[0], C + 3, 0, C, latent, latent_stride, s)) return rc;
    }
  }
  if (g_latent) {
    hipLaunchKernelGGL(train::k_train_glatent, dim3((unsigned)((C + 255) / 256), (unsigned)p.nseg), dim3(256), 0, s, (const float*)p.colseg[0], (const float*)p.colseg[1], w->W[0],
                       w->W[4], C, p.ld4, p.n3, g_latent);
    LAUNCH_CHECK("k_train_glatent");
  }
  return DISTR_OK;
}


// THE way into the forward: every public forward is this call on a description
int train_forward_entry(distr_ctx* ctx, const distr_train_net* net, const char* name, int32_t nseg, const int64_t* counts, const float* latent, int64_t latent_stride,
                        const float* xyz, float clamp, float* out, void* ws, size_t ws_bytes, void* stream, const distr_train_dropout* drop) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  TrainPlan p;
  if (int rc = train_call(ctx, net, name, nseg, counts, latent, latent_stride, xyz, clamp, ws, drop, false, nullptr, p)) return rc;
  if (p.n > 0 && !out) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  if (ws_bytes < p.bytes) return fail(ctx, DISTR_ERR_WORKSPACE, "layer-wise decoder: workspace too small");
  return train_forward_launch(ctx, net, p, latent, latent_stride, xyz, clamp, out, stream);
}

// THE way into the backward
int train_backward_entry(distr_ctx* ctx, const distr_train_net* net, const char* name, int32_t nseg, const int64_t* counts, const float* latent, int64_t latent_stride,
                         const float* g_out, float clamp, void* ws, const distr_train_grads* gr, float* g_latent, void* stream, const distr_train_dropout* drop) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  TrainPlan p;
  if (int rc = train_call(ctx, net, name, nseg, counts, latent, latent_stride, g_out, clamp, ws, drop, true, gr, p)) return rc;
  return train_backward_launch(ctx, net, p, latent, latent_stride, g_out, clamp, gr, g_latent, stream);
}

// ---- the spatial gradient g = grad_x f with gradients to the weights

// one step of the unit-delta chain: Delta_(l-1) = G_(l-1) (Delta_l W_l) into `out`, lin4: its lin3 columns only (the delta GEMM of
// train_backward_launch with an upstream of one)
int train_unit_delta(distr_ctx* ctx, const distr_train_net* w, TrainPlan& p, int l, const float* delta, int ldd, float* out, hipStream_t s) {
  train::GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = delta; g.lda = ldd; g.B = w->W[l]; g.ldb = l == 4 ? p.ld4 : HID; g.M = p.rows; g.N = p.in_w[l]; g.K = p.out_w[l];
  g.Cout = out; g.ldc = HID; g.gate = p.X[l]; g.ldg = HID;
  return train_gemm<true, false, train::EPI_GATE>(ctx, "k_train_gemm<delta>", g, 1, s, (p.drop_mask >> (l - 1) & 1u) ? &p.da : nullptr);
}

// f as train_forward_launch without a clamp, then the unit deltas 8 -> 0 (Delta_4 kept in T[1]) and k_train_gx
int train_grad_forward_launch(distr_ctx* ctx, const distr_train_net* w, TrainPlan& p, const float* latent, int64_t latent_stride, const float* xyz,
                              float* sdf, float* grad, void* stream) {
  if (p.rows == 0) return DISTR_OK;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = train_forward_launch(ctx, w, p, latent, latent_stride, xyz, -1.f, sdf, stream)) return rc;
  hipLaunchKernelGGL(train::k_train_unit, grid1(p.rows), dim3(256), 0, s, (const int32_t*)p.rowpt, p.rows, p.dz);
  LAUNCH_CHECK("k_train_unit");
  const float* delta = p.dz;
  int ldd = 1, cur = 0;
  for (int l = 8; l >= 1; --l) {
    float* out = l == 5 ? p.T[1] : p.D[cur];      // l == 5: Delta_4, read again at the end
    if (int rc = train_unit_delta(ctx, w, p, l, delta, ldd, out, s)) return rc;
    delta = out; ldd = HID;
    if (l != 5) cur ^= 1;
  }
  hipLaunchKernelGGL(train::k_train_gx, dim3((unsigned)p.blocks), dim3(256), 0, s, delta, (const float*)p.T[1], w->W[0], w->W[4], p.C, p.ld4, (const float*)p.th,
                     (const int32_t*)p.rowpt, grad);
  LAUNCH_CHECK("k_train_gx");
  return DISTR_OK;
}

// weighted column sums of a unit delta (k_train_colsum_w on p.rw), then as train_bias_grad: g_b and, for lin0 / lin4, the xyz and
// latent columns of g_W
int train_bias_grad_w(distr_ctx* ctx, const TrainPlan& p, const float* delta, int ldd, int ncols, bool moments, float* seg, float* g_b, float* g_W, int ldw,
                      int lat_col, int xyz_col, const float* latent, int64_t latent_stride, hipStream_t s) {
  hipLaunchKernelGGL(train::k_train_colsum_w, dim3((unsigned)p.blocks), dim3(256), 0, s, delta, ldd, ncols, (const float*)p.rw, moments ? 1 : 0, p.colpart);
  LAUNCH_CHECK("k_train_colsum_w");
  hipLaunchKernelGGL(train::k_train_colsum_seg, dim3((unsigned)p.nseg, HID / 32, moments ? 4 : 1), dim3(256), 0, s, (const float*)p.colpart, p.sg, ncols, seg);
  LAUNCH_CHECK("k_train_colsum_seg");
  hipLaunchKernelGGL(train::k_train_bias, dim3((unsigned)ncols), dim3(256), 0, s, (const float*)seg, p.nseg, g_b, g_W, ldw, lat_col, xyz_col, g_W ? p.C : 0, latent,
                     latent_stride);
  LAUNCH_CHECK("k_train_bias");
  return DISTR_OK;
}

// g_W's activation columns of lin m: the combined operand c2 X_m + c1 tau_m (in tau_m's buffer), then Delta_m^T times it
int train_weight_grad_w(distr_ctx* ctx, const TrainPlan& p, int m, const float* delta, int ldd, float* g_W, hipStream_t s) {
  hipLaunchKernelGGL(train::k_train_combine, grid1((int64_t)p.rows * (HID / 4)), dim3(256), 0, s, (const float*)p.X[m], (const float*)p.c1, (const float*)p.c2, p.rows,
                     p.in_w[m], p.T[m]);
  LAUNCH_CHECK("k_train_combine");
  return train_weight_grad(ctx, p, delta, ldd, p.out_w[m], p.T[m], p.in_w[m], g_W, m == 4 ? p.ld4 : HID, s);
}

// the backward for the upstreams phi = dL/df (g_sdf) and u = dL/dg (g_grad), either may be null = 0, on the workspace of
// train_grad_forward_launch: the tangents forward, the row scalars, then the walk 8 -> 1 with the unit deltas recomputed
int train_grad_backward_launch(distr_ctx* ctx, const distr_train_net* w, TrainPlan& p, const float* latent, int64_t latent_stride, const float* g_sdf,
                               const float* g_grad, const distr_train_grads* gr, float* g_latent, void* stream) {
  const int C = p.C;
  hipStream_t s = (hipStream_t)stream;
  if (p.rows == 0) return train_zero_grads(ctx, p, gr, g_latent, s);
  hipLaunchKernelGGL(train::k_train_tan0, dim3((unsigned)p.blocks), dim3(256), 0, s, g_grad, (const int32_t*)p.rowpt, w->W[0], C, (const float*)p.X[1],
                     (p.drop_mask & 1u) ? p.da.scale : 1.f, p.T[1], p.u4);
  LAUNCH_CHECK("k_train_tan0");
  for (int l = 1; l <= 8; ++l) {      // tau_(l+1) = G_l (W_l tau_l), lin4 with u again behind its lin3 columns; l = 8: Q, no gate
    train::GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = p.T[l]; g.lda = HID; g.B = w->W[l]; g.ldb = l == 4 ? p.ld4 : HID; g.M = p.rows; g.N = p.out_w[l]; g.K = p.in_w[l];
    g.Cout = l < 8 ? p.T[l + 1] : p.q; g.ldc = l < 8 ? HID : 1;
    if (l < 8) { g.gate = p.X[l + 1]; g.ldg = HID; }
    if (l == 4) { g.tailW = w->W[4] + (p.ld4 - 3); g.tail_ld = p.ld4; g.xyz4 = p.u4; }
    if (int rc = train_gemm<true, true, train::EPI_TAN>(ctx, "k_train_gemm<tangent>", g, 1, s, (l < 8 && (p.drop_mask >> l & 1u)) ? &p.da : nullptr)) return rc;
  }
  hipLaunchKernelGGL(train::k_train_rowscal, grid1(p.rows), dim3(256), 0, s, g_sdf, (const float*)p.th, (const float*)p.q, (const int32_t*)p.rowpt, (const float*)p.xyz4,
                     (const float*)p.u4, p.rows, p.c1, p.c2, p.rw, p.dz);
  LAUNCH_CHECK("k_train_rowscal");
  // lin8: Delta_8 = p.dz, one column
  if (int rc = train_weight_grad_w(ctx, p, 8, p.dz, 1, gr->g_W[8], s)) return rc;
  if (int rc = train_bias_grad_w(ctx, p, p.dz, 1, 1, false, p.colseg[2], gr->g_b[8], nullptr, 0, 0, 0, latent, latent_stride, s)) return rc;
  const float* delta = p.dz;
  int ldd = 1, cur = 0;
  for (int l = 8; l >= 1; --l) {
    if (int rc = train_unit_delta(ctx, w, p, l, delta, ldd, p.D[cur], s)) return rc;
    delta = p.D[cur]; ldd = HID; cur ^= 1;
    const int m = l - 1;       // delta now belongs to lin m
    if (m >= 1) {
      if (int rc = train_weight_grad_w(ctx, p, m, delta, HID, gr->g_W[m], s)) return rc;
      if (int rc = train_bias_grad_w(ctx, p, delta, HID, p.out_w[m], m == 4, p.colseg[m == 4 ? 1 : 2], gr->g_b[m], m == 4 ? gr->g_W[4] : nullptr, p.ld4, p.n3,
                                     p.ld4 - 3, latent, latent_stride, s))
        return rc;
    } else {
      if (int rc = train_bias_grad_w(ctx, p, delta, HID, HID, true, p.colseg[0], gr->g_b[0], gr->g_W[0], C + 3, 0, C, latent, latent_stride, s)) return rc;
    }
  }
  if (g_latent) {
    hipLaunchKernelGGL(train::k_train_glatent, dim3((unsigned)((C + 255) / 256), (unsigned)p.nseg), dim3(256), 0, s, (const float*)p.colseg[0], (const float*)p.colseg[1], w->W[0],
                       w->W[4], C, p.ld4, p.n3, g_latent);
    LAUNCH_CHECK("k_train_glatent");
  }
  return DISTR_OK;
}

// workspace bytes (layer 0) or the byte offset of X_layer (1..8) behind the aligned base; 0 for what the calls refuse
size_t train_bytes_or_offset(const distr_train_net* net, int32_t nseg, const int64_t* counts, int32_t layer, bool grad = false) {
  TrainPlan p;
  if (layer < 0 || layer > 8 || train_layout(nullptr, net, nseg, counts, nullptr, p, grad) != DISTR_OK) return 0;
  return layer ? (size_t)((uintptr_t)p.X[layer] - (uintptr_t)p.rowpt) : p.bytes;
}

}  // namespace

extern "C" {

size_t distr_train_workspace_bytes(int32_t latent_size, int32_t nseg, const int64_t* counts_host) {
  distr_train_net net;
  return train_sdf_net(latent_size, net) ? train_bytes_or_offset(&net, nseg, counts_host, 0) : 0;
}

size_t distr_train_activation_offset(int32_t latent_size, int32_t nseg, const int64_t* counts_host, int32_t layer) {
  distr_train_net net;
  return layer >= 1 && train_sdf_net(latent_size, net) ? train_bytes_or_offset(&net, nseg, counts_host, layer) : 0;
}

size_t distr_train_net_workspace_bytes(const distr_train_net* net, int32_t nseg, const int64_t* counts_host) {
  return train_bytes_or_offset(net, nseg, counts_host, 0);
}

size_t distr_train_net_activation_offset(const distr_train_net* net, int32_t nseg, const int64_t* counts_host, int32_t layer) {
  return layer >= 1 ? train_bytes_or_offset(net, nseg, counts_host, layer) : 0;
}

int64_t distr_train_segment_row(int32_t nseg, const int64_t* counts_host, int32_t seg) {
  TrainPlan p;
  if (seg < 0 || seg > nseg || train_plan(nullptr, 1, 1, 1, nseg, counts_host, p) != DISTR_OK) return -1;
  return p.seg_row[seg];
}

int distr_train_dropout_keep(uint64_t seed, uint32_t threshold, int32_t layer, int64_t segment, int64_t point, int32_t unit) {
  const Philox4 u = dropout_draws((uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), (uint32_t)layer, (uint32_t)segment, (uint32_t)(point >> 2), (uint32_t)unit);
  return u.v[point & 3] >= threshold ? 1 : 0;
}

void distr_train_slab_plan(int64_t rows, int64_t* slab_len, int32_t* num_slabs) {
  int64_t L = 0; int n = 0;
  train_slab_plan(rows < 0 ? 0 : rows, &L, &n);
  if (slab_len) *slab_len = L;
  if (num_slabs) *num_slabs = n;
}

int distr_train_forward(distr_ctx* ctx, const distr_train_weights* w, int32_t nseg, const int64_t* counts_host, const float* latent, int64_t latent_stride,
                        const float* xyz, float clamp, float* sdf, void* ws, size_t ws_bytes, void* stream) {
  return distr_train_forward_dropout(ctx, w, nseg, counts_host, latent, latent_stride, xyz, clamp, sdf, ws, ws_bytes, stream, nullptr);
}

int distr_train_forward_dropout(distr_ctx* ctx, const distr_train_weights* w, int32_t nseg, const int64_t* counts_host, const float* latent, int64_t latent_stride,
                                const float* xyz, float clamp, float* sdf, void* ws, size_t ws_bytes, void* stream, const distr_train_dropout* drop) {
  distr_train_net net;
  if (int rc = train_net_of(ctx, w, net)) return rc;
  return train_forward_entry(ctx, &net, "distr_train_weights", nseg, counts_host, latent, latent_stride, xyz, clamp, sdf, ws, ws_bytes, stream, drop);
}

int distr_train_net_forward(distr_ctx* ctx, const distr_train_net* net, int32_t nseg, const int64_t* counts_host, const float* latent, int64_t latent_stride,
                            const float* xyz, float clamp, float* out, void* ws, size_t ws_bytes, void* stream, const distr_train_dropout* drop) {
  return train_forward_entry(ctx, net, "distr_train_net", nseg, counts_host, latent, latent_stride, xyz, clamp, out, ws, ws_bytes, stream, drop);
}

int distr_train_backward(distr_ctx* ctx, const distr_train_weights* w, int32_t nseg, const int64_t* counts_host, const float* latent, int64_t latent_stride,
                         const float* g_sdf, float clamp, void* ws, const distr_train_grads* gr, float* g_latent, void* stream) {
  return distr_train_backward_dropout(ctx, w, nseg, counts_host, latent, latent_stride, g_sdf, clamp, ws, gr, g_latent, stream, nullptr);
}

int distr_train_backward_dropout(distr_ctx* ctx, const distr_train_weights* w, int32_t nseg, const int64_t* counts_host, const float* latent, int64_t latent_stride,
                                 const float* g_sdf, float clamp, void* ws, const distr_train_grads* gr, float* g_latent, void* stream,
                                 const distr_train_dropout* drop) {
  distr_train_net net;
  if (int rc = train_net_of(ctx, w, net)) return rc;
  return train_backward_entry(ctx, &net, "distr_train_weights", nseg, counts_host, latent, latent_stride, g_sdf, clamp, ws, gr, g_latent, stream, drop);
}

int distr_train_net_backward(distr_ctx* ctx, const distr_train_net* net, int32_t nseg, const int64_t* counts_host, const float* latent, int64_t latent_stride,
                             const float* g_out, float clamp, void* ws, const distr_train_grads* gr, float* g_latent, void* stream,
                             const distr_train_dropout* drop) {
  return train_backward_entry(ctx, net, "distr_train_net", nseg, counts_host, latent, latent_stride, g_out, clamp, ws, gr, g_latent, stream, drop);
}

size_t distr_train_grad_workspace_bytes(const distr_train_net* net, int32_t nseg, const int64_t* counts_host) {
  return train_bytes_or_offset(net, nseg, counts_host, 0, true);
}

int distr_train_grad_forward(distr_ctx* ctx, const distr_train_net* net, int32_t nseg, const int64_t* counts_host, const float* latent, int64_t latent_stride,
                             const float* xyz, float* sdf, float* grad, void* ws, size_t ws_bytes, void* stream, const distr_train_dropout* drop) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  TrainPlan p;
  if (int rc = train_call(ctx, net, "distr_train_net", nseg, counts_host, latent, latent_stride, xyz, -1.f, ws, drop, false, nullptr, p, true)) return rc;
  if (p.n > 0 && (!sdf || !grad)) return fail(ctx, DISTR_ERR_INVALID_ARG, "null device pointer");
  if (ws_bytes < p.bytes) return fail(ctx, DISTR_ERR_WORKSPACE, "layer-wise decoder: workspace too small");
  return train_grad_forward_launch(ctx, net, p, latent, latent_stride, xyz, sdf, grad, stream);
}

int distr_train_grad_backward(distr_ctx* ctx, const distr_train_net* net, int32_t nseg, const int64_t* counts_host, const float* latent, int64_t latent_stride,
                              const float* g_sdf, const float* g_grad, void* ws, const distr_train_grads* gr, float* g_latent, void* stream,
                              const distr_train_dropout* drop) {
  if (!ctx) return DISTR_ERR_INVALID_ARG;
  EntryGuard guard_(ctx);
  TrainPlan p;
  const float* io = g_sdf ? g_sdf : g_grad ? g_grad : latent;      // (both upstreams null: all zero, no per-point array to check)
  if (int rc = train_call(ctx, net, "distr_train_net", nseg, counts_host, latent, latent_stride, io, -1.f, ws, drop, true, gr, p, true)) return rc;
  return train_grad_backward_launch(ctx, net, p, latent, latent_stride, g_sdf, g_grad, gr, g_latent, stream);
}

}  // extern "C"
