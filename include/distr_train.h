/*
 * distr_train.h -- C ABI of libdistr.so, part 7: the LAYER-WISE decoder path -- decode_sdf with gradients to the decoder's WEIGHTS.
 * Included by distr.h. Every other decoder entry point runs the fused tiles on the packed copy of distr_set_decoder and treats the
 * weights as constants. The calls below evaluate the same DeepSDF 8x512 network (latent_in=[4], code length C in 1..508, eval mode)
 * one layer at a time: every layer is one f32-MFMA GEMM over the whole point list, the layer inputs stay in the workspace (16 KB per
 * row), and the backward returns g_W / g_b of all nine layers and the code gradient. The weights are the caller's own arrays, plain
 * row-major (out, in) as torch keeps them: nothing is packed, the context's decoder (if any) is not involved.
 *
 * Point list. Segments as in distr_multi.h: nseg (1..DISTR_MAX_VIEWS), counts_host[s] >= 0 points (HOST array, at most 2^30 in all), the
 * code of segment s at latent_dev + s * latent_stride (0: one shared code, else >= C). In the workspace every segment is padded to a
 * multiple of 64 ROWS: segment s starts at row distr_train_segment_row(nseg, counts_host, s), point i of it is row + i. A padded row
 * has xyz = 0 and an upstream gradient of 0; it adds exactly nothing to any sum.
 *
 * Saved activations. X_l (l = 1..8) is the input of lin_l = relu of lin_(l-1)'s output, point-major f32 rows of 512 floats each,
 * at byte offset distr_train_activation_offset(latent_size, nseg, counts_host, l) from the workspace pointer rounded up to 256 bytes.
 * X_4 holds the 509 - C outputs of lin3 in its first columns (the rest of the row is not written); lin4's remaining inputs are the code
 * (folded into a per-segment constant) and xyz.
 *
 * What is identical to what. Sums run in fixed orders (k in natural order inside a GEMM; a weight gradient's row dimension in at most
 * 64 slabs whose length depends on the row count only -- distr_train_slab_plan -- added in slab order; column sums per 64-row block,
 * per segment, then over segments in order): no float atomics, the same bytes on every run and every machine. A segment's sdf slice
 * and its g_latent row are byte for byte those of a call on that segment alone. f32 arithmetic only.
 *
 * Conventions of distr.h: struct_size first (DISTR_INIT), everything enqueued on the caller's stream, no allocation, no host
 * synchronisation. Refused: what distr_multi.h refuses, a latent_size outside 1..508, a null weight / gradient pointer
 * (DISTR_ERR_INVALID_ARG), a workspace that is too small (DISTR_ERR_WORKSPACE). distr_train_workspace_bytes,
 * distr_train_activation_offset return 0 and distr_train_segment_row returns -1 for arguments the calls refuse.
 */
#ifndef DISTR_TRAIN_H_
#define DISTR_TRAIN_H_

#include "distr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DISTR_TRAIN_MAX_SLABS 64

/* the nine layers, device pointers: W[l] row-major (out_l, in_l), b[l] (out_l); shapes of DeepSDF 8x512 with latent_in=[4]:
 * lin0 (512, C + 3), lin3 (509 - C, 512), lin8 (1, 512), the others (512, 512) */
typedef struct distr_train_weights {
  uint32_t struct_size;
  int32_t latent_size; /* C */
  const float* W[9];
  const float* b[9];
} distr_train_weights;

/* where the backward writes (overwrites, does not add): g_W[l] and g_b[l] in the shapes of W[l] and b[l], all eighteen required */
typedef struct distr_train_grads {
  uint32_t struct_size;
  uint32_t reserved;
  float* g_W[9];
  float* g_b[9];
} distr_train_grads;

/* one workspace serves the forward and its backward */
size_t distr_train_workspace_bytes(int32_t latent_size, int32_t nseg, const int64_t* counts_host);
/* byte offset of X_layer (layer 1..8) behind the 256-byte aligned workspace base; rows of 512 floats */
size_t distr_train_activation_offset(int32_t latent_size, int32_t nseg, const int64_t* counts_host, int32_t layer);
/* first workspace row of segment seg (0..nseg; nseg: the number of rows in all) */
int64_t distr_train_segment_row(int32_t nseg, const int64_t* counts_host, int32_t seg);
/* K slabs of a weight-gradient GEMM over `rows` rows: a function of the row count alone; at most DISTR_TRAIN_MAX_SLABS slabs */
void distr_train_slab_plan(int64_t rows, int64_t* slab_len, int32_t* num_slabs);

/* sdf_dev[sum counts] in the caller's point order; clamp_dist < 0 = no clamp. Fills the workspace for distr_train_backward. */
int distr_train_forward(distr_ctx* ctx, const distr_train_weights* weights, int32_t nseg, const int64_t* counts_host,
                        const float* latent_dev, int64_t latent_stride, const float* xyz_dev, float clamp_dist, float* sdf_dev,
                        void* ws_dev, size_t ws_bytes, void* stream);
/* backward of distr_train_forward with the SAME weights, list, codes and clamp, on the workspace it filled: g_sdf[sum counts] ->
 * grads, g_latent[nseg][C] (may be NULL; a row per segment, also for a shared code: the caller adds the rows up) */
int distr_train_backward(distr_ctx* ctx, const distr_train_weights* weights, int32_t nseg, const int64_t* counts_host,
                         const float* latent_dev, int64_t latent_stride, const float* g_sdf, float clamp, void* ws_dev,
                         const distr_train_grads* grads, float* g_latent, void* stream);

/* ---- dropout in training mode. The mask is a pure function, no generator state and no stored mask:
 *   keep(seed, l, g, i, n) = out[i & 3] >= threshold
 *   out = philox4x32_10(counter = (i >> 2, g, n, l), key = (seed & 0xffffffff, seed >> 32))
 * l = 0..7: the layer whose relu output is dropped (lin_l); n: its output unit; g = segment_base + s: the segment's global index
 * (its low 32 bits); i: the point's index inside its segment. threshold = min(2^32 - 1, floor(p * 2^32)) and scale = float(1 / (1 - p))
 * are the caller's (computed in double). A kept value is multiplied by scale, a dropped one is stored as +0: the saved X_(l+1) is the
 * activation behind the dropout. The mask does not depend on the padding, on how a list is cut into calls, or on the machine.
 * drop == NULL or layer_mask == 0: exactly the calls above. The backward takes the struct of its forward. Refused
 * (DISTR_ERR_INVALID_ARG): a wrong struct_size, layer_mask above 0xff, a scale that is not finite or below 1, segment_base < 0 or
 * segment_base + nseg > 2^32. */
typedef struct distr_train_dropout {
  uint32_t struct_size;
  uint32_t layer_mask;      /* bit l: drop lin_l's output, l = 0..7 */
  uint32_t threshold;       /* T */
  float    scale;
  uint64_t seed;
  int64_t  segment_base;    /* global index of segment 0 of this call */
} distr_train_dropout;

int distr_train_forward_dropout(distr_ctx* ctx, const distr_train_weights* weights, int32_t nseg, const int64_t* counts_host,
                                const float* latent_dev, int64_t latent_stride, const float* xyz_dev, float clamp_dist, float* sdf_dev,
                                void* ws_dev, size_t ws_bytes, void* stream, const distr_train_dropout* drop);
int distr_train_backward_dropout(distr_ctx* ctx, const distr_train_weights* weights, int32_t nseg, const int64_t* counts_host,
                                 const float* latent_dev, int64_t latent_stride, const float* g_sdf, float clamp, void* ws_dev,
                                 const distr_train_grads* grads, float* g_latent, void* stream, const distr_train_dropout* drop);
/* host code, no GPU: the definition above (1 = kept), for tests and callers */
int distr_train_dropout_keep(uint64_t seed, uint32_t threshold, int32_t layer, int64_t segment, int64_t point, int32_t unit);

/* ---- the same path for a network that is DESCRIBED instead of derived from C: the colour decoder.
 * The 8x512 chain with latent_in=[4] and
 *   lin0 (512, L + 3)                       columns [code (L) | xyz (3)]
 *   lin3 (lin3_rows, 512)
 *   lin4 (512, ld4 = lin3_rows + L + 3)     columns [lin3's outputs (lin3_rows) | code (L) | xyz (3)]
 *   lin8 (out_dim, 512)                     followed by tanh
 * The SDF decoder is L = C, lin3_rows = 509 - C, out_dim = 1 (ld4 = 512): the calls above are exactly these calls on that description.
 * The colour decoder of load_decoder(color_size=cs) is L = 256 + cs, lin3_rows = 253, out_dim = 3; its code rows are [shape | colour].
 * out[sum counts][out_dim] and g_out[sum counts][out_dim] in the caller's point order, g_latent[nseg][L]; distr_train_grads in the
 * shapes the description implies. clamp_dist is honoured for out_dim == 1 and must be negative for out_dim == 3. X_4 holds lin3_rows
 * columns. For out_dim == 1 the workspace is carved as above (the size and the offsets do not depend on L or lin3_rows); for out_dim ==
 * 3 the three per-row arrays behind X_8 have three floats per row. Sum orders, padding, segments, latent_dev / latent_stride (0 or >=
 * L), streams and the dropout struct (may be NULL) as above. Refused (DISTR_ERR_INVALID_ARG): a wrong struct_size, out_dim other than
 * 1 or 3, lin3_rows outside 1..509, L outside 1..65536, a null pointer, a clamp_dist >= 0 with out_dim == 3; DISTR_ERR_WORKSPACE for
 * a workspace that is too small. The two size functions return 0 for a description the calls refuse (pointers are not looked at). */
typedef struct distr_train_net {
  uint32_t struct_size;
  int32_t  latent_size;   /* L: code length folded into c0 / c4 (SDF: C; colour: 256 + cs) */
  int32_t  lin3_rows;     /* outputs of lin3 = activation columns of lin4 (SDF: 509 - C; colour: 253) */
  int32_t  out_dim;       /* rows of lin8: 1 or 3 */
  const float* W[9];
  const float* b[9];
} distr_train_net;

size_t distr_train_net_workspace_bytes(const distr_train_net* net, int32_t nseg, const int64_t* counts_host);
size_t distr_train_net_activation_offset(const distr_train_net* net, int32_t nseg, const int64_t* counts_host, int32_t layer);
int distr_train_net_forward(distr_ctx* ctx, const distr_train_net* net, int32_t nseg, const int64_t* counts_host, const float* latent_dev,
                            int64_t latent_stride, const float* xyz_dev, float clamp_dist, float* out_dev, void* ws_dev, size_t ws_bytes,
                            void* stream, const distr_train_dropout* drop);
int distr_train_net_backward(distr_ctx* ctx, const distr_train_net* net, int32_t nseg, const int64_t* counts_host, const float* latent_dev,
                             int64_t latent_stride, const float* g_out, float clamp_dist, void* ws_dev, const distr_train_grads* grads,
                             float* g_latent, void* stream, const distr_train_dropout* drop);

/* ---- the SPATIAL GRADIENT g = grad_x f of an out_dim == 1 net, with gradients to the weights and the codes:
 * what a normal or an Eikonal term is made of. The forward returns f = tanh(z) WITHOUT a clamp (sdf_dev[sum counts]) and the true
 * gradient g (grad_dev[sum counts][3]; not decode_sdf_gradient's 3 x, no clamp mask), in the caller's point order. The backward takes the
 * upstreams g_sdf = dL/df [sum counts] and g_grad = dL/dg [sum counts][3] (either may be NULL = zero) and makes ONE pass for both:
 * grads and g_latent as distr_train_net_backward. With g_grad == NULL the result is the gradient of distr_train_net_forward without a
 * clamp (another sum order: the row scalar is applied to the operands, not to the delta). The ReLU's second derivative is taken as
 * zero. Weights, list, codes, streams, padding and the dropout struct (the tangent and the deltas see the forward's mask and scale) as
 * above; the backward runs on the workspace its forward filled and may be repeated. Workspace: the carve of
 * distr_train_net_workspace_bytes, unchanged, and behind it eight tangent rows of 512 floats, the padded upstream and the row scalars:
 * 40 KB + 44 bytes per padded row against 24 KB. Sum orders: those of the calls above; g itself is one fmaf chain per component, the
 * hidden units in natural order, lin0's 512 then lin4's 512. Same bytes on every run; a segment's sdf / grad slices and its g_latent
 * row are those of a call on that segment alone. Refused as above, and out_dim != 1 (DISTR_ERR_INVALID_ARG: the colour net has no such
 * gradient); distr_train_grad_workspace_bytes returns 0 for what the calls refuse. */
size_t distr_train_grad_workspace_bytes(const distr_train_net* net, int32_t nseg, const int64_t* counts_host);
int distr_train_grad_forward(distr_ctx* ctx, const distr_train_net* net, int32_t nseg, const int64_t* counts_host, const float* latent_dev,
                             int64_t latent_stride, const float* xyz_dev, float* sdf_dev, float* grad_dev, void* ws_dev, size_t ws_bytes,
                             void* stream, const distr_train_dropout* drop);
int distr_train_grad_backward(distr_ctx* ctx, const distr_train_net* net, int32_t nseg, const int64_t* counts_host, const float* latent_dev,
                              int64_t latent_stride, const float* g_sdf, const float* g_grad, void* ws_dev, const distr_train_grads* grads,
                              float* g_latent, void* stream, const distr_train_dropout* drop);

#ifdef __cplusplus
}
#endif
#endif /* DISTR_TRAIN_H_ */
