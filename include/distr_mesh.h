/*
 * distr_mesh.h -- C ABI of libdistr.so, part 2: shape evaluation (marching cubes, surface sampling, nearest-point distances for the
 * chamfer distance). Included by distr.h; the reference's counterpart is core/evaluation/ (create_mesh.py's marching cubes through
 * scikit-image, transforms.py's trimesh sampling, eval_func.py's scipy KD-tree chamfer). At the end, without a counterpart there:
 * signed distances to a triangle mesh and DeepSDF-style query points, the SDF samples a decoder is trained on; and depth, normal and
 * mask maps of a triangle mesh in the renderer's camera convention (distr_mesh_render), the observations the image losses and
 * distr_samples.h consume -- the reference loads them from files its Blender pipeline (synthesis/) wrote.
 *
 * Same conventions as distr.h: caller-owned device buffers and workspaces, everything enqueued on `stream`, DISTR_OK or a negative
 * code with text in distr_last_error. These need a context (its device) but no decoder. Only distr_mc_count synchronises the stream:
 * it returns the sizes of the mesh so that the caller can allocate it.
 *
 * Grids are dense float32 (nx, ny, nz), x slowest: value (i, j, k) at grid_dev[(i * ny + j) * nz + k]. Refused (DISTR_ERR_INVALID_ARG):
 * fewer than 2 values along an axis, 2^31 values or more. Determinism: every output is the same byte for byte on every run.
 */
#ifndef DISTR_MESH_H_
#define DISTR_MESH_H_

#include "distr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Marching cubes at `level` (inside = value < level, strict). Bytes of the workspace for distr_mc_count + distr_mc_emit of a grid
 * (0 for a grid they refuse). */
size_t distr_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
/* Classifies every cell and scans the counts; returns the number of vertices (one per sign-changing grid edge, shared by the cells
 * around it) and triangles. Synchronises `stream`. DISTR_ERR_UNSUPPORTED when either count exceeds INT32_MAX. The workspace then
 * holds what distr_mc_emit needs: pass it on untouched, with the same grid and level. */
int distr_mc_count(distr_ctx* ctx, const float* grid_dev, int32_t nx, int32_t ny, int32_t nz, float level, int64_t* nverts,
                   int64_t* nfaces, void* ws_dev, size_t ws_bytes, void* stream);
/* Writes verts_dev[nverts][3] and faces_dev[nfaces][3] (int32 indices into verts_dev; nverts / nfaces = what distr_mc_count returned:
 * nothing is written beyond them). Vertex on the edge from grid point p0 to p1 along axis d: t = a0 / (a0 - a1) with a = value - level,
 * coordinate d = origin[d] + voxel_size[d] * (index_d + t), the others origin + voxel_size * index (float32, in that order).
 * Vertices are ordered by (owning grid point = the edge's lower end, axis x < y < z), triangles by (cell = its lowest corner, table
 * order). Triangles wind counter-clockwise seen from the side of larger values (right-hand normals point towards increasing values).
 * origin / voxel_size: HOST arrays of 3. */
int distr_mc_emit(distr_ctx* ctx, const float* grid_dev, int32_t nx, int32_t ny, int32_t nz, float level, const float* origin,
                  const float* voxel_size, float* verts_dev, int64_t nverts, int32_t* faces_dev, int64_t nfaces, void* ws_dev,
                  size_t ws_bytes, void* stream);

/* Area-weighted surface sampling (trimesh.sample.sample_surface): n points on the triangles faces_dev[nfaces][3] of
 * verts_dev[nverts][3]. Per sample, three counter-based random numbers of (seed, sample index, k): the face is the first whose
 * cumulative float64 area exceeds u0 * total area, the point a + u1 (b - a) + u2 (c - a) with (u1, u2) folded into the triangle
 * (u -> 1 - u when u1 + u2 > 1). Writes points_dev[n][3] and face_index_dev[n]. A face that names a vertex outside [0, nverts) has
 * area 0 (a point that lands on one anyway -- all areas 0 -- is NaN). */
size_t distr_sample_workspace_bytes(int64_t nfaces);
int distr_sample_surface(distr_ctx* ctx, const float* verts_dev, int64_t nverts, const int32_t* faces_dev, int64_t nfaces, int64_t n,
                         uint64_t seed, float* points_dev, int32_t* face_index_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* d2_dev[i] = min over j of |a_i - b_j|^2 (brute force, float32 (dx*dx + dy*dy) + dz*dz on coordinate differences) for a_dev[na][3],
 * b_dev[nb][3] (nb >= 1). sums_dev (may be NULL): double[2] = { sum_i d2_i, sum_i sqrt(d2_i) } accumulated in float64 in a fixed
 * order -- the two means of one chamfer direction. */
size_t distr_nearest_workspace_bytes(int64_t na);
int distr_nearest_sqdist(distr_ctx* ctx, const float* a_dev, int64_t na, const float* b_dev, int64_t nb, float* d2_dev,
                         double* sums_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* Signed distance of q_dev[nq][3] to the triangles faces_dev[nfaces][3] of verts_dev[nverts][3], brute force over all pairs:
 * sdf_dev[i] = (|w_i| > 0.5 ? -1 : +1) * sqrtf(d2_i), d2_i = the smallest float32 squared distance to the closest point of a triangle
 * (Ericson's seven regions; the operation order is spelled out in csrc/distr_mesh.hpp), w_i = the generalised winding number (sum of
 * the triangles' signed solid angles / 4 pi: +1 inside a closed mesh whose normals point outwards, as distr_mc_emit winds them, 0
 * outside; |w| so that an inward-wound mesh gives the same signs). Optional outputs (NULL: not written): d2_dev[nq], winding_dev[nq]
 * (float32), face_dev[nq] = the nearest triangle, the lowest index among equal distances.
 * A triangle is skipped -- no distance, no solid angle -- when it names a vertex outside [0, nverts), has a coordinate that is not
 * finite, or its float32 cross product (b - a) x (c - a) is exactly zero. No triangle left: sdf = +inf, face = -1. A query with a
 * coordinate that is not finite: sdf = d2 = winding = NaN, face = -1. nfaces < 1: DISTR_ERR_INVALID_ARG.
 * The row of a query does not depend on the other queries of the call: triangles are summed in chunks of a fixed 1024. */
size_t distr_mesh_sdf_workspace_bytes(int64_t nq, int64_t nfaces);
int distr_mesh_sdf(distr_ctx* ctx, const float* verts_dev, int64_t nverts, const int32_t* faces_dev, int64_t nfaces, const float* q_dev,
                   int64_t nq, float* sdf_dev, float* d2_dev, float* winding_dev, int32_t* face_dev, void* ws_dev, size_t ws_bytes,
                   void* stream);
/* DeepSDF-style query points from ns surface points surf_dev[ns][3] (distr_sample_surface): q_out_dev[2 * ns + n_uniform][3], rows
 * 2 i and 2 i + 1 = surface point i plus sigma_a resp. sigma_b times three standard normals each (Box-Muller), rows 2 * ns + j uniform
 * in [-half_extent, half_extent)^3. Counter-based like the sampler (slot k = 3 of its generator, which the sampler never draws):
 * every row is a function of (seed, its index) alone. */
int distr_sdf_queries(distr_ctx* ctx, const float* surf_dev, int64_t ns, float sigma_a, float sigma_b, int64_t n_uniform,
                      float half_extent, uint64_t seed, float* q_out_dev, void* stream);

/* Depth, normal and mask maps of a triangle mesh seen by nviews (1..DISTR_MAX_VIEWS) pinhole cameras of one image size, in the
 * renderer's camera convention: RT_dev[v] (3, 4) row-major = [R | T], pixel centres at the integer (x, y), camera position
 * c = -R^T T and ray d exactly as the march forms them, both moved to the mesh's frame with M^T. Brute force over all (ray, triangle)
 * pairs, float32 throughout; the operation order is spelled out in csrc/distr_mesh.hpp (k_mesh_cast), a numpy float32 restatement
 * gives the same bits. Not differentiable: the maps are observations.
 *   Per triangle and view, with the corners relative to the camera (A, B, C): Na = C x B, Nb = A x C, Nc = B x A; per ray e the edge
 *   functions U = e.Na, V = e.Nb, W = e.Nc. A hit: the signs of U, V, W are not mixed (zeros inclusive), det = (U + V) + W != 0,
 *   t = (A.Ng) / (e.Ng) finite and > 0 with Ng = (B - A) x (C - A). The edge functions of an edge shared by two triangles of an indexed
 *   mesh are exact negatives of each other: no ray passes between them. The nearest hit wins, the lowest face among equal t.
 * Outputs, [nviews][H*W] each, any of them may be NULL:
 *   zdepth_dev  t                          depth_dev  t * calib (what render returns for a valid pixel); a miss: 1e11 in both
 *   normal_dev  [..][3] the geometric normal +-Ng / |Ng| oriented towards the camera whatever the winding;
 *               DISTR_MESH_NORMAL_WORLD: M n (what distr_depth_samples_forward expects: it multiplies by M^T itself),
 *               DISTR_MESH_NORMAL_IMAGE: R (M n) with its x component negated (render's autograd normals); a miss: 0
 *   mask_dev    uint8, 1 for a hit         face_dev   int32, the triangle hit, -1 for a miss
 *   bary_dev    [..][2] = (V / det, W / det), the weights of corners b and c; a miss: 0
 * Triangles are skipped by the rule of distr_mesh_sdf (a vertex outside [0, nverts), a coordinate that is not finite, a float32 cross
 * product (b - a) x (c - a) of exactly zero); a view whose RT holds a number that is not finite gives all misses.
 * Determinism: the per-pixel minimum meets in an integer atomic min on (bits(t) << 32) | face; no float atomic. The same bytes on every
 * run, and a view's maps do not depend on the other views of the call.
 * Refused (DISTR_ERR_INVALID_ARG): nfaces < 1, more than 65535 * 1024 triangles, H * W * nviews >= 2^31, a wrong struct_size. */
#define DISTR_MESH_NORMAL_WORLD 0
#define DISTR_MESH_NORMAL_IMAGE 1

typedef struct distr_mesh_render_cfg {
  uint32_t struct_size; /* sizeof(distr_mesh_render_cfg): DISTR_INIT */
  int32_t H, W;         /* img_hw */
  float K_inv[9];       /* float32(inv(K)), row-major */
  float M[9];           /* transform_matrix (3x3): mesh frame -> world, x_world = M x_mesh */
  int32_t normal_frame; /* DISTR_MESH_NORMAL_* */
} distr_mesh_render_cfg;

size_t distr_mesh_render_workspace_bytes(int32_t H, int32_t W, int32_t nviews);
int distr_mesh_render(distr_ctx* ctx, const distr_mesh_render_cfg* cfg, const float* verts_dev, int64_t nverts, const int32_t* faces_dev,
                      int64_t nfaces, int32_t nviews, const float* RT_dev, float* depth_dev, float* zdepth_dev, float* normal_dev,
                      uint8_t* mask_dev, int32_t* face_dev, float* bary_dev, void* ws_dev, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DISTR_MESH_H_ */
