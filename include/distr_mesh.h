/*
 * distr_mesh.h -- C ABI of libdistr.so, part 2: shape evaluation (marching cubes, surface sampling, nearest-point distances for the
 * chamfer distance). Included by distr.h; the reference's counterpart is core/evaluation/ (create_mesh.py's marching cubes through
 * scikit-image, transforms.py's trimesh sampling, eval_func.py's scipy KD-tree chamfer).
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

#ifdef __cplusplus
}
#endif
#endif /* DISTR_MESH_H_ */
