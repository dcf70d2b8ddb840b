// distr_mesh.hpp -- shape evaluation after the render path (reference: core/evaluation/create_mesh.py, transforms.py, eval_func.py):
//
//   marching cubes     over a dense f32 grid (nx, ny, nz), x slowest (the layout create_sdf_grid returns)
//   surface sampling   area-weighted, trimesh.sample.sample_surface's rule (searchsorted on the cumulative area, folded parallelogram)
//   nearest distance   brute force squared distance from every point of A to the nearest of B (one chamfer direction)
// and the way back from a mesh to training data (no counterpart in the reference, which loads preprocessed files; at the end of the file):
//   signed distance    brute force exact point-to-triangle distance, signed by the generalised winding number
//   query points       DeepSDF-style: surface samples perturbed at two scales plus uniform points, from the sampler's generator
// and from a mesh to images (the reference loads them from a Blender pipeline's files; at the very end):
//   depth / normal / mask maps   brute force ray-triangle intersection in the renderer's camera convention, watertight in float32
//
// No MFMA: scans and VALU loops. Every output position comes from an exclusive scan in a fixed order (per-thread serial run of
// MTILE / MB items -> LDS scan over the block -> one ordered pass over the block totals), never from an atomic, so every output is
// the same byte for byte from run to run. The only atomic (nearest distance) is a min, whose result does not depend on order.
//
// Marching cubes, in four launches (distr_mc_count: 1-2, distr_mc_emit: 3-4):
//   1 k_mc_classify  per grid point p = (i*ny + j)*nz + k: the cube index of the cell whose minimum corner p is (inside = v < level,
//                    strict), its triangle count from kMcTri, and the sign-changing x / y / z edges p OWNS (those leaving p towards
//                    +x, +y, +z); block totals of (active points, vertices, faces)
//   2 k_mc_top_scan  exclusive scan of the block totals (int64), grand totals behind them: what distr_mc_count reads back
//   3 k_mc_compact   block-local scan again: active points (an owned crossing or a cell with triangles) into a list in point order,
//                    each point's first vertex index (vbase), each active point's first face index; the point's vertices are written
//                    here: t = a0 / (a0 - a1), a = v - level, coord = origin + voxel_size * (index + t) along the edge axis
//   4 k_mc_faces     one thread per active point: the cell's triangles from kMcTri, every corner an owned-edge vertex of the cell's
//                    own corner point or of a neighbour (vbase[q] + rank of the axis among q's owned crossings): vertices are shared
// Order: vertices by (owning point, axis x < y < z), faces by (cell = its minimum corner point, table order).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "distr_kernels.hpp"    // DISTR_GLOBAL (distr_mlp.hpp), make_ray

namespace distr {
namespace mesh {

constexpr int MB = 256;           // threads per block
constexpr int MPER = 8;           // consecutive items per thread
constexpr int MTILE = MB * MPER;  // items per block

// Triangle table: 256 cube indices (bit c set when corner c is inside, v < level) x up to 5 triangles of cube-edge numbers, -1 ends.
// Corners (x, y, z): 0 (0,0,0) 1 (1,0,0) 2 (1,1,0) 3 (0,1,0) 4 (0,0,1) 5 (1,0,1) 6 (1,1,1) 7 (0,1,1); edges 0: 0-1, 1: 1-2, 2: 2-3,
// 3: 3-0, 4: 4-5, 5: 5-6, 6: 6-7, 7: 7-4, 8: 0-4, 9: 1-5, 10: 2-6, 11: 3-7 (the public-domain layout of Bourke's table). Each row is
// the boundary of the inside region on the cube's faces, closed into loops and fanned from the loop's lowest edge: on a face whose
// four corners alternate, the two INSIDE corners are cut off separately -- a decision taken from that face's corners alone, so the
// two cells that share the face agree and a closed level set gives a closed mesh (not Lewiner's asymptotic decider).
// Winding: counter-clockwise seen from the outside (v >= level), so right-hand normals point towards increasing values.
__constant__ signed char kMcTri[256][16] = {
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 8, 9, 1, 3, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 1, 10, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 10, 2, 0, 9, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 9, 10, 2, 8, 9, 2, 3, 8, -1, -1, -1, -1, -1, -1, -1},
    {2, 11, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 11, 8, 0, 2, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 2, 11, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 8, 9, 1, 11, 8, 1, 2, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 11, 3, 1, 10, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 11, 8, 0, 10, 11, 0, 1, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 11, 3, 0, 10, 11, 0, 9, 10, -1, -1, -1, -1, -1, -1, -1},
    {8, 10, 11, 8, 9, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 8, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 7, 4, 0, 3, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 4, 9, 1, 7, 4, 1, 3, 7, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 2, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 7, 4, 0, 3, 7, 1, 10, 2, -1, -1, -1, -1, -1, -1, -1},
    {0, 10, 2, 0, 9, 10, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1},
    {2, 9, 10, 2, 4, 9, 2, 7, 4, 2, 3, 7, -1, -1, -1, -1},
    {2, 11, 3, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 7, 4, 0, 11, 7, 0, 2, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 2, 11, 3, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1},
    {1, 4, 9, 1, 7, 4, 1, 11, 7, 1, 2, 11, -1, -1, -1, -1},
    {1, 11, 3, 1, 10, 11, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1},
    {0, 7, 4, 0, 11, 7, 0, 10, 11, 0, 1, 10, -1, -1, -1, -1},
    {0, 11, 3, 0, 10, 11, 0, 9, 10, 4, 8, 7, -1, -1, -1, -1},
    {4, 11, 7, 4, 10, 11, 4, 9, 10, -1, -1, -1, -1, -1, -1, -1},
    {4, 5, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 4, 5, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 5, 1, 0, 4, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 4, 5, 1, 8, 4, 1, 3, 8, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 2, 4, 5, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 1, 10, 2, 4, 5, 9, -1, -1, -1, -1, -1, -1, -1},
    {0, 10, 2, 0, 5, 10, 0, 4, 5, -1, -1, -1, -1, -1, -1, -1},
    {2, 5, 10, 2, 4, 5, 2, 8, 4, 2, 3, 8, -1, -1, -1, -1},
    {2, 11, 3, 4, 5, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 11, 8, 0, 2, 11, 4, 5, 9, -1, -1, -1, -1, -1, -1, -1},
    {0, 5, 1, 0, 4, 5, 2, 11, 3, -1, -1, -1, -1, -1, -1, -1},
    {1, 4, 5, 1, 8, 4, 1, 11, 8, 1, 2, 11, -1, -1, -1, -1},
    {1, 11, 3, 1, 10, 11, 4, 5, 9, -1, -1, -1, -1, -1, -1, -1},
    {0, 11, 8, 0, 10, 11, 0, 1, 10, 4, 5, 9, -1, -1, -1, -1},
    {0, 11, 3, 0, 10, 11, 0, 5, 10, 0, 4, 5, -1, -1, -1, -1},
    {4, 11, 8, 4, 10, 11, 4, 5, 10, -1, -1, -1, -1, -1, -1, -1},
    {5, 8, 7, 5, 9, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 5, 9, 0, 7, 5, 0, 3, 7, -1, -1, -1, -1, -1, -1, -1},
    {0, 5, 1, 0, 7, 5, 0, 8, 7, -1, -1, -1, -1, -1, -1, -1},
    {1, 7, 5, 1, 3, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 2, 5, 8, 7, 5, 9, 8, -1, -1, -1, -1, -1, -1, -1},
    {0, 5, 9, 0, 7, 5, 0, 3, 7, 1, 10, 2, -1, -1, -1, -1},
    {0, 10, 2, 0, 5, 10, 0, 7, 5, 0, 8, 7, -1, -1, -1, -1},
    {2, 5, 10, 2, 7, 5, 2, 3, 7, -1, -1, -1, -1, -1, -1, -1},
    {2, 11, 3, 5, 8, 7, 5, 9, 8, -1, -1, -1, -1, -1, -1, -1},
    {0, 5, 9, 0, 7, 5, 0, 11, 7, 0, 2, 11, -1, -1, -1, -1},
    {0, 5, 1, 0, 7, 5, 0, 8, 7, 2, 11, 3, -1, -1, -1, -1},
    {1, 7, 5, 1, 11, 7, 1, 2, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 11, 3, 1, 10, 11, 5, 8, 7, 5, 9, 8, -1, -1, -1, -1},
    {0, 5, 9, 0, 7, 5, 0, 11, 7, 0, 10, 11, 0, 1, 10, -1},
    {0, 11, 3, 0, 10, 11, 0, 5, 10, 0, 7, 5, 0, 8, 7, -1},
    {5, 11, 7, 5, 10, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {5, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 8, 9, 1, 3, 8, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {1, 6, 2, 1, 5, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 1, 6, 2, 1, 5, 6, -1, -1, -1, -1, -1, -1, -1},
    {0, 6, 2, 0, 5, 6, 0, 9, 5, -1, -1, -1, -1, -1, -1, -1},
    {2, 5, 6, 2, 9, 5, 2, 8, 9, 2, 3, 8, -1, -1, -1, -1},
    {2, 11, 3, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 11, 8, 0, 2, 11, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 2, 11, 3, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {1, 8, 9, 1, 11, 8, 1, 2, 11, 5, 6, 10, -1, -1, -1, -1},
    {1, 11, 3, 1, 6, 11, 1, 5, 6, -1, -1, -1, -1, -1, -1, -1},
    {0, 11, 8, 0, 6, 11, 0, 5, 6, 0, 1, 5, -1, -1, -1, -1},
    {0, 11, 3, 0, 6, 11, 0, 5, 6, 0, 9, 5, -1, -1, -1, -1},
    {5, 8, 9, 5, 11, 8, 5, 6, 11, -1, -1, -1, -1, -1, -1, -1},
    {4, 8, 7, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 7, 4, 0, 3, 7, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 4, 8, 7, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {1, 4, 9, 1, 7, 4, 1, 3, 7, 5, 6, 10, -1, -1, -1, -1},
    {1, 6, 2, 1, 5, 6, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1},
    {0, 7, 4, 0, 3, 7, 1, 6, 2, 1, 5, 6, -1, -1, -1, -1},
    {0, 6, 2, 0, 5, 6, 0, 9, 5, 4, 8, 7, -1, -1, -1, -1},
    {2, 5, 6, 2, 9, 5, 2, 4, 9, 2, 7, 4, 2, 3, 7, -1},
    {2, 11, 3, 4, 8, 7, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 7, 4, 0, 11, 7, 0, 2, 11, 5, 6, 10, -1, -1, -1, -1},
    {0, 9, 1, 2, 11, 3, 4, 8, 7, 5, 6, 10, -1, -1, -1, -1},
    {1, 4, 9, 1, 7, 4, 1, 11, 7, 1, 2, 11, 5, 6, 10, -1},
    {1, 11, 3, 1, 6, 11, 1, 5, 6, 4, 8, 7, -1, -1, -1, -1},
    {0, 7, 4, 0, 11, 7, 0, 6, 11, 0, 5, 6, 0, 1, 5, -1},
    {0, 11, 3, 0, 6, 11, 0, 5, 6, 0, 9, 5, 4, 8, 7, -1},
    {4, 11, 7, 4, 6, 11, 4, 5, 6, 4, 9, 5, -1, -1, -1, -1},
    {4, 10, 9, 4, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 4, 10, 9, 4, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 10, 1, 0, 6, 10, 0, 4, 6, -1, -1, -1, -1, -1, -1, -1},
    {1, 6, 10, 1, 4, 6, 1, 8, 4, 1, 3, 8, -1, -1, -1, -1},
    {1, 6, 2, 1, 4, 6, 1, 9, 4, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 1, 6, 2, 1, 4, 6, 1, 9, 4, -1, -1, -1, -1},
    {0, 6, 2, 0, 4, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 4, 6, 2, 8, 4, 2, 3, 8, -1, -1, -1, -1, -1, -1, -1},
    {2, 11, 3, 4, 10, 9, 4, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 11, 8, 0, 2, 11, 4, 10, 9, 4, 6, 10, -1, -1, -1, -1},
    {0, 10, 1, 0, 6, 10, 0, 4, 6, 2, 11, 3, -1, -1, -1, -1},
    {1, 6, 10, 1, 4, 6, 1, 8, 4, 1, 11, 8, 1, 2, 11, -1},
    {1, 11, 3, 1, 6, 11, 1, 4, 6, 1, 9, 4, -1, -1, -1, -1},
    {0, 11, 8, 0, 6, 11, 0, 4, 6, 0, 9, 4, 0, 1, 9, -1},
    {0, 11, 3, 0, 6, 11, 0, 4, 6, -1, -1, -1, -1, -1, -1, -1},
    {4, 11, 8, 4, 6, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {6, 8, 7, 6, 9, 8, 6, 10, 9, -1, -1, -1, -1, -1, -1, -1},
    {0, 10, 9, 0, 6, 10, 0, 7, 6, 0, 3, 7, -1, -1, -1, -1},
    {0, 10, 1, 0, 6, 10, 0, 7, 6, 0, 8, 7, -1, -1, -1, -1},
    {1, 6, 10, 1, 7, 6, 1, 3, 7, -1, -1, -1, -1, -1, -1, -1},
    {1, 6, 2, 1, 7, 6, 1, 8, 7, 1, 9, 8, -1, -1, -1, -1},
    {0, 1, 9, 0, 2, 1, 0, 6, 2, 0, 7, 6, 0, 3, 7, -1},
    {0, 6, 2, 0, 7, 6, 0, 8, 7, -1, -1, -1, -1, -1, -1, -1},
    {2, 7, 6, 2, 3, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 11, 3, 6, 8, 7, 6, 9, 8, 6, 10, 9, -1, -1, -1, -1},
    {0, 10, 9, 0, 6, 10, 0, 7, 6, 0, 11, 7, 0, 2, 11, -1},
    {0, 10, 1, 0, 6, 10, 0, 7, 6, 0, 8, 7, 2, 11, 3, -1},
    {1, 6, 10, 1, 7, 6, 1, 11, 7, 1, 2, 11, -1, -1, -1, -1},
    {1, 11, 3, 1, 6, 11, 1, 7, 6, 1, 8, 7, 1, 9, 8, -1},
    {0, 1, 9, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 11, 3, 0, 6, 11, 0, 7, 6, 0, 8, 7, -1, -1, -1, -1},
    {6, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {6, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 8, 9, 1, 3, 8, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 2, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 1, 10, 2, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 10, 2, 0, 9, 10, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {2, 9, 10, 2, 8, 9, 2, 3, 8, 6, 7, 11, -1, -1, -1, -1},
    {2, 7, 3, 2, 6, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 7, 8, 0, 6, 7, 0, 2, 6, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 2, 7, 3, 2, 6, 7, -1, -1, -1, -1, -1, -1, -1},
    {1, 8, 9, 1, 7, 8, 1, 6, 7, 1, 2, 6, -1, -1, -1, -1},
    {1, 7, 3, 1, 6, 7, 1, 10, 6, -1, -1, -1, -1, -1, -1, -1},
    {0, 7, 8, 0, 6, 7, 0, 10, 6, 0, 1, 10, -1, -1, -1, -1},
    {0, 7, 3, 0, 6, 7, 0, 10, 6, 0, 9, 10, -1, -1, -1, -1},
    {6, 9, 10, 6, 8, 9, 6, 7, 8, -1, -1, -1, -1, -1, -1, -1},
    {4, 11, 6, 4, 8, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 6, 4, 0, 11, 6, 0, 3, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 4, 11, 6, 4, 8, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 4, 9, 1, 6, 4, 1, 11, 6, 1, 3, 11, -1, -1, -1, -1},
    {1, 10, 2, 4, 11, 6, 4, 8, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 6, 4, 0, 11, 6, 0, 3, 11, 1, 10, 2, -1, -1, -1, -1},
    {0, 10, 2, 0, 9, 10, 4, 11, 6, 4, 8, 11, -1, -1, -1, -1},
    {2, 9, 10, 2, 4, 9, 2, 6, 4, 2, 11, 6, 2, 3, 11, -1},
    {2, 8, 3, 2, 4, 8, 2, 6, 4, -1, -1, -1, -1, -1, -1, -1},
    {0, 6, 4, 0, 2, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 2, 8, 3, 2, 4, 8, 2, 6, 4, -1, -1, -1, -1},
    {1, 4, 9, 1, 6, 4, 1, 2, 6, -1, -1, -1, -1, -1, -1, -1},
    {1, 8, 3, 1, 4, 8, 1, 6, 4, 1, 10, 6, -1, -1, -1, -1},
    {0, 6, 4, 0, 10, 6, 0, 1, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 8, 3, 0, 4, 8, 0, 6, 4, 0, 10, 6, 0, 9, 10, -1},
    {4, 10, 6, 4, 9, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 5, 9, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 4, 5, 9, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 5, 1, 0, 4, 5, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 4, 5, 1, 8, 4, 1, 3, 8, 6, 7, 11, -1, -1, -1, -1},
    {1, 10, 2, 4, 5, 9, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 1, 10, 2, 4, 5, 9, 6, 7, 11, -1, -1, -1, -1},
    {0, 10, 2, 0, 5, 10, 0, 4, 5, 6, 7, 11, -1, -1, -1, -1},
    {2, 5, 10, 2, 4, 5, 2, 8, 4, 2, 3, 8, 6, 7, 11, -1},
    {2, 7, 3, 2, 6, 7, 4, 5, 9, -1, -1, -1, -1, -1, -1, -1},
    {0, 7, 8, 0, 6, 7, 0, 2, 6, 4, 5, 9, -1, -1, -1, -1},
    {0, 5, 1, 0, 4, 5, 2, 7, 3, 2, 6, 7, -1, -1, -1, -1},
    {1, 4, 5, 1, 8, 4, 1, 7, 8, 1, 6, 7, 1, 2, 6, -1},
    {1, 7, 3, 1, 6, 7, 1, 10, 6, 4, 5, 9, -1, -1, -1, -1},
    {0, 7, 8, 0, 6, 7, 0, 10, 6, 0, 1, 10, 4, 5, 9, -1},
    {0, 7, 3, 0, 6, 7, 0, 10, 6, 0, 5, 10, 0, 4, 5, -1},
    {4, 7, 8, 4, 6, 7, 4, 10, 6, 4, 5, 10, -1, -1, -1, -1},
    {5, 11, 6, 5, 8, 11, 5, 9, 8, -1, -1, -1, -1, -1, -1, -1},
    {0, 5, 9, 0, 6, 5, 0, 11, 6, 0, 3, 11, -1, -1, -1, -1},
    {0, 5, 1, 0, 6, 5, 0, 11, 6, 0, 8, 11, -1, -1, -1, -1},
    {1, 6, 5, 1, 11, 6, 1, 3, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 2, 5, 11, 6, 5, 8, 11, 5, 9, 8, -1, -1, -1, -1},
    {0, 5, 9, 0, 6, 5, 0, 11, 6, 0, 3, 11, 1, 10, 2, -1},
    {0, 10, 2, 0, 5, 10, 0, 6, 5, 0, 11, 6, 0, 8, 11, -1},
    {2, 5, 10, 2, 6, 5, 2, 11, 6, 2, 3, 11, -1, -1, -1, -1},
    {2, 8, 3, 2, 9, 8, 2, 5, 9, 2, 6, 5, -1, -1, -1, -1},
    {0, 5, 9, 0, 6, 5, 0, 2, 6, -1, -1, -1, -1, -1, -1, -1},
    {0, 5, 1, 0, 6, 5, 0, 2, 6, 0, 3, 2, 0, 8, 3, -1},
    {1, 6, 5, 1, 2, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 8, 3, 1, 9, 8, 1, 5, 9, 1, 6, 5, 1, 10, 6, -1},
    {0, 5, 9, 0, 6, 5, 0, 10, 6, 0, 1, 10, -1, -1, -1, -1},
    {0, 8, 3, 5, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {5, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {5, 11, 10, 5, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 5, 11, 10, 5, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 5, 11, 10, 5, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 8, 9, 1, 3, 8, 5, 11, 10, 5, 7, 11, -1, -1, -1, -1},
    {1, 11, 2, 1, 7, 11, 1, 5, 7, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 1, 11, 2, 1, 7, 11, 1, 5, 7, -1, -1, -1, -1},
    {0, 11, 2, 0, 7, 11, 0, 5, 7, 0, 9, 5, -1, -1, -1, -1},
    {2, 7, 11, 2, 5, 7, 2, 9, 5, 2, 8, 9, 2, 3, 8, -1},
    {2, 7, 3, 2, 5, 7, 2, 10, 5, -1, -1, -1, -1, -1, -1, -1},
    {0, 7, 8, 0, 5, 7, 0, 10, 5, 0, 2, 10, -1, -1, -1, -1},
    {0, 9, 1, 2, 7, 3, 2, 5, 7, 2, 10, 5, -1, -1, -1, -1},
    {1, 8, 9, 1, 7, 8, 1, 5, 7, 1, 10, 5, 1, 2, 10, -1},
    {1, 7, 3, 1, 5, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 7, 8, 0, 5, 7, 0, 1, 5, -1, -1, -1, -1, -1, -1, -1},
    {0, 7, 3, 0, 5, 7, 0, 9, 5, -1, -1, -1, -1, -1, -1, -1},
    {5, 8, 9, 5, 7, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 10, 5, 4, 11, 10, 4, 8, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 5, 4, 0, 10, 5, 0, 11, 10, 0, 3, 11, -1, -1, -1, -1},
    {0, 9, 1, 4, 10, 5, 4, 11, 10, 4, 8, 11, -1, -1, -1, -1},
    {1, 4, 9, 1, 5, 4, 1, 10, 5, 1, 11, 10, 1, 3, 11, -1},
    {1, 11, 2, 1, 8, 11, 1, 4, 8, 1, 5, 4, -1, -1, -1, -1},
    {0, 5, 4, 0, 1, 5, 0, 2, 1, 0, 11, 2, 0, 3, 11, -1},
    {0, 11, 2, 0, 8, 11, 0, 4, 8, 0, 5, 4, 0, 9, 5, -1},
    {2, 3, 11, 4, 9, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 8, 3, 2, 4, 8, 2, 5, 4, 2, 10, 5, -1, -1, -1, -1},
    {0, 5, 4, 0, 10, 5, 0, 2, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 2, 8, 3, 2, 4, 8, 2, 5, 4, 2, 10, 5, -1},
    {1, 4, 9, 1, 5, 4, 1, 10, 5, 1, 2, 10, -1, -1, -1, -1},
    {1, 8, 3, 1, 4, 8, 1, 5, 4, -1, -1, -1, -1, -1, -1, -1},
    {0, 5, 4, 0, 1, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 8, 3, 0, 4, 8, 0, 5, 4, 0, 9, 5, -1, -1, -1, -1},
    {4, 9, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 10, 9, 4, 11, 10, 4, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 4, 10, 9, 4, 11, 10, 4, 7, 11, -1, -1, -1, -1},
    {0, 10, 1, 0, 11, 10, 0, 7, 11, 0, 4, 7, -1, -1, -1, -1},
    {1, 11, 10, 1, 7, 11, 1, 4, 7, 1, 8, 4, 1, 3, 8, -1},
    {1, 11, 2, 1, 7, 11, 1, 4, 7, 1, 9, 4, -1, -1, -1, -1},
    {0, 3, 8, 1, 11, 2, 1, 7, 11, 1, 4, 7, 1, 9, 4, -1},
    {0, 11, 2, 0, 7, 11, 0, 4, 7, -1, -1, -1, -1, -1, -1, -1},
    {2, 7, 11, 2, 4, 7, 2, 8, 4, 2, 3, 8, -1, -1, -1, -1},
    {2, 7, 3, 2, 4, 7, 2, 9, 4, 2, 10, 9, -1, -1, -1, -1},
    {0, 7, 8, 0, 4, 7, 0, 9, 4, 0, 10, 9, 0, 2, 10, -1},
    {0, 10, 1, 0, 2, 10, 0, 3, 2, 0, 7, 3, 0, 4, 7, -1},
    {1, 2, 10, 4, 7, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 7, 3, 1, 4, 7, 1, 9, 4, -1, -1, -1, -1, -1, -1, -1},
    {0, 7, 8, 0, 4, 7, 0, 9, 4, 0, 1, 9, -1, -1, -1, -1},
    {0, 7, 3, 0, 4, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 7, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {8, 10, 9, 8, 11, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 10, 9, 0, 11, 10, 0, 3, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 10, 1, 0, 11, 10, 0, 8, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 11, 10, 1, 3, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 11, 2, 1, 8, 11, 1, 9, 8, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 9, 0, 2, 1, 0, 11, 2, 0, 3, 11, -1, -1, -1, -1},
    {0, 11, 2, 0, 8, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 3, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 8, 3, 2, 9, 8, 2, 10, 9, -1, -1, -1, -1, -1, -1, -1},
    {0, 10, 9, 0, 2, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 10, 1, 0, 2, 10, 0, 3, 2, 0, 8, 3, -1, -1, -1, -1},
    {1, 2, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 8, 3, 1, 9, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 8, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
};

// owner of cube edge e relative to the cell's minimum corner (dx, dy, dz) and its axis (0 x, 1 y, 2 z)
__constant__ unsigned char kMcEdge[12][4] = {{0, 0, 0, 0}, {1, 0, 0, 1}, {0, 1, 0, 0}, {0, 0, 0, 1}, {0, 0, 1, 0}, {1, 0, 1, 1},
                                              {0, 1, 1, 0}, {0, 0, 1, 1}, {0, 0, 0, 2}, {1, 0, 0, 2}, {1, 1, 0, 2}, {0, 1, 0, 2}};

struct McGrid {
  const float* v;
  int nx, ny, nz;
  float level;
  long long P;                     // nx * ny * nz (< 2^31)
};

struct C3 {                        // (active points, vertices, faces)
  long long a, v, f;
};
__device__ __forceinline__ C3 operator+(C3 x, C3 y) { return C3{x.a + y.a, x.v + y.v, x.f + y.f}; }

struct D2 {                        // (sum of squared distances, sum of distances)
  double s, r;
};
__device__ __forceinline__ D2 operator+(D2 x, D2 y) { return D2{x.s + y.s, x.r + y.r}; }

// Exclusive scan of one value per thread over the block (Hillis-Steele in LDS, fixed order); *total = the block's sum.
template <typename T>
__device__ T block_excl_scan(T x, T* lds, T* total) {
  const int t = threadIdx.x;
  lds[t] = x;
  __syncthreads();
  for (int off = 1; off < MB; off <<= 1) {
    T y = lds[t];
    if (t >= off) y = lds[t - off] + y;
    __syncthreads();
    lds[t] = y;
    __syncthreads();
  }
  T ex = t ? lds[t - 1] : T{};
  *total = lds[MB - 1];
  __syncthreads();
  return ex;
}

// Exclusive scan of n block totals by one block, in order: out[b] = sum of in[0..b); *total = the sum of all.
template <typename T>
DISTR_GLOBAL void __launch_bounds__(MB) k_mesh_top_scan(const T* __restrict__ in, long long n, T* __restrict__ out, T* __restrict__ total) {
  __shared__ T lds[MB];
  T carry{};
  for (long long b0 = 0; b0 < n; b0 += MB) {
    const long long b = b0 + threadIdx.x;
    T x = b < n ? in[b] : T{};
    T tot;
    T ex = block_excl_scan(x, lds, &tot);
    if (b < n) out[b] = carry + ex;
    carry = carry + tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

// info word of grid point p: bits 0-7 cube index of the cell at p (0 when p is on a maximum face), 8-10 owned crossing edges x/y/z,
// 11-13 triangles of the cell
__device__ __forceinline__ unsigned mc_info(const McGrid g, long long p) {
  const long long syz = (long long)g.ny * g.nz;
  const int i = (int)(p / syz);
  const long long r = p - i * syz;
  const int j = (int)(r / g.nz), k = (int)(r - (long long)j * g.nz);
  const float* v = g.v;
  const bool in0 = v[p] < g.level;
  unsigned em = 0;
  if (i + 1 < g.nx && ((v[p + syz] < g.level) != in0)) em |= 1;
  if (j + 1 < g.ny && ((v[p + g.nz] < g.level) != in0)) em |= 2;
  if (k + 1 < g.nz && ((v[p + 1] < g.level) != in0)) em |= 4;
  unsigned code = 0, nt = 0;
  if (i + 1 < g.nx && j + 1 < g.ny && k + 1 < g.nz) {
    const long long c[8] = {p, p + syz, p + syz + g.nz, p + g.nz, p + 1, p + syz + 1, p + syz + g.nz + 1, p + g.nz + 1};
#pragma unroll
    for (int q = 0; q < 8; ++q) code |= (v[c[q]] < g.level ? 1u : 0u) << q;
    while (nt < 5 && kMcTri[code][3 * nt] >= 0) ++nt;
  }
  return code | em << 8 | nt << 11;
}

__device__ __forceinline__ C3 mc_counts(unsigned inf) {
  return C3{(inf >> 8) ? 1 : 0, __popc((inf >> 8) & 7), (long long)(inf >> 11)};
}

DISTR_GLOBAL void __launch_bounds__(MB) k_mc_classify(const McGrid g, uint16_t* __restrict__ info, C3* __restrict__ btot) {
  __shared__ C3 lds[MB];
  const long long base = (long long)blockIdx.x * MTILE + (long long)threadIdx.x * MPER;
  C3 s{};
  for (int q = 0; q < MPER; ++q) {
    const long long p = base + q;
    if (p >= g.P) break;
    const unsigned inf = mc_info(g, p);
    info[p] = (uint16_t)inf;
    s = s + mc_counts(inf);
  }
  C3 tot;
  block_excl_scan(s, lds, &tot);
  if (threadIdx.x == 0) btot[blockIdx.x] = tot;
}

struct McOut {
  float ox, oy, oz, vx, vy, vz;    // origin, voxel size per axis
  float* verts;                    // [vcap][3]
  long long vcap;
  int* faces;                      // [fcap][3]
  long long fcap;
};

DISTR_GLOBAL void __launch_bounds__(MB) k_mc_compact(const McGrid g, const uint16_t* __restrict__ info, const C3* __restrict__ boff,
                                                     int* __restrict__ act, int* __restrict__ afb, int* __restrict__ vbase, const McOut o) {
  __shared__ C3 lds[MB];
  const long long base = (long long)blockIdx.x * MTILE + (long long)threadIdx.x * MPER;
  C3 s{};
  for (int q = 0; q < MPER; ++q) {
    const long long p = base + q;
    if (p >= g.P) break;
    s = s + mc_counts(info[p]);
  }
  C3 tot;
  C3 at = boff[blockIdx.x] + block_excl_scan(s, lds, &tot);
  const long long syz = (long long)g.ny * g.nz;
  for (int q = 0; q < MPER; ++q) {
    const long long p = base + q;
    if (p >= g.P) break;
    const unsigned inf = info[p];
    if (!(inf >> 8)) continue;
    act[at.a] = (int)p;
    afb[at.a] = (int)at.f;
    vbase[p] = (int)at.v;
    const int i = (int)(p / syz);
    const long long r = p - i * syz;
    const int j = (int)(r / g.nz), k = (int)(r - (long long)j * g.nz);
    const float a0 = g.v[p] - g.level;
    const long long step[3] = {syz, (long long)g.nz, 1};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      if (!((inf >> (8 + ax)) & 1)) continue;
      const float a1 = g.v[p + step[ax]] - g.level;
      const float t = a0 / (a0 - a1);
      if (at.v < o.vcap) {
        float* d = o.verts + 3 * at.v;
        d[0] = o.ox + o.vx * ((float)i + (ax == 0 ? t : 0.f));
        d[1] = o.oy + o.vy * ((float)j + (ax == 1 ? t : 0.f));
        d[2] = o.oz + o.vz * ((float)k + (ax == 2 ? t : 0.f));
      }
      ++at.v;
    }
    ++at.a;
    at.f += inf >> 11;
  }
}

// grid-stride over the active list; its length is on the device (the grand total of k_mesh_top_scan)
DISTR_GLOBAL void __launch_bounds__(MB) k_mc_faces(const McGrid g, const uint16_t* __restrict__ info, const int* __restrict__ act,
                                                   const int* __restrict__ afb, const int* __restrict__ vbase, const C3* __restrict__ totals,
                                                   const McOut o) {
  const long long M = totals->a;
  const long long syz = (long long)g.ny * g.nz;
  for (long long m = (long long)blockIdx.x * MB + threadIdx.x; m < M; m += (long long)gridDim.x * MB) {
    const long long p = act[m];
    const unsigned inf = info[p];
    const int code = inf & 255, nt = inf >> 11;
    const long long fb = afb[m];
    for (int t = 0; t < nt; ++t) {
      if (fb + t >= o.fcap) break;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int e = kMcTri[code][3 * t + c];
        const long long q = p + kMcEdge[e][0] * syz + kMcEdge[e][1] * (long long)g.nz + kMcEdge[e][2];
        const int ax = kMcEdge[e][3];
        const unsigned em = (info[q] >> 8) & 7;
        o.faces[3 * (fb + t) + c] = vbase[q] + __popc(em & ((1u << ax) - 1u));
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ surface sampling
struct SurfMesh {
  const float* verts;              // [nv][3]
  long long nv;
  const int* faces;                // [nf][3]
  long long nf;
};

__device__ __forceinline__ bool face_ok(const SurfMesh m, long long f) {
  const int* fi = m.faces + 3 * f;
  return fi[0] >= 0 && fi[0] < m.nv && fi[1] >= 0 && fi[1] < m.nv && fi[2] >= 0 && fi[2] < m.nv;
}

// area of face f in float64 (trimesh computes on float64 vertices); 0 for a face that names a vertex outside [0, nv)
__device__ __forceinline__ double face_area(const SurfMesh m, long long f) {
  if (!face_ok(m, f)) return 0.0;
  const int* fi = m.faces + 3 * f;
  const float* a = m.verts + 3 * (long long)fi[0];
  const float* b = m.verts + 3 * (long long)fi[1];
  const float* c = m.verts + 3 * (long long)fi[2];
  const double e1[3] = {(double)b[0] - a[0], (double)b[1] - a[1], (double)b[2] - a[2]};
  const double e2[3] = {(double)c[0] - a[0], (double)c[1] - a[1], (double)c[2] - a[2]};
  const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
  return 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
}

// pass 1 (CDF = false): block totals of the areas; pass 2: cdf[f] = inclusive cumulative area, summed in point order
template <bool CDF>
DISTR_GLOBAL void __launch_bounds__(MB) k_area_scan(const SurfMesh m, double* __restrict__ btot, const double* __restrict__ boff,
                                                    double* __restrict__ cdf) {
  __shared__ double lds[MB];
  const long long base = (long long)blockIdx.x * MTILE + (long long)threadIdx.x * MPER;
  double a[MPER], s = 0.0;
  for (int q = 0; q < MPER; ++q) {
    a[q] = base + q < m.nf ? face_area(m, base + q) : 0.0;
    s += a[q];
  }
  double tot;
  const double ex = block_excl_scan(s, lds, &tot);
  if (!CDF) {
    if (threadIdx.x == 0) btot[blockIdx.x] = tot;
    return;
  }
  double run = boff[blockIdx.x] + ex;
  for (int q = 0; q < MPER && base + q < m.nf; ++q) {
    run += a[q];
    cdf[base + q] = run;
  }
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {        // splitmix64 finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// counter-based random bits of (seed, sample, k): no state, the same for a given seed on any grid
__device__ __forceinline__ uint64_t rnd_bits(uint64_t seed, uint64_t i, uint64_t k) { return mix64(mix64(seed) ^ mix64(i * 4 + k)); }

DISTR_GLOBAL void __launch_bounds__(MB) k_sample(const SurfMesh m, const double* __restrict__ cdf, long long n, uint64_t seed,
                                                 float* __restrict__ pts, int* __restrict__ fidx) {
  const long long i = (long long)blockIdx.x * MB + threadIdx.x;
  if (i >= n) return;
  // face: the first whose cumulative area exceeds u * total (searchsorted on the cumulative area; a face of area 0 is never picked)
  const double pick = (double)(rnd_bits(seed, i, 0) >> 11) * 0x1.0p-53 * cdf[m.nf - 1];
  long long lo = 0, hi = m.nf - 1;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (cdf[mid] > pick) hi = mid; else lo = mid + 1;
  }
  float* d = pts + 3 * i;
  fidx[i] = (int)lo;
  if (!face_ok(m, lo)) {                                       // a face that names a vertex outside the array: no point

    d[0] = d[1] = d[2] = __int_as_float(0x7fc00000);
    return;
  }
  const int* fi = m.faces + 3 * lo;
  const float* a = m.verts + 3 * (long long)fi[0];
  const float* b = m.verts + 3 * (long long)fi[1];
  const float* c = m.verts + 3 * (long long)fi[2];
  // folded parallelogram: u1 + u2 > 1 folds back into the triangle (u -> 1 - u)
  float u1 = (float)(rnd_bits(seed, i, 1) >> 40) * 0x1.0p-24f, u2 = (float)(rnd_bits(seed, i, 2) >> 40) * 0x1.0p-24f;
  if (u1 + u2 > 1.f) { u1 = 1.f - u1; u2 = 1.f - u2; }
#pragma unroll
  for (int x = 0; x < 3; ++x) d[x] = (u1 * (b[x] - a[x]) + u2 * (c[x] - a[x])) + a[x];
}

// ------------------------------------------------------------------------------------------ nearest squared distance
constexpr int NN_TILE = 256;       // points of B per LDS tile

DISTR_GLOBAL void __launch_bounds__(MB) k_fill_inf(unsigned* __restrict__ d, long long n) {
  const long long i = (long long)blockIdx.x * MB + threadIdx.x;
  if (i < n) d[i] = 0x7f800000u;
}

// blockIdx.y = one chunk of B; the chunks' minima meet in an atomic min on the bits of a non-negative float (order-independent)
DISTR_GLOBAL void __launch_bounds__(MB) k_nearest(const float* __restrict__ A, long long na, const float* __restrict__ B, long long nb,
                                                  long long chunk, unsigned* __restrict__ d2) {
  __shared__ float4 tile[NN_TILE];
  const long long i = (long long)blockIdx.x * MB + threadIdx.x;
  float ax = 0.f, ay = 0.f, az = 0.f;
  if (i < na) { ax = A[3 * i]; ay = A[3 * i + 1]; az = A[3 * i + 2]; }
  float best = __int_as_float(0x7f800000);
  const long long b0 = (long long)blockIdx.y * chunk, b1 = b0 + chunk < nb ? b0 + chunk : nb;
  for (long long t0 = b0; t0 < b1; t0 += NN_TILE) {
    const long long j = t0 + threadIdx.x;
    const int cnt = (int)(b1 - t0 < NN_TILE ? b1 - t0 : NN_TILE);
    __syncthreads();
    if (threadIdx.x < cnt) tile[threadIdx.x] = make_float4(B[3 * j], B[3 * j + 1], B[3 * j + 2], 0.f);
    __syncthreads();
    if (cnt == NN_TILE) {
#pragma unroll 8
      for (int q = 0; q < NN_TILE; ++q) {
        const float4 b = tile[q];
        const float dx = ax - b.x, dy = ay - b.y, dz = az - b.z;
        best = fminf(best, (dx * dx + dy * dy) + dz * dz);
      }
    } else {
      for (int q = 0; q < cnt; ++q) {
        const float4 b = tile[q];
        const float dx = ax - b.x, dy = ay - b.y, dz = az - b.z;
        best = fminf(best, (dx * dx + dy * dy) + dz * dz);
      }
    }
  }
  if (i < na) atomicMin(d2 + i, __float_as_uint(best));
}

// block totals of (d2, sqrt(d2)) in float64
DISTR_GLOBAL void __launch_bounds__(MB) k_dist_sums(const float* __restrict__ d2, long long n, D2* __restrict__ btot) {
  __shared__ D2 lds[MB];
  const long long base = (long long)blockIdx.x * MTILE + (long long)threadIdx.x * MPER;
  D2 s{};
  for (int q = 0; q < MPER && base + q < n; ++q) {
    const double x = d2[base + q];
    s = s + D2{x, sqrt(x)};
  }
  D2 tot;
  block_excl_scan(s, lds, &tot);
  if (threadIdx.x == 0) btot[blockIdx.x] = tot;
}

// ------------------------------------------------------------------------------------------ signed distance to a triangle mesh
// k_sdf_pairs: one thread per query q, faces staged through LDS in tiles of SDF_TILE records (a, ab = b - a, ac = c - a and a flag:
// three float4 per face, 12 KB per tile; every lane reads the same record, a broadcast). blockIdx.y = one chunk of SDF_CHUNK faces, a
// compile-time constant: which faces a thread sums together never depends on nq or on the device, so the row of a query does not
// depend on which other queries are in the call. Brute force over all pairs, like k_nearest.
//
// A face is SKIPPED (no distance, no solid angle) when it names a vertex outside [0, nv) (face_ok), when one of its nine coordinates
// is not finite, or when its float32 cross product ab x ac is exactly (0, 0, 0): (aby*acz - abz*acy, abz*acx - abx*acz, abx*acy - aby*acx).
//
// Per pair, all in float32, no fused multiply-add (-ffp-contract=off), IEEE division and square root; dot(u, v) is
// (ux*vx + uy*vy) + uz*vz throughout:
//   ap = q - a,  bp = ap - ab,  cp = ap - ac                          (componentwise)
//   d1 = dot(ab, ap)  d2 = dot(ac, ap)  d3 = dot(ab, bp)  d4 = dot(ac, bp)  d5 = dot(ab, cp)  d6 = dot(ac, cp)
//   vc = d1*d4 - d3*d2,  vb = d5*d2 - d1*d6,  va = d3*d6 - d5*d4,  e43 = d4 - d3,  e56 = d5 - d6
//   (sn, sd, tn, td) and the second direction e, the first of (Ericson, Real-Time Collision Detection 5.1.5, in its order):
//     d1 <= 0 and d2 <= 0                 vertex a   (0, 1, 0, 1)                                   e = ac
//     d3 >= 0 and d4 <= d3                vertex b   (1, 1, 0, 1)                                   e = ac
//     vc <= 0 and d1 >= 0 and d3 <= 0     edge ab    (d1, d1 - d3, 0, 1)                            e = ac
//     d6 >= 0 and d5 <= d6                vertex c   (0, 1, 1, 1)                                   e = ac
//     vb <= 0 and d2 >= 0 and d6 <= 0     edge ac    (0, 1, d2, d2 - d6)                            e = ac
//     va <= 0 and e43 >= 0 and e56 >= 0   edge bc    (1, 1, e43, e43 + e56)                         e = ac - ab
//     otherwise                           interior   (vb, (va + vb) + vc, vc, (va + vb) + vc)       e = ac
//   s = sn / sd,  t = tn / td,  p = (a + s*ab) + t*e,  d = q - p,  dist2 = (dx*dx + dy*dy) + dz*dz
// (edge bc is Ericson's b + w (c - b) with b = a + ab: two independently rounded weights s + t = 1 on ab and ac would leave p off the
// edge by an ulp of the edge's length in every coordinate, also in those where b and c agree.)
// A pair counts for the minimum only when dist2 < +inf (a 0 / 0 of a face too small for float32, or an overflow, never wins). Ties go
// to the lowest face index: within a thread faces come in ascending order under a strict <, between chunks the key
// (bits(dist2) << 32) | face meets in an integer atomicMin (dist2 >= +0, so the order of the bits is the order of the values).
//
// Signed solid angle (Van Oosterom & Strackee) of the same pair:
//   A = a - q,  B = A + ab,  C = A + ac
//   cr = (By*Cz - Bz*Cy, Bz*Cx - Bx*Cz, Bx*Cy - By*Cx),  num = dot(A, cr)
//   la = sqrt(dot(A, A)),  lb = sqrt(dot(B, B)),  lc = sqrt(dot(C, C))
//   den = ((((la*lb)*lc) + dot(A, B)*lc) + dot(B, C)*la) + dot(C, A)*lb
//   half = atan2f(num, den)                                            (Omega = 2 * half)
// A thread adds `half` in float32 over one tile in face order (from +0), adds the tile sums to a float64 in tile order and writes the
// chunk's float64 to wsum[chunk][query]; k_sdf_finish adds the chunks in chunk order and scales by 1 / (2 pi): the generalised winding
// number w = sum(Omega) / (4 pi), +1 inside a closed mesh whose normals point outwards, 0 outside. No float atomic anywhere.
constexpr int SDF_TILE = 256;      // face records per LDS tile
constexpr int SDF_CHUNK = 1024;    // faces per blockIdx.y: a constant of the ABI (distr.mesh.SDF_CHUNK mirrors it)
constexpr unsigned long long SDF_NONE = 0x7f800000ffffffffull;     // (+inf, face -1): no face counted

__device__ __forceinline__ float dot3(float ux, float uy, float uz, float vx, float vy, float vz) { return (ux * vx + uy * vy) + uz * vz; }
__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ void cross3(const float* p, const float* q, float* r) {
  r[0] = p[1] * q[2] - p[2] * q[1];
  r[1] = p[2] * q[0] - p[0] * q[2];
  r[2] = p[0] * q[1] - p[1] * q[0];
}

// the skip rule (above) of k_sdf_pairs, and of k_mesh_cast further down: is face f counted
__device__ __forceinline__ bool face_counted(const SurfMesh m, long long f) {
  if (!face_ok(m, f)) return false;
  const int* fi = m.faces + 3 * f;
  const float* a = m.verts + 3 * (long long)fi[0];
  const float* b = m.verts + 3 * (long long)fi[1];
  const float* c = m.verts + 3 * (long long)fi[2];
  const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  float n[3];
  cross3(ab, ac, n);
  bool fin = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) fin = fin && finite_f(a[i]) && finite_f(b[i]) && finite_f(c[i]);
  return fin && !(n[0] == 0.f && n[1] == 0.f && n[2] == 0.f);
}

DISTR_GLOBAL void __launch_bounds__(MB) k_sdf_init(unsigned long long* __restrict__ best, long long n) {
  const long long i = (long long)blockIdx.x * MB + threadIdx.x;
  if (i < n) best[i] = SDF_NONE;
}

DISTR_GLOBAL void __launch_bounds__(MB) k_sdf_pairs(const SurfMesh m, const float* __restrict__ Q, long long nq,
                                                    unsigned long long* __restrict__ best, double* __restrict__ wsum) {
  __shared__ float4 tile[3][SDF_TILE];     // [0] a.xyz, ab.x   [1] ab.yz, ac.xy   [2] ac.z, flag (1 counted, 0 skipped), -, -
  const long long i = (long long)blockIdx.x * MB + threadIdx.x;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (i < nq) { qx = Q[3 * i]; qy = Q[3 * i + 1]; qz = Q[3 * i + 2]; }
  const float inf = __int_as_float(0x7f800000);
  float bestd = inf;
  unsigned bestf = 0xffffffffu;
  double wacc = 0.0;
  const long long f0 = (long long)blockIdx.y * SDF_CHUNK, f1 = f0 + SDF_CHUNK < m.nf ? f0 + SDF_CHUNK : m.nf;
  for (long long t0 = f0; t0 < f1; t0 += SDF_TILE) {
    const int cnt = (int)(f1 - t0 < SDF_TILE ? f1 - t0 : SDF_TILE);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
      const long long f = t0 + threadIdx.x;
      float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
      if (face_counted(m, f)) {
        const int* fi = m.faces + 3 * f;
        const float* a = m.verts + 3 * (long long)fi[0];
        const float* b = m.verts + 3 * (long long)fi[1];
        const float* c = m.verts + 3 * (long long)fi[2];
        r0 = make_float4(a[0], a[1], a[2], b[0] - a[0]);
        r1 = make_float4(b[1] - a[1], b[2] - a[2], c[0] - a[0], c[1] - a[1]);
        r2 = make_float4(c[2] - a[2], 1.f, 0.f, 0.f);
      }
      tile[0][threadIdx.x] = r0;
      tile[1][threadIdx.x] = r1;
      tile[2][threadIdx.x] = r2;
    }
    __syncthreads();
    float wt = 0.f;
#pragma unroll 2
    for (int k = 0; k < cnt; ++k) {
      const float4 r2 = tile[2][k];
      if (r2.y == 0.f) continue;                               // a skipped face (the same for every lane)
      const float4 r0 = tile[0][k], r1 = tile[1][k];
      const float ax = r0.x, ay = r0.y, az = r0.z, abx = r0.w, aby = r1.x, abz = r1.y, acx = r1.z, acy = r1.w, acz = r2.x;
      // closest point of the triangle
      const float apx = qx - ax, apy = qy - ay, apz = qz - az;
      const float bpx = apx - abx, bpy = apy - aby, bpz = apz - abz;
      const float cpx = apx - acx, cpy = apy - acy, cpz = apz - acz;
      const float d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
      const float d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
      const float d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
      const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
      const float e43 = d4 - d3, e56 = d5 - d6;
      float sn = vb, tn = vc, sd = (va + vb) + vc, td = sd;    // interior, then the regions from the last to the first in priority
      bool bc = false;
      if (va <= 0.f && e43 >= 0.f && e56 >= 0.f) { sn = 1.f; sd = 1.f; tn = e43; td = e43 + e56; bc = true; }
      if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { sn = 0.f; sd = 1.f; tn = d2; td = d2 - d6; bc = false; }
      if (d6 >= 0.f && d5 <= d6) { sn = 0.f; sd = 1.f; tn = 1.f; td = 1.f; bc = false; }
      if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { sn = d1; sd = d1 - d3; tn = 0.f; td = 1.f; bc = false; }
      if (d3 >= 0.f && d4 <= d3) { sn = 1.f; sd = 1.f; tn = 0.f; td = 1.f; bc = false; }
      if (d1 <= 0.f && d2 <= 0.f) { sn = 0.f; sd = 1.f; tn = 0.f; td = 1.f; bc = false; }
      const float s = sn / sd, t = tn / td;
      const float ex = bc ? acx - abx : acx, ey = bc ? acy - aby : acy, ez = bc ? acz - abz : acz;
      const float dx = qx - ((ax + s * abx) + t * ex), dy = qy - ((ay + s * aby) + t * ey), dz = qz - ((az + s * abz) + t * ez);
      const float dist2 = (dx * dx + dy * dy) + dz * dz;
      if (dist2 < bestd) { bestd = dist2; bestf = (unsigned)(t0 + k); }       // NaN never passes; +inf never beats the initial +inf
      // signed solid angle
      const float Ax = ax - qx, Ay = ay - qy, Az = az - qz;
      const float Bx = Ax + abx, By = Ay + aby, Bz = Az + abz;
      const float Cx = Ax + acx, Cy = Ay + acy, Cz = Az + acz;
      const float num = dot3(Ax, Ay, Az, By * Cz - Bz * Cy, Bz * Cx - Bx * Cz, Bx * Cy - By * Cx);
      const float la = sqrtf(dot3(Ax, Ay, Az, Ax, Ay, Az)), lb = sqrtf(dot3(Bx, By, Bz, Bx, By, Bz)), lc = sqrtf(dot3(Cx, Cy, Cz, Cx, Cy, Cz));
      const float den = ((((la * lb) * lc) + dot3(Ax, Ay, Az, Bx, By, Bz) * lc) + dot3(Bx, By, Bz, Cx, Cy, Cz) * la) +
                        dot3(Cx, Cy, Cz, Ax, Ay, Az) * lb;
      wt += atan2f(num, den);
    }
    wacc += (double)wt;
  }
  if (i < nq) {
    wsum[(long long)blockIdx.y * nq + i] = wacc;
    if (bestf != 0xffffffffu) atomicMin(best + i, (unsigned long long)__float_as_uint(bestd) << 32 | bestf);
  }
}

// Adds the chunks' float64 solid-angle sums in chunk order and writes the outputs: sdf = (|w| > 0.5 ? -1 : +1) * sqrtf(dist2) with w in
// float32 (|w|: a consistently inward-wound mesh gives the same signs). No counted face: sdf = +inf, face = -1. A query with a
// coordinate that is not finite: sdf = dist2 = w = NaN, face = -1. d2 / w / face may be null.
DISTR_GLOBAL void __launch_bounds__(MB) k_sdf_finish(const float* __restrict__ Q, long long nq, const unsigned long long* __restrict__ best,
                                                     const double* __restrict__ wsum, long long nchunks, float* __restrict__ sdf,
                                                     float* __restrict__ d2, float* __restrict__ wind, int* __restrict__ face) {
  const long long i = (long long)blockIdx.x * MB + threadIdx.x;
  if (i >= nq) return;
  double tot = 0.0;
  for (long long c = 0; c < nchunks; ++c) tot += wsum[c * nq + i];
  float w = (float)(tot * 0.15915494309189535);                  // 1 / (2 pi): the sums are of Omega / 2
  const unsigned long long key = best[i];
  float dist2 = __uint_as_float((unsigned)(key >> 32));
  int f = (int)(unsigned)(key & 0xffffffffu);
  float out = (fabsf(w) > 0.5f ? -1.f : 1.f) * sqrtf(dist2);
  if (!(finite_f(Q[3 * i]) && finite_f(Q[3 * i + 1]) && finite_f(Q[3 * i + 2]))) {
    out = dist2 = w = __int_as_float(0x7fc00000);
    f = -1;
  }
  sdf[i] = out;
  if (d2) d2[i] = dist2;
  if (wind) wind[i] = w;
  if (face) face[i] = f;
}

// ------------------------------------------------------------------------------------------ DeepSDF-style query points
// From ns surface points (distr_sample_surface) 2 * ns + nu queries, each a pure function of (seed, its index):
//   out[2 i]     = p_i + sigma_a * (z0, z1, z2)          out[2 i + 1] = p_i + sigma_b * (z3, z4, z5)         i < ns
//   out[2 ns + j] = ((2 ux - 1) * h, (2 uy - 1) * h, (2 uz - 1) * h)                                           j < nu
// Random words: W(n) = rnd_bits(seed, n, 3) -- slot k = 3, which k_sample (k = 0..2 of its sample index) never draws: the counters
// 4 n + 3 and 4 i + k <= 2 differ for every n and i. Surface point i owns W(8 i), W(8 i + 1), W(8 i + 2), uniform point j owns
// W(8 j + 4), W(8 j + 5). A word gives two 24-bit numbers, hi = W >> 40 and lo = (W >> 8) & 0xffffff.
//   Box-Muller of word m = 0, 1, 2 of point i: u1 = (hi + 1) * 2^-24 in (0, 1], u2 = lo * 2^-24 in [0, 1),
//     r = sqrtf(-2 * logf(u1)),  ang = 6.2831855f * u2,  z(2m) = r * cosf(ang),  z(2m + 1) = r * sinf(ang)
//   uniform point j: ux = hi(W(8 j + 4)) * 2^-24, uy = lo(W(8 j + 4)) * 2^-24, uz = hi(W(8 j + 5)) * 2^-24
DISTR_GLOBAL void __launch_bounds__(MB) k_sdf_queries(const float* __restrict__ surf, long long ns, float sigma_a, float sigma_b,
                                                      long long nu, float h, uint64_t seed, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * MB + threadIdx.x;
  if (i < ns) {
    float z[6];
#pragma unroll
    for (int mth = 0; mth < 3; ++mth) {
      const uint64_t w = rnd_bits(seed, 8ull * (uint64_t)i + mth, 3);
      const float u1 = (float)((unsigned)(w >> 40) + 1u) * 0x1.0p-24f, u2 = (float)((unsigned)(w >> 8) & 0xffffffu) * 0x1.0p-24f;
      const float r = sqrtf(-2.f * logf(u1)), ang = 6.2831855f * u2;
      z[2 * mth] = r * cosf(ang);
      z[2 * mth + 1] = r * sinf(ang);
    }
    const float* p = surf + 3 * i;
    float* d = out + 6 * i;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      d[x] = p[x] + sigma_a * z[x];
      d[3 + x] = p[x] + sigma_b * z[3 + x];
    }
  }
  if (i < nu) {
    const uint64_t w0 = rnd_bits(seed, 8ull * (uint64_t)i + 4, 3), w1 = rnd_bits(seed, 8ull * (uint64_t)i + 5, 3);
    float* d = out + 3 * (2 * ns + i);
    d[0] = (2.f * ((float)(unsigned)(w0 >> 40) * 0x1.0p-24f) - 1.f) * h;
    d[1] = (2.f * ((float)((unsigned)(w0 >> 8) & 0xffffffu) * 0x1.0p-24f) - 1.f) * h;
    d[2] = (2.f * ((float)(unsigned)(w1 >> 40) * 0x1.0p-24f) - 1.f) * h;
  }
}

// ------------------------------------------------------------------------------------------ depth, normal and mask maps of a mesh
// k_mesh_cast: rays of up to DISTR_MAX_VIEWS pinhole views against every triangle, brute force over all (ray, triangle) pairs; the
// nearest hit per pixel as the key (bits(t) << 32) | face in best[view][pixel]. k_mesh_finish decodes the key and writes the maps.
// Not differentiable: the maps are observations (the depth / normal arguments of get_samples, the targets of the image losses).
//
// All rays of a view start at the camera, so the work happens in the mesh's frame with the camera at the origin. Everything is
// float32, no fused multiply-add (-ffp-contract=off), IEEE division and square root; sums run left to right where no brackets are
// written; dot(u, v) is (ux*vx + uy*vy) + uz*vz and cross(p, q) = (py*qz - pz*qy, pz*qx - px*qz, px*qy - py*qx).
//
// Per view (RT = [R | T], row-major 3 x 4; the order of k_prep and make_point):
//   c[i] = -(R[0][i]*T[0] + R[1][i]*T[1] + R[2][i]*T[2]),   o[i] = M[0][i]*c[0] + M[1][i]*c[1] + M[2][i]*c[2]        (o = M^T c)
// Per pixel (x, y) = (pix % W, pix / W) as floats: d and calib of make_ray(K_inv, R, x, y);
//   e[i] = M[0][i]*d[0] + M[1][i]*d[1] + M[2][i]*d[2]                                                                 (e = M^T d)
// Per triangle (a, b, c) and view: A = a - o, B = b - o, C = c - o;  Na = cross(C, B), Nb = cross(A, C), Nc = cross(B, A).
// Per pair: U = dot(e, Na), V = dot(e, Nb), W = dot(e, Nc). The two triangles of an indexed mesh that share an edge get edge
// functions that are exact negatives of each other (products commute, p*q - r*s = -(r*s - p*q)), so a ray never passes between them.
// The pair is a HIT when
//   not ((U < 0 or V < 0 or W < 0) and (U > 0 or V > 0 or W > 0))          zeros are inclusive
//   det = (U + V) + W != 0
//   t = dot(A, Ng) / dot(e, Ng) is finite and > 0, with E1 = B - A, E2 = C - A, Ng = cross(E1, E2)   (computed on such a pair only)
// The nearest hit wins, the lowest face among equal t: t > 0, so the order of the keys is the order of (t, face); a thread keeps the
// smallest key of its chunk, the chunks (blockIdx.y, RC_CHUNK faces, a compile-time constant) meet in the integer atomicMin of
// k_sdf_pairs. The result depends neither on the arrival order nor on the chunking. No float atomic: the same bytes on every run.
// Outputs of a hit (k_mesh_finish recomputes A .. Ng of the winning face with the same operations):
//   zdepth = t,  depth = t * calib,  bary = (V / det, W / det) (the weights of b and c),  face,  mask = 1
//   n = (dot(e, Ng) > 0 ? -Ng : Ng) / sqrtf(dot(Ng, Ng)) + 0                (towards the camera whatever the winding; + 0 turns a
//                                                                            -0 component into +0, so both windings give the same bytes)
//   world:  w[i] = M[i][0]*n[0] + M[i][1]*n[1] + M[i][2]*n[2]               (M n; get_samples multiplies by M^T itself)
//   image:  r[i] = R[i][0]*w[0] + R[i][1]*w[1] + R[i][2]*w[2], r[0] = -r[0] (render's autograd normals: R (M n), x negated)
// A miss: depth = zdepth = 1e11, normal = bary = 0, face = -1, mask = 0.
// A face is SKIPPED by the rule of k_sdf_pairs (a vertex outside [0, nv), a coordinate that is not finite, a float32 cross product
// (b - a) x (c - a) of exactly zero); a view whose RT holds a number that is not finite skips every face: all misses.
//
// Layout: a thread owns RC_PPT pixels (blockIdx.x * MB * RC_PPT + q * MB + threadIdx.x: every record read from LDS serves RC_PPT
// edge tests); blockIdx.z = the view. The staging thread forms the record (Na, Nb, Nc, counted: three float4) of its face from the
// vertices and the view's o, so there is no record workspace; every lane reads the same record, a broadcast.
constexpr int RC_TILE = 256;       // face records per LDS tile (12 KB)
constexpr int RC_CHUNK = 1024;     // faces per blockIdx.y (distr.mesh.RENDER_CHUNK mirrors it)
constexpr int RC_PPT = 2;          // pixels per thread
constexpr int FRAME_WORLD = 0, FRAME_IMAGE = 1;     // DISTR_MESH_NORMAL_*

struct CastGeo {                   // per call
  int H, W, P;                     // P = H * W
  float Ki[9], M[9];
  int frame;
};
struct CastCam { float R[9], o[3]; bool ok; };
struct CastOut { float* depth; float* zdepth; float* normal; uint8_t* mask; int* face; float* bary; };     // [view][pixel]; any may be null

__device__ __forceinline__ CastCam cast_cam(const CastGeo& G, const float* __restrict__ RT) {
  CastCam k;
  float T[3], c[3];
  k.ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { k.R[j * 3 + i] = RT[j * 4 + i]; k.ok = k.ok && finite_f(k.R[j * 3 + i]); }
    T[j] = RT[j * 4 + 3];
    k.ok = k.ok && finite_f(T[j]);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) c[i] = -(k.R[0 * 3 + i] * T[0] + k.R[1 * 3 + i] * T[1] + k.R[2 * 3 + i] * T[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) k.o[i] = G.M[0 * 3 + i] * c[0] + G.M[1 * 3 + i] * c[1] + G.M[2 * 3 + i] * c[2];
  return k;
}

// e = M^T d of pixel pix; returns calib
__device__ __forceinline__ float cast_ray(const CastGeo& G, const CastCam& cam, int pix, float* e) {
  const RayGeo g = make_ray(G.Ki, cam.R, (float)(pix % G.W), (float)(pix / G.W));
#pragma unroll
  for (int i = 0; i < 3; ++i) e[i] = G.M[0 * 3 + i] * g.d[0] + G.M[1 * 3 + i] * g.d[1] + G.M[2 * 3 + i] * g.d[2];
  return g.calib;
}

// corners of a counted face relative to the camera
__device__ __forceinline__ void face_rel(const SurfMesh m, long long f, const float* o, float* A, float* B, float* C) {
  const int* fi = m.faces + 3 * f;
  const float* a = m.verts + 3 * (long long)fi[0];
  const float* b = m.verts + 3 * (long long)fi[1];
  const float* c = m.verts + 3 * (long long)fi[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) { A[i] = a[i] - o[i]; B[i] = b[i] - o[i]; C[i] = c[i] - o[i]; }
}

// t of a pair whose edge functions agree in sign; Ng and den = dot(e, Ng) on the way
__device__ __forceinline__ float face_t(const float* A, const float* B, const float* C, const float* e, float* Ng, float* den) {
  const float E1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, E2[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
  cross3(E1, E2, Ng);
  *den = dot3(e[0], e[1], e[2], Ng[0], Ng[1], Ng[2]);
  return dot3(A[0], A[1], A[2], Ng[0], Ng[1], Ng[2]) / *den;
}

__device__ __forceinline__ bool signs_mixed(float U, float V, float W) {
  return (U < 0.f || V < 0.f || W < 0.f) && (U > 0.f || V > 0.f || W > 0.f);
}

// grid (blocks of MB * RC_PPT pixels, chunks of RC_CHUNK faces, views); best[view][pixel] preset to SDF_NONE (k_sdf_init)
DISTR_GLOBAL void __launch_bounds__(MB) k_mesh_cast(const SurfMesh m, const CastGeo G, const float* __restrict__ RT,
                                                    unsigned long long* __restrict__ best) {
  __shared__ float4 tile[3][RC_TILE];      // [0] Na.xyz, Nb.x   [1] Nb.yz, Nc.xy   [2] Nc.z, flag (1 counted, 0 skipped), -, -
  const int v = blockIdx.z;
  const CastCam cam = cast_cam(G, RT + 12 * v);
  const long long i0 = (long long)blockIdx.x * (MB * RC_PPT) + threadIdx.x;
  float e[RC_PPT][3];
  unsigned long long bk[RC_PPT];
#pragma unroll
  for (int q = 0; q < RC_PPT; ++q) {
    const long long i = i0 + q * MB;
    cast_ray(G, cam, i < G.P ? (int)i : 0, e[q]);               // a lane beyond the image casts pixel 0's ray and writes nothing
    bk[q] = SDF_NONE;
  }
  const long long f0 = (long long)blockIdx.y * RC_CHUNK, f1 = f0 + RC_CHUNK < m.nf ? f0 + RC_CHUNK : m.nf;
  for (long long t0 = f0; t0 < f1; t0 += RC_TILE) {
    const int cnt = (int)(f1 - t0 < RC_TILE ? f1 - t0 : RC_TILE);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
      const long long f = t0 + threadIdx.x;
      float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
      if (cam.ok && face_counted(m, f)) {
        float A[3], B[3], C[3], Na[3], Nb[3], Nc[3];
        face_rel(m, f, cam.o, A, B, C);
        cross3(C, B, Na);
        cross3(A, C, Nb);
        cross3(B, A, Nc);
        r0 = make_float4(Na[0], Na[1], Na[2], Nb[0]);
        r1 = make_float4(Nb[1], Nb[2], Nc[0], Nc[1]);
        r2 = make_float4(Nc[2], 1.f, 0.f, 0.f);
      }
      tile[0][threadIdx.x] = r0;
      tile[1][threadIdx.x] = r1;
      tile[2][threadIdx.x] = r2;
    }
    __syncthreads();
#pragma unroll 2
    for (int k = 0; k < cnt; ++k) {
      const float4 r2 = tile[2][k];
      if (r2.y == 0.f) continue;                                 // a skipped face (the same for every lane)
      const float4 r0 = tile[0][k], r1 = tile[1][k];
#pragma unroll
      for (int q = 0; q < RC_PPT; ++q) {
        const float U = dot3(e[q][0], e[q][1], e[q][2], r0.x, r0.y, r0.z);
        const float V = dot3(e[q][0], e[q][1], e[q][2], r0.w, r1.x, r1.y);
        const float W = dot3(e[q][0], e[q][1], e[q][2], r1.z, r1.w, r2.x);
        if (signs_mixed(U, V, W) || (U + V) + W == 0.f) continue;
        float A[3], B[3], C[3], Ng[3], den;                      // rare: a few faces per ray
        face_rel(m, t0 + k, cam.o, A, B, C);
        const float t = face_t(A, B, C, e[q], Ng, &den);
        if (!(finite_f(t) && t > 0.f)) continue;
        const unsigned long long key = (unsigned long long)__float_as_uint(t) << 32 | (unsigned)(t0 + k);
        if (key < bk[q]) bk[q] = key;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < RC_PPT; ++q) {
    const long long i = i0 + q * MB;
    if (i < G.P && bk[q] != SDF_NONE) atomicMin(best + (long long)v * G.P + i, bk[q]);
  }
}

// grid (blocks of MB pixels, views)
DISTR_GLOBAL void __launch_bounds__(MB) k_mesh_finish(const SurfMesh m, const CastGeo G, const float* __restrict__ RT,
                                                      const unsigned long long* __restrict__ best, const CastOut O) {
  const int i = blockIdx.x * MB + threadIdx.x, v = blockIdx.y;
  if (i >= G.P) return;
  const long long at = (long long)v * G.P + i;
  const unsigned long long key = best[at];
  float depth = 1e11f, z = 1e11f, n[3] = {0.f, 0.f, 0.f}, bu = 0.f, bv = 0.f;
  int f = -1;
  if (key != SDF_NONE) {
    f = (int)(unsigned)(key & 0xffffffffu);
    const CastCam cam = cast_cam(G, RT + 12 * v);
    float e[3], A[3], B[3], C[3], Nb[3], Nc[3], Ng[3], den;
    const float calib = cast_ray(G, cam, i, e);
    face_rel(m, f, cam.o, A, B, C);
    float Na[3];
    cross3(C, B, Na);
    cross3(A, C, Nb);
    cross3(B, A, Nc);
    const float U = dot3(e[0], e[1], e[2], Na[0], Na[1], Na[2]);
    const float V = dot3(e[0], e[1], e[2], Nb[0], Nb[1], Nb[2]);
    const float W = dot3(e[0], e[1], e[2], Nc[0], Nc[1], Nc[2]);
    const float det = (U + V) + W;
    z = face_t(A, B, C, e, Ng, &den);                            // the bits of the key
    depth = z * calib;
    bu = V / det;
    bv = W / det;
    const float len = sqrtf(dot3(Ng[0], Ng[1], Ng[2], Ng[0], Ng[1], Ng[2]));
    float g[3], w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = (den > 0.f ? -Ng[k] : Ng[k]) / len + 0.f;          // + 0: a zero component is +0 for either winding
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = G.M[k * 3 + 0] * g[0] + G.M[k * 3 + 1] * g[1] + G.M[k * 3 + 2] * g[2];
    if (G.frame == FRAME_IMAGE) {
#pragma unroll
      for (int k = 0; k < 3; ++k) n[k] = cam.R[k * 3 + 0] * w[0] + cam.R[k * 3 + 1] * w[1] + cam.R[k * 3 + 2] * w[2];
      n[0] = -n[0];
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) n[k] = w[k];
    }
  }
  if (O.depth) O.depth[at] = depth;
  if (O.zdepth) O.zdepth[at] = z;
  if (O.normal) { O.normal[3 * at] = n[0]; O.normal[3 * at + 1] = n[1]; O.normal[3 * at + 2] = n[2]; }
  if (O.mask) O.mask[at] = f >= 0 ? 1 : 0;
  if (O.face) O.face[at] = f;
  if (O.bary) { O.bary[2 * at] = bu; O.bary[2 * at + 1] = bv; }
}

}  // namespace mesh
}  // namespace distr
