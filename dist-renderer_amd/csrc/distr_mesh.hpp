// distr_mesh.hpp -- shape evaluation after the render path (reference: core/evaluation/create_mesh.py, transforms.py, eval_func.py):
//
//   marching cubes     over a dense f32 grid (nx, ny, nz), x slowest (the layout create_sdf_grid returns)
//   surface sampling   area-weighted, trimesh.sample.sample_surface's rule (searchsorted on the cumulative area, folded parallelogram)
//   nearest distance   brute force squared distance from every point of A to the nearest of B (one chamfer direction)
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

#include "distr_mlp.hpp"        // DISTR_GLOBAL

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

}  // namespace mesh
}  // namespace distr
