"""core.evaluation: bulk SDF-grid evaluation and shape evaluation on the GPU -- marching cubes, surface sampling,
chamfer distance (distr.mesh) behind the reference's names: create_mesh*, latent_vec_to_points, compute_chamfer_distance*,
Evaluator (core/evaluation/__init__.py:3-5). When a reference checkout is importable next to this build its Evaluator is re-exported
(its `from eval_func import *` / `from transforms import *` land on this build's flat modules, so it runs on the GPU too); without
one, gpu_evaluator.Evaluator stands in."""
import os
import types

from core import _dropin

__path__ = _dropin.extend(__path__, __name__)

from .create_mesh import (create_mesh, create_mesh_speedup, create_sdf_grid, create_sdf_grid_speedup, get_samples,   # noqa: E402
                          infer_samples)
from .eval_func import compute_chamfer_distance, compute_chamfer_distance_separate                                  # noqa: E402
from .transforms import decode_sdf, latent_vec_to_points, sample_points_from_ply_file                              # noqa: E402

_dropin.absorb(globals(), __name__, ('evaluator', 'eval_func', 'transforms'), os.path.dirname(os.path.abspath(__file__)))
from .gpu_evaluator import Evaluator as _GpuEvaluator                                                              # noqa: E402
globals().setdefault('Evaluator', _GpuEvaluator)
__all__ = [n for n, v in globals().items() if not n.startswith('_') and not isinstance(v, types.ModuleType)]
