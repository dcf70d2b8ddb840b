"""compute_chamfer_distance / compute_chamfer_distance_separate with the reference's names, signatures and formulas
(core/evaluation/eval_func.py), by brute force on the GPU instead of two scipy KD-trees (distr.mesh.chamfer)."""
from distr import mesh as _mesh

__all__ = ['compute_chamfer_distance', 'compute_chamfer_distance_separate']


def compute_chamfer_distance(points_1, points_2, use_square_dist=True):
    """Symmetric chamfer distance: the sum of both directions' mean (squared) nearest-point distances."""
    return _mesh.chamfer(points_1, points_2, use_square_dist=use_square_dist)


def compute_chamfer_distance_separate(points_1, points_2):
    """(mean over points_2 of the squared distance to points_1, mean over points_1 of the squared distance to points_2)."""
    return _mesh.chamfer(points_1, points_2, separate=True)
