"""latent_vec_to_points / sample_points_from_ply_file with the reference's names and signatures (core/evaluation/transforms.py),
on the GPU: SDF grid -> marching cubes -> area-weighted samples without leaving the device (distr.mesh); the PLY is written only when
a file name is given. Re-exports create_mesh, create_mesh_speedup and decode_sdf like the reference's file: its evaluator.py does
`from transforms import *` and relies on them."""
import numpy as np
import torch

from core.evaluation.create_mesh import create_mesh, create_mesh_speedup, create_sdf_grid, create_sdf_grid_speedup
from core.utils.decoder_utils import decode_sdf
from distr import mesh as _mesh

__all__ = ['create_mesh', 'create_mesh_speedup', 'decode_sdf', 'sample_points_from_ply_file', 'latent_vec_to_points']


def sample_points_from_ply_file(fname, num_points, seed=0):
    """(num_points, 3) float64 surface samples of a triangle PLY (trimesh.load + sample_surface in the reference), drawn on the GPU."""
    verts, faces = _mesh.read_ply(fname)
    dev = torch.device('cuda', torch.cuda.current_device())
    pts, _ = _mesh.sample_surface(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), num_points, seed)
    return pts.cpu().numpy().astype(np.float64)


def latent_vec_to_points(decoder, latent_vec, N=256, max_batch=32 ** 3, num_points=30000, silent=False, fname=None, transform=False,
                         meshcreator_type='speedup', seed=0):
    """Surface samples (num_points, 3) float64 of the decoder's zero level set, or None when the grid does not cross 0.
    meshcreator_type 'speedup': the coarse-to-fine grid of create_mesh_speedup, 'original': the plain grid of create_mesh. fname: the
    mesh is also written there as PLY. seed (not in the reference, which draws from numpy's global generator): the sampling seed."""
    if meshcreator_type == 'original':
        grid = create_sdf_grid(decoder, latent_vec, N, transform)
    elif meshcreator_type == 'speedup':
        grid = create_sdf_grid_speedup(decoder, latent_vec, N, transform)
    else:
        raise NotImplementedError
    verts, faces = _mesh.marching_cubes(grid, 0.0, origin=(-1.0, -1.0, -1.0), voxel_size=2.0 / (N - 1))
    if faces.shape[0] == 0:
        return None
    if fname is not None:
        _mesh.write_ply(fname, verts, faces)
    pts, _ = _mesh.sample_surface(verts, faces, num_points, seed)
    return pts.cpu().numpy().astype(np.float64)
