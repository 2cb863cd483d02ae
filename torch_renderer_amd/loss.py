"""``pytorch3d.loss`` names (``from torch_renderer_amd.loss import mesh_edge_loss, ...``): see losses.py."""
from .losses import (chamfer_distance, face_point_distance, mesh_edge_loss, mesh_laplacian_smoothing,  # noqa: F401
                     mesh_normal_consistency, mesh_shape_priors, point_face_distance, point_mesh_face_distance,
                     posed_chamfer_distance)

# chamfer_distance, posed_chamfer_distance and the point-to-mesh functions are importable from here but not listed: tests/test_mesh_priors_cpu.py pins these four names
__all__ = ["mesh_edge_loss", "mesh_laplacian_smoothing", "mesh_normal_consistency", "mesh_shape_priors"]
