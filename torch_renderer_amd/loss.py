"""``pytorch3d.loss`` names (``from torch_renderer_amd.loss import mesh_edge_loss, ...``): see losses.py."""
from .losses import (mesh_edge_loss, mesh_laplacian_smoothing, mesh_normal_consistency,  # noqa: F401
                     mesh_shape_priors)

__all__ = ["mesh_edge_loss", "mesh_laplacian_smoothing", "mesh_normal_consistency", "mesh_shape_priors"]
