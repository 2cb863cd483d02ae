"""Fused losses: the pose optimiser's loss, the mesh shape priors of the deformation loops and the chamfer distance.

Chamfer distance (``pytorch3d.loss.chamfer_distance`` as the geometry-fitting loops call it on sampled points,
mesh_deformer.py:299-352, deform_mesh_from_pcd.py:160-212, and on whole clouds, chamfer_loss_evaluation.py:126):
``chamfer_distance`` is one autograd node over a tiled nearest-neighbour kernel that keeps the targets in LDS and
never writes the (N, P1, P2) distance matrix (kernels.ChamferDistance, csrc/mr_points.hip). Deterministic.
``posed_chamfer_distance`` scores S pose hypotheses of ONE cloud pair (the inner loop of chamfer_loss_evaluation.py:
105-126 and pytorch3d_icp_evaluation.py:158-239) in one fused pass that never materialises the S transformed clouds,
with gradients to the poses (kernels.PosedChamfer).

Point to mesh (``pytorch3d.loss.point_mesh_face_distance`` for a target that is a scan, deform_mesh_from_pcd.py):
``point_mesh_face_distance`` is one autograd node over an all-pairs point-to-triangle kernel that never writes a
(P, T) matrix (kernels.PointMeshFaceDistance, csrc/mr_pointmesh.hip); ``point_face_distance`` and
``face_point_distance`` are upstream's unreduced per-point and per-face distances over the same kernels.
Deterministic.

Mesh shape priors (``pytorch3d.loss.mesh_edge_loss`` / ``mesh_laplacian_smoothing`` / ``mesh_normal_consistency``,
called together by update_mesh_shape_prior_losses at deform_mesh_with_color.py:248-256 and mesh_deformer.py:
314-320): ``mesh_shape_priors`` returns all three from one autograd node — one HIP pass over the edges,
vertices and face pairs plus a fixed-order reduction forward, one gathering launch backward
(kernels.MeshShapePriors, csrc/mr_priors.hip) — instead of ~40 torch index / elementwise launches each way. The
three upstream-named functions run the same node with only their own term switched on. Deterministic.

Fused pose-optimiser loss.

``pose_loss`` is camera_pose_optimizer.py:257-276 ``Model.calc_loss`` in three HIP launches forward
(mask count, one pass that sums the loss AND writes its gradients for dL/dtotal = 1, final reduction)
and one near-empty rescale in the backward (``mr_pose_loss_*``), instead of ~15 torch elementwise /
reduction kernels forward and as many backward:

* ``sil_loss   = torch.nn.L1Loss()(silhouette, mask.float())``
* ``hloss      = torch.nn.HuberLoss(delta=0.05)(depth[mask], depth_ref[mask])``
* ``color_loss = torch.nn.MSELoss()(color, rgb_ref)``
* ``total      = sil_loss + hloss + 0.01 * color_loss``

``color`` may be the RGBA view ``image[..., :3]`` and ``silhouette`` the view ``sil_image[..., 3]``
the reference passes (camera_pose_optimizer.py:248,250): both are read in place, and their gradients
are written by the loss's backward straight in the RGBA images' layout (zero in the channels the
views leave out) and handed to autograd for the images themselves — what the slices' backward
would produce, without its zero-filled (N,H,W,4) buffer and strided copy per image. The reductions
run in a fixed order (deterministic); the values agree with torch's to float32 rounding of a
different summation order. An empty mask gives NaN, like torch's mean of nothing.
"""
from __future__ import annotations

import torch

from . import _lib
from .kernels import (ChamferDistance, MeshShapePriors, PointFaceDistances, PointMeshBatch, PointMeshFaceDistance,
                      PosedChamfer, _require_cuda, mesh_prior_topology)
from .structures import Meshes, Pointclouds


def _rgba_base(t: torch.Tensor, channels):
    """The dense float32 (..., 4) tensor `t` is the slice ``base[..., channels]`` of (a slice object
    or an int channel), or None."""
    b = t._base
    if b is None or b.dtype != torch.float32 or t.dtype != torch.float32 or b.dim() < 2 or b.shape[-1] != 4 \
            or not b.is_contiguous() or t.device != b.device:
        return None
    if isinstance(channels, int):
        ok = (tuple(t.shape) == tuple(b.shape[:-1]) and tuple(t.stride()) == tuple(b.stride()[:-1]) and
              t.storage_offset() == b.storage_offset() + channels)
    else:
        ok = (tuple(t.shape) == tuple(b.shape[:-1]) + (3,) and tuple(t.stride()) == tuple(b.stride()) and
              t.storage_offset() == b.storage_offset())
    return b if ok else None


def pose_loss(depth, silhouette, color, mask, depth_ref, rgb_ref, delta: float = 0.05, w_color: float = 0.01,
              return_terms: bool = False):
    """camera_pose_optimizer.py:257-276 calc_loss on the GPU. Returns the total loss (0-dim,
    differentiable w.r.t. depth, silhouette and color), or (total, (sil_loss, hloss, color_loss))
    with ``return_terms`` (the terms the reference logs; not differentiable)."""
    _require_cuda(depth, silhouette, color, mask, depth_ref, rgb_ref)
    sb = _rgba_base(silhouette, 3)
    cb = _rgba_base(color, slice(0, 3))
    # the autograd node is C++ (_mr_torch.pose_loss, csrc/mr_torch.cpp): forward and backward without Python
    total, terms = _lib.torch_ext().pose_loss(depth, silhouette if sb is None else sb, color if cb is None else cb,
                                              mask, depth_ref, rgb_ref, float(delta), float(w_color), sb is not None,
                                              cb is not None)
    if return_terms:
        return total, (terms[0], terms[1], terms[2])
    return total


def _mesh_priors(meshes, target_length: float, terms: int):
    """(edge, laplacian, normal) of `meshes`, computing the terms in the MR_PRIOR_* mask `terms`."""
    if meshes.isempty():  # upstream: a zero that requires grad
        dev = meshes.device if len(meshes) else torch.device("cpu")
        return tuple(torch.zeros(1, dtype=torch.float32, device=dev, requires_grad=True) for _ in range(3))
    if meshes.is_shared():
        # one mesh, or Meshes.extend(N): N equal meshes weighted 1/N each are the single mesh, and its
        # vertices take the gradient once
        verts, faces = meshes.shared_verts(), [meshes.shared_faces()]
        sizes = [verts.shape[0]]
    else:
        vl, faces = meshes.verts_list(), meshes.faces_list()
        sizes = [v.shape[0] for v in vl]
        verts = torch.cat(vl, 0)
    _require_cuda(verts, *faces)
    return MeshShapePriors.apply(verts, mesh_prior_topology(faces, sizes), float(target_length), terms)


def mesh_shape_priors(meshes, target_length: float = 0.0):
    """(mesh_edge_loss(meshes, target_length), mesh_laplacian_smoothing(meshes, "uniform"),
    mesh_normal_consistency(meshes)) from ONE autograd node and one forward pass: what a deformation loop's
    update_mesh_shape_prior_losses should call. Each is a 0-dim float32 tensor on the meshes' device,
    differentiable w.r.t. the vertex tensors of `meshes`."""
    return _mesh_priors(meshes, target_length, _lib.MR_PRIOR_ALL)


def mesh_edge_loss(meshes, target_length: float = 0.0):
    """pytorch3d.loss.mesh_edge_loss: per mesh the mean over its unique edges of (|v0 - v1| - target_length)^2,
    averaged over the meshes."""
    return _mesh_priors(meshes, target_length, _lib.MR_PRIOR_EDGE)[0]


def mesh_laplacian_smoothing(meshes, method: str = "uniform"):
    """pytorch3d.loss.mesh_laplacian_smoothing(method="uniform"): per mesh the mean over its vertices of
    |mean of the neighbours - v|, averaged over the meshes. The cotangent weightings are not built."""
    if method in ("cot", "cotcurv"):
        raise NotImplementedError(f"mesh_laplacian_smoothing: method {method!r} is not built (only 'uniform')")
    if method != "uniform":
        raise ValueError("Method should be one of {uniform, cot, cotcurv}")
    return _mesh_priors(meshes, 0.0, _lib.MR_PRIOR_LAPLACIAN)[1]


def mesh_normal_consistency(meshes):
    """pytorch3d.loss.mesh_normal_consistency: per mesh the mean over the pairs of faces sharing an edge of
    1 - cos(angle between their normals), averaged over the meshes (0 for a mesh without such pairs)."""
    return _mesh_priors(meshes, 0.0, _lib.MR_PRIOR_NORMAL)[2]


def _cloud_input(points, lengths, name):
    """(padded tensor, lengths) of a chamfer_distance input: a Pointclouds brings its own lengths (None when no cloud
    is padded, which is decided on the host)."""
    if isinstance(points, Pointclouds):
        if lengths is not None:
            raise ValueError(f"{name} must be None for a Pointclouds input: the lengths are the clouds'")
        padded = points.points_padded()
        full = all(c == padded.shape[1] for c in points.counts())
        return padded, None if full else points.num_points_per_cloud()
    if not torch.is_tensor(points):
        raise NotImplementedError("chamfer_distance: the inputs are (N, P, 3) tensors or Pointclouds")
    return points, lengths


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, weights=None,
                     batch_reduction="mean", point_reduction="mean", norm: int = 2, single_directional: bool = False):
    """pytorch3d.loss.chamfer_distance for (N,P,3) tensors or Pointclouds (whose lengths are then the clouds' own;
    explicit ``x_lengths`` / ``y_lengths`` beside a Pointclouds raise ValueError): per cloud the sum (``point_reduction="sum"``) or the mean
    over max(length, 1) points (``"mean"``) of every point's distance to its nearest point of the other cloud
    (squared L2 for ``norm=2``, L1 for ``norm=1``), x -> y plus y -> x (x -> y alone with ``single_directional``),
    times ``weights`` (N,); then summed over the batch (``batch_reduction="sum"``), divided by sum(weights) or N
    (``"mean"``), or left as (N,) (``None``). Returns ``(loss, None)``: normals are not built. Differentiable
    w.r.t. x and y (``weights`` is a constant); given lengths are checked on the host, otherwise nothing
    synchronises."""
    if x_normals is not None or y_normals is not None:
        raise NotImplementedError("chamfer_distance: normals are not built")
    if point_reduction is None:
        raise NotImplementedError("chamfer_distance: point_reduction=None is not built")
    if batch_reduction is not None and batch_reduction not in ("mean", "sum"):
        raise ValueError('batch_reduction must be one of ["mean", "sum"] or None')
    if point_reduction not in ("mean", "sum"):
        raise ValueError('point_reduction must be one of ["mean", "sum"] or None')
    if norm not in (1, 2):
        raise ValueError("Support for 1 or 2 norm.")
    x, x_lengths = _cloud_input(x, x_lengths, "x_lengths")
    y, y_lengths = _cloud_input(y, y_lengths, "y_lengths")
    if x.dim() != 3 or y.dim() != 3:
        raise ValueError("Expected points to be of shape (N, P, D)")
    if x.shape[2] != 3 or y.shape[2] != 3:
        raise NotImplementedError("chamfer_distance: only D = 3 is built")
    N = x.shape[0]
    if y.shape[0] != N:
        raise ValueError("y does not have the correct shape.")
    if weights is not None and tuple(weights.shape) != (N,):
        raise ValueError("weights must be of shape (N,).")
    for name, l, P in (("x_lengths", x_lengths, x.shape[1]), ("y_lengths", y_lengths, y.shape[1])):
        if l is None:
            continue
        if tuple(l.shape) != (N,):
            raise ValueError(f"{name} must be of shape (N,).")
        if N and (int(l.min()) < 0 or int(l.max()) > P):  # reads the lengths on the host
            raise ValueError(f"{name}: a length is outside [0, {P}]")
    _require_cuda(x, y, x_lengths, y_lengths, weights)
    flags = (_lib.MR_CHAMFER_POINT_MEAN if point_reduction == "mean" else 0) | \
        {None: 0, "mean": _lib.MR_CHAMFER_BATCH_MEAN, "sum": _lib.MR_CHAMFER_BATCH_SUM}[batch_reduction] | \
        (_lib.MR_CHAMFER_SINGLE if single_directional else 0)
    return ChamferDistance.apply(x, y, x_lengths, y_lengths, weights, flags, norm), None


def posed_chamfer_distance(x, y, R, T=None, s=None, *, norm: int = 2, point_reduction="mean",
                           single_directional: bool = False):
    """The chamfer distance of ONE source cloud ``x`` ((P1,3) or (1,P1,3)) to ONE target cloud ``y`` ((P2,3) or
    (1,P2,3)) under S pose hypotheses, as (S,) float32: entry k is
    ``chamfer_distance((s[k] * x[None] @ R[k] + T[k]), y[None], batch_reduction=None, norm=..., point_reduction=...,
    single_directional=...)[0]``, without the S copies of either cloud.

    ``R (S,3,3)`` (any strides), ``T (S,3)`` or ``(S,1,3)`` and the optional scale ``s (S,)`` follow the library's
    row-vector convention ``x' = s (x R) + T`` of ``SimilarityTransform`` and ``ICPSolution.RTs``; an ``(R, T, s)``
    triple may be passed in place of ``R``. The reference scripts' ``transform_pcd_tensors(pcds, ts, Rs)`` applies
    column-vector rotations ``Rs @ p``: pass ``R = Rs.transpose(1, 2)`` (and ``T = ts``).

    Differentiable w.r.t. ``R``, ``T`` and ``s`` (bitwise reproducible; through ``transforms.euler_angles_to_matrix``
    also w.r.t. Euler angles); the clouds are constants, and one that requires grad while grad mode is on raises
    NotImplementedError. The kernel is built for many poses of small clouds; a large cloud under a handful of poses
    is computed correctly but leaves most of the chip idle (materialise the clouds and call ``chamfer_distance``
    there: nothing routes automatically)."""
    if isinstance(R, (tuple, list)):
        if len(R) != 3 or T is not None or s is not None:
            raise ValueError("posed_chamfer_distance: pass either R, T[, s] or one (R, T, s) triple")
        R, T, s = R
    if T is None:
        raise ValueError("posed_chamfer_distance: T is missing")
    if norm not in (1, 2):
        raise ValueError("Support for 1 or 2 norm.")
    if point_reduction not in ("mean", "sum"):
        raise ValueError('point_reduction must be one of ["mean", "sum"]')
    for t in (x, y, R, T):
        if not torch.is_tensor(t):
            raise ValueError("posed_chamfer_distance: x, y, R and T are tensors")
    if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
        raise NotImplementedError("posed_chamfer_distance: not differentiable w.r.t. the clouds (x or y requires "
                                  "grad; detach them: the gradients go to R, T and s)")
    flags = (_lib.MR_CHAMFER_POINT_MEAN if point_reduction == "mean" else 0) | \
        (_lib.MR_CHAMFER_SINGLE if single_directional else 0)
    return PosedChamfer.apply(x, y, R, T, s, flags, norm)


def point_mesh_face_distance(meshes, pcls, min_triangle_area: float = 5e-3):
    """pytorch3d.loss.point_mesh_face_distance for a ``Meshes`` and a ``Pointclouds`` of equal batch size: per pair the
    mean over the cloud's points of the squared distance to the nearest face of its mesh, plus the mean over the
    mesh's faces of the squared distance to the nearest point of its cloud; then the mean over the batch. A pair
    whose cloud is empty or whose mesh has no faces contributes 0 and receives no gradient.

    The distance is upstream's: a face whose area is below ``min_triangle_area`` (default 5e-3, upstream's) counts as
    its three edges, not as a filled triangle; ``min_triangle_area=0`` gives the true point-to-triangle distance.
    Differentiable w.r.t. the points and the vertices (through ``offset_verts`` to a ``deform_verts`` leaf; the
    shared tensors of an ``extend``-ed batch receive the sum over their copies); bitwise reproducible; nothing
    synchronises."""
    if not isinstance(meshes, Meshes) or not isinstance(pcls, Pointclouds):
        raise ValueError("point_mesh_face_distance: the inputs are a Meshes and a Pointclouds")
    if len(meshes) != len(pcls):
        raise ValueError("meshes and pointclouds must be equal sized batches")
    if len(meshes) < 1:
        raise ValueError("point_mesh_face_distance: the batch is empty")
    points = pcls.points_packed()
    verts = meshes.verts_packed()
    if points.dim() != 2 or points.shape[1] != 3 or verts.shape[1] != 3:
        raise NotImplementedError("point_mesh_face_distance: only D = 3 is built")
    faces, faces_first, faces_count, max_faces = meshes._face_table()
    batch = PointMeshBatch(pcls.cloud_to_packed_first_idx(), pcls.num_points_per_cloud(), max(pcls.counts()), faces,
                           faces_first, faces_count, max_faces)
    return PointMeshFaceDistance.apply(points, verts, batch, float(min_triangle_area))


def _tris_batch(points, points_first_idx, tris, tris_first_idx, max_points, max_tris):
    """The PointMeshBatch of upstream's (points, points_first_idx, tris (T,3,3), tris_first_idx) arguments: the
    triangles' corners are the vertices, under a trivial face table; the counts follow from the first indices on the
    device."""
    if points.dim() != 2 or tris.dim() != 3 or tuple(tris.shape[1:]) != (3, points.shape[1]):
        raise ValueError("points must be (P, D) and tris (T, 3, D)")
    if points.shape[1] != 3:
        raise NotImplementedError("point-face distance: only D = 3 is built")
    if points_first_idx.dim() != 1 or points_first_idx.shape != tris_first_idx.shape:
        raise ValueError("points_first_idx and tris_first_idx must be (N,) tensors of one batch size")
    _require_cuda(points, tris, points_first_idx, tris_first_idx)
    P, T = points.shape[0], tris.shape[0]

    def count(first, total):
        first = first.to(torch.int64)
        return first, torch.cat((first[1:], first.new_full((1,), total))) - first

    pf, pc = count(points_first_idx, P)
    ff, fc = count(tris_first_idx, T)
    faces = torch.arange(3 * T, dtype=torch.int32, device=tris.device).view(T, 3)
    return PointMeshBatch(pf, pc, P if max_points is None else min(int(max_points), P), faces, ff, fc,
                          T if max_tris is None else min(int(max_tris), T))


def point_face_distance(points, points_first_idx, tris, tris_first_idx, max_points=None, min_triangle_area: float = 5e-3):
    """upstream's unreduced point_face_distance: (P,) squared distances from every point of the packed ``points`` (P,3)
    to the nearest of its own mesh's triangles ``tris`` (T,3,3); ``*_first_idx`` (N,) are the packed first indices,
    ``max_points`` a bound of the points per cloud. Differentiable w.r.t. points and tris."""
    batch = _tris_batch(points, points_first_idx, tris, tris_first_idx, max_points, None)
    return PointFaceDistances.apply(points, tris.reshape(-1, 3), batch, float(min_triangle_area), 0)[0]


def face_point_distance(points, points_first_idx, tris, tris_first_idx, max_tris=None, min_triangle_area: float = 5e-3):
    """upstream's unreduced face_point_distance: (T,) squared distances from every triangle of ``tris`` (T,3,3) to the
    nearest point of its own cloud. Differentiable w.r.t. points and tris."""
    batch = _tris_batch(points, points_first_idx, tris, tris_first_idx, None, max_tris)
    return PointFaceDistances.apply(points, tris.reshape(-1, 3), batch, float(min_triangle_area), 1)[0]
