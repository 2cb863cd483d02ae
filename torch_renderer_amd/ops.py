"""``pytorch3d.ops`` names: ``sample_points_from_meshes`` (mesh_deformer.py:299-352 and deform_mesh_from_pcd.py:
160-212 sample 1000 points of the target and of the deformed source every step).

The random draws are torch calls on the meshes' device — ``torch.multinomial`` over the padded per-mesh face areas
(with replacement) and ``torch.rand(2, N, S)`` — so ``torch.manual_seed`` reproduces a call. The face areas
(kernels.face_areas) and the construction of the points with its backward (kernels.SamplePoints) are native
(csrc/mr_points.hip).

``iterative_closest_point`` and ``corresponding_points_alignment`` (pytorch3d_icp_registeration.py:154-185,
pytorch3d_icp_evaluation.py) take (N, P, 3) tensors or ``Pointclouds``; the ICP loop, its nearest-neighbour search,
the Procrustes solve and the convergence test run on the device (kernels.icp / kernels.points_alignment, the
k_icp_* kernels of csrc/mr_points.hip). Neither is differentiable.

``iterative_closest_point_to_plane`` is a second, rigid estimator on that loop (kernels.icp_plane, k_icp_plane_*): the
same neighbour search, then a damped Gauss-Newton step on the point-to-plane residual against the target's normals,
given or estimated with ``estimate_pointcloud_normals``. Not differentiable.

``iterative_closest_point_to_mesh`` is a third: the clouds register onto mesh surfaces (kernels.icp_mesh,
csrc/mr_icpmesh.hip), the same Gauss-Newton step against the closest surface points and the distance function's
gradient there. Not differentiable.

``knn_points`` (K <= 32 nearest neighbours, csrc/mr_knn.hip; ``dists`` is differentiable) and ``knn_gather``.
``PointGrid`` (csrc/mr_grid.hip) is a uniform-grid index over the targets that ``knn_points(..., grid=)`` searches
instead of scanning every target, with the same result bit for bit. ``iterative_closest_point`` and
``iterative_closest_point_to_plane`` take one in place of ``Y`` and search it in every iteration (k_icp_nn_grid of
csrc/mr_points.hip), again with the same result bit for bit.

``ball_query`` (the first K neighbours inside a radius, any K, csrc/mr_ballquery.hip; ``dists`` is differentiable) and
``masked_gather``. ``ball_query(..., grid=PointGrid(p2))`` searches the index instead, K <= 64, bit for bit.

``sample_farthest_points`` (csrc/mr_fps.hip): one workgroup per cloud runs all K rounds on the device; the selected
points are differentiable w.r.t. the input points.

``estimate_pointcloud_normals`` and ``estimate_pointcloud_local_coord_frames`` (csrc/mr_normals.hip): the K <= 64
neighbourhood scan, the covariance and its 3x3 eigen solve in one launch. Not differentiable. Both take a
``PointGrid`` in place of the cloud and then search it (k_frames_grid), bit for bit.
"""
from __future__ import annotations

import inspect
import warnings
import weakref
from typing import NamedTuple, Optional

import torch

from . import _lib, kernels
from .kernels import SamplePoints, _require_cuda, face_areas
from .structures import Meshes, Pointclouds

_FACES_CACHE: dict = {}


class SimilarityTransform(NamedTuple):
    R: torch.Tensor
    T: torch.Tensor
    s: torch.Tensor


class ICPSolution(NamedTuple):
    converged: bool
    rmse: Optional[torch.Tensor]
    Xt: object
    RTs: SimilarityTransform
    t_history: list


def _clouds_and_lengths(pc, who):
    """(padded (N,P,D) tensor, host-side counts or None, lengths tensor or None) of a tensor or a Pointclouds."""
    if isinstance(pc, Pointclouds):
        counts = pc.counts()
        padded = pc.points_padded()
        if all(c == padded.shape[1] for c in counts):
            return padded, counts, None
        return padded, counts, pc.num_points_per_cloud()
    if not torch.is_tensor(pc):
        raise ValueError("The inputs X, Y should be either Pointclouds objects or tensors.")
    if pc.dim() != 3:
        raise ValueError(f"{who}: point sets must be (N, P, D) tensors or Pointclouds")
    return pc, None, None


def _icp_target(Y, who):
    """(padded (N,P2,D) tensor, host-side counts or None, lengths tensor or None, grid buffer or None) of an ICP
    target: a tensor or a Pointclouds as ``_clouds_and_lengths`` reads them, or a PointGrid, which stands for the
    points it was built from."""
    if isinstance(Y, PointGrid):
        padded, lengths, counts = Y.points()
        return padded, counts, None if Y.full else lengths, Y.buffer
    return (*_clouds_and_lengths(Y, who), None)


def _refuse_grad(who, *ts):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise NotImplementedError(f"{who}: not differentiable (an input requires grad; call it under torch.no_grad() "
                                  "or detach the inputs)")


def _split_rts(rts):
    return SimilarityTransform(rts[..., :9].reshape(*rts.shape[:-1], 3, 3), rts[..., 9:12], rts[..., 12])


def corresponding_points_alignment(X, Y, weights=None, estimate_scale: bool = False, allow_reflection: bool = False,
                                   eps: float = 1e-9):
    """pytorch3d.ops.corresponding_points_alignment: the similarity transform (R, T, s) minimising
    sum_i w_i |s X_i R + T - Y_i|^2 per cloud (Umeyama), for (N,P,3) tensors or Pointclouds of equal sizes
    (their lengths weigh the padding 0). Means, covariance and the 3x3 SVD are float64 on the device
    (kernels.points_alignment, csrc/mr_points.hip); the result is float32. Not differentiable."""
    Xt, xc, xl = _clouds_and_lengths(X, "corresponding_points_alignment")
    Yt, yc, _ = _clouds_and_lengths(Y, "corresponding_points_alignment")
    counts = xc if xc is not None else [Xt.shape[1]] * Xt.shape[0]
    if Xt.shape != Yt.shape or counts != (yc if yc is not None else [Yt.shape[1]] * Yt.shape[0]):
        raise ValueError("Point sets X and Y have to have the same number of batches, points and dimensions.")
    if weights is not None and tuple(weights.shape) != tuple(Xt.shape[:2]):
        raise ValueError("weights should have the same first two dimensions as X.")
    if Xt.shape[2] != 3:
        raise NotImplementedError("corresponding_points_alignment: only D = 3 is built")
    _refuse_grad("corresponding_points_alignment", Xt, Yt, weights)
    if any(c < 4 for c in counts):
        warnings.warn("The size of one of the point clouds is <= dim+1. "
                      "corresponding_points_alignment cannot return a unique rotation.")
    _require_cuda(Xt, Yt, weights)
    flags = (_lib.MR_ICP_ESTIMATE_SCALE if estimate_scale else 0) | \
        (_lib.MR_ICP_ALLOW_REFLECTION if allow_reflection else 0)
    return _split_rts(kernels.points_alignment(Xt, Yt, xl, weights, flags, eps))


def iterative_closest_point(X, Y, init_transform=None, max_iterations: int = 100, relative_rmse_thr: float = 1e-6,
                            estimate_scale: bool = False, allow_reflection: bool = False, verbose: bool = False):
    """pytorch3d.ops.iterative_closest_point for (N,P,3) tensors or Pointclouds (pytorch3d_icp_registeration.py:
    154-185): from ``Xt = s X R + T`` (``init_transform`` or the identity), repeat { nearest target of every Xt point;
    align the ORIGINAL X to those targets; rmse of the new Xt against them } until every cloud's relative rmse drop
    is <= ``relative_rmse_thr`` (``converged=True``) or ``max_iterations`` have run. Returns
    ``ICPSolution(converged, rmse (N,), Xt, RTs, t_history)``, ``len(t_history)`` being the iterations run.

    The loop runs on the device, four launches an iteration and no (N, P1, P2) matrix (kernels.icp, csrc/mr_points.hip);
    the host reads two status words every few iterations. Deterministic; not differentiable.

    ``Y`` may be a ``PointGrid`` built from the target points (a tensor with optional lengths, or a Pointclouds): every
    iteration then searches that index instead of scanning every target, and the solution is that of the call with the
    points, bit for bit. A grid whose tensor has been freed or modified in place since the build raises ValueError.
    Nothing routes automatically."""
    if verbose:
        raise NotImplementedError("iterative_closest_point: verbose=True is not built")
    Xt, xc, xl = _clouds_and_lengths(X, "iterative_closest_point")
    Yt, yc, yl, grid = _icp_target(Y, "iterative_closest_point")
    b, dim = Xt.shape[0], Xt.shape[2]
    if dim != Yt.shape[2] or b != Yt.shape[0]:
        raise ValueError("Point sets X and Y have to have the same number of batches and data dimensions.")
    if init_transform is not None:
        try:
            R, T, s = init_transform
            assert tuple(R.shape) == (b, dim, dim) and tuple(T.shape) == (b, dim) and tuple(s.shape) == (b,)
        except Exception:
            raise ValueError("The initial transformation init_transform has to be a named tuple SimilarityTransform "
                             "with elements (R, T, s). R are dim x dim orthonormal matrices of shape "
                             "(minibatch, dim, dim), T is a batch of dim-dimensional translations of shape "
                             "(minibatch, dim) and s is a batch of scalars of shape (minibatch,).") from None
    if dim != 3:
        raise NotImplementedError("iterative_closest_point: only D = 3 is built")
    _refuse_grad("iterative_closest_point", Xt, Yt, *(init_transform or ()))
    if yc is not None and any(cy == 0 and cx > 0 for cx, cy in zip(xc or [Xt.shape[1]] * b, yc)):
        raise ValueError("iterative_closest_point: a target cloud is empty where its source is not")
    _require_cuda(Xt, Yt, *(init_transform or ()))
    flags = (_lib.MR_ICP_ESTIMATE_SCALE if estimate_scale else 0) | \
        (_lib.MR_ICP_ALLOW_REFLECTION if allow_reflection else 0)
    converged, iters, rmse, xt, rts, hist = kernels.icp(Xt, Yt, xl, yl, init_transform, max_iterations,
                                                        relative_rmse_thr, flags, grid=grid)
    if isinstance(X, Pointclouds):
        xt = X.update_padded(xt)
    return ICPSolution(converged, rmse, xt, _split_rts(rts), [_split_rts(hist[i]) for i in range(iters)])


def iterative_closest_point_to_plane(X, Y, Y_normals=None, init_transform=None, max_iterations: int = 100,
                                     relative_rmse_thr: float = 1e-6, max_correspondence_distance=None,
                                     neighborhood_size: int = 50):
    """Point-to-plane ICP of X onto Y, (N,P,3) tensors or Pointclouds handled as in ``iterative_closest_point``: a
    rigid Gauss-Newton estimator on the same device-side loop (a convention of this library; upstream has none).
    Returns ``ICPSolution(converged, rmse (N,), Xt, RTs, t_history)``; ``rmse`` is the point-to-plane rmse below.

    ``Y_normals`` (N,P2,3), Y's padded shape, is read as float32 and used as given: a zero normal contributes nothing
    and a normal's sign does not matter. ``None`` computes ``estimate_pointcloud_normals(Y, neighborhood_size)``,
    whose errors propagate (every target cloud needs more than ``neighborhood_size`` points); ``neighborhood_size`` is
    ignored otherwise. ``init_transform`` is an (R, T, s) triple whose ``s`` stays fixed. With
    ``max_correspondence_distance`` d (None, or a finite float > 0) a pair is valid iff its float32 squared distance
    is <= r2 = float32(d) * float32(d); without, every pair is valid.

    Per cloud, with L1 and L2 its lengths and (R, T, s) float32, every iteration:

    1. p_i = s (x_i R) + T in float32 for i < L1; j(i) is the nearest target j < L2 by the float32 squared distance
       (dx*dx + dy*dy) + dz*dz, ties to the lowest index; m counts the valid pairs.
    2. In float64 and a fixed order: c = s (mx R) + T with mx the mean of the cloud's source points; per valid pair
       with q = y_j and n = Y_normals_j: r = (p - q).n and J = [(p - c) x n, n]; A = sum J J^T, b = sum J r.
    3. xi = (w, t) solves (A + lam I) xi = -b, lam = 1e-9 trace(A) / 6, by a 6x6 Cholesky in float64 (xi = 0 if
       trace(A) is 0 or m is 0); E = exp([w]x) by Rodrigues in float64.
    4. R <- R E^T, T <- (T - c) E^T + c + t in the row-vector convention, s unchanged; formed in float64 from the
       float32 values and rounded once to float32.
    5. rmse = float32(sqrt(sum_valid ((p'_i - q_i).n_i)^2 / max(m, 1))), p' under the new transform, with this
       iteration's correspondences and validity.
    6. rel = (prev - rmse) / prev in float32, 1 on the first iteration; a cloud is done when
       rel <= ``relative_rmse_thr`` (a NaN does not pass). A cloud with m == 0 keeps its transform, reports rmse 0
       and counts as done. ``converged``: every cloud is done in the same iteration.

    Four launches an iteration, no (N, P1, P2) matrix, the host reads two status words every few iterations
    (kernels.icp_plane, the k_icp_plane_* kernels of csrc/mr_points.hip). Rigid only, normals as given, a brute-force
    neighbour scan, deterministic, not differentiable.

    ``Y`` may be a ``PointGrid`` built from the target points, as in ``iterative_closest_point``: step 1 then searches
    that index, and with ``max_correspondence_distance`` a source point's search ends where no unvisited cell can hold
    a target within d. The solution is that of the call with the points, bit for bit; ``Y_normals`` has the padded
    shape of the grid's points, and ``None`` estimates them from those points through the same grid (k_frames_grid),
    bit for bit the normals of ``estimate_pointcloud_normals``."""
    who = "iterative_closest_point_to_plane"
    Xt, xc, xl = _clouds_and_lengths(X, who)
    Yt, yc, yl, grid = _icp_target(Y, who)
    b, dim = Xt.shape[0], Xt.shape[2]
    if dim != Yt.shape[2] or b != Yt.shape[0]:
        raise ValueError("Point sets X and Y have to have the same number of batches and data dimensions.")
    if init_transform is not None:
        try:
            R, T, s = init_transform
            assert tuple(R.shape) == (b, dim, dim) and tuple(T.shape) == (b, dim) and tuple(s.shape) == (b,)
        except Exception:
            raise ValueError("The initial transformation init_transform has to be a named tuple SimilarityTransform "
                             "with elements (R, T, s). R are dim x dim orthonormal matrices of shape "
                             "(minibatch, dim, dim), T is a batch of dim-dimensional translations of shape "
                             "(minibatch, dim) and s is a batch of scalars of shape (minibatch,).") from None
    if max_correspondence_distance is not None:
        try:
            d = float(max_correspondence_distance)
        except (TypeError, ValueError):
            d = float("nan")
        if isinstance(max_correspondence_distance, bool) or not (0.0 < d < float("inf")):
            raise ValueError(f"{who}: max_correspondence_distance must be None or a finite float > 0")
        max_correspondence_distance = d
    if dim != 3:
        raise NotImplementedError(f"{who}: only D = 3 is built")
    if Y_normals is not None and (not torch.is_tensor(Y_normals) or tuple(Y_normals.shape) != tuple(Yt.shape)):
        raise ValueError(f"{who}: Y_normals must be a tensor of Y's padded shape {tuple(Yt.shape)}")
    _refuse_grad(who, Xt, Yt, Y_normals, *(init_transform or ()))
    if yc is not None and any(cy == 0 and cx > 0 for cx, cy in zip(xc or [Xt.shape[1]] * b, yc)):
        raise ValueError(f"{who}: a target cloud is empty where its source is not")
    if Y_normals is None:
        with torch.no_grad():
            Y_normals = estimate_pointcloud_normals(Y, neighborhood_size) if grid is None else \
                _local_frames(Yt, yl, yc, neighborhood_size, True, grid)[1][..., 0]
    _require_cuda(Xt, Yt, Y_normals, *(init_transform or ()))
    converged, iters, rmse, xt, rts, hist = kernels.icp_plane(Xt, Yt, Y_normals, xl, yl, init_transform,
                                                              max_iterations, relative_rmse_thr,
                                                              max_correspondence_distance, grid=grid)
    if isinstance(X, Pointclouds):
        xt = X.update_padded(xt)
    return ICPSolution(converged, rmse, xt, _split_rts(rts), [_split_rts(hist[i]) for i in range(iters)])


def iterative_closest_point_to_mesh(X, meshes, init_transform=None, max_iterations: int = 100,
                                    relative_rmse_thr: float = 1e-6, max_correspondence_distance=None,
                                    min_triangle_area: float = 0.0, verbose: bool = False):
    """ICP of the clouds X, an (N,P,3) tensor or a Pointclouds, onto the surfaces of the N ``meshes`` (a Meshes; cloud n
    registers onto mesh n): a rigid Gauss-Newton estimator on the device-side loop of ``iterative_closest_point`` (a
    convention of this library; upstream has none). The scan is the moving cloud and the target the surface itself:
    every point has a counterpart on a complete model and there is no sampling-density floor. Returns
    ``ICPSolution(converged, rmse (N,), Xt, RTs, t_history)``; ``rmse`` is the point-to-plane rmse below.

    ``meshes`` may be a ``Meshes.extend(N)`` batch, whose one copy of vertices and faces every cloud then reads.
    ``min_triangle_area`` defaults to 0, the true surface, not upstream's 5e-3 of ``point_mesh_face_distance`` (a loss
    setting, under which a face below that area counts as its three edges). ``init_transform`` is an (R, T, s) triple
    whose ``s`` stays fixed. With ``max_correspondence_distance`` d (None, or a float >= 0) a pair is valid iff its
    float32 squared distance is <= float32(d)^2 rounded once; without, every pair is valid.

    Per cloud n with L1 points, mesh n with T_n faces and (R, T, s) float32, every iteration:

    1. Search. p_i = s (x_i R) + T in float32 for i < L1; f(i) is the face of mesh n with the smallest d(p_i, tri), d
       exactly ``point_face_distance``'s float32 distance for ``min_triangle_area``. The lowest face index wins a tie;
       a face with a vertex id out of range is skipped.
    2. Closest point and normal, in float32 without FMA, from the winner's pair: q_i = (b0 v0 + b1 v1) + b2 v2 per
       component with the closest point's barycentrics b. n_i is the triangle's unit normal if the plane branch
       returned the distance; otherwise e = p_i - q_i, l = sqrt((e0 e0 + e1 e1) + e2 e2) and n_i = e / l if l > 1e-8,
       else 0. That is the gradient of the distance function: where the closest point lies on an edge or vertex
       shared by several faces, it does not depend on which of the tied faces won. A zero normal contributes nothing
       and the sign does not matter. A pair is valid iff d <= the squared distance limit; m counts the valid pairs.
    3. Update. Steps 2 to 6 of ``iterative_closest_point_to_plane``, unchanged, with q_i and n_i in place of y_j and
       Y_normals_j: float64 A and b about c = s (mx R) + T; lam = 1e-9 trace(A) / 6; the 6x6 Cholesky and Rodrigues;
       one rounding to float32; rmse = float32(sqrt(sum_valid ((p'_i - q_i).n_i)^2 / max(m, 1))) under the new
       transform; rel = (prev - rmse) / prev in float32, 1 on the first iteration, and a cloud is done when
       rel <= ``relative_rmse_thr``. A cloud with m == 0 (an empty cloud, a mesh with no usable face, no pair within
       the distance) keeps its transform bit for bit, reports rmse 0 and counts as done.

    Four launches an iteration, no (P, T) matrix, the host reads two status words every few iterations (kernels.icp_mesh,
    csrc/mr_icpmesh.hip); the triangle records are built once per call. Rigid only, a brute-force scan of every face,
    the mesh fixed during the call, deterministic, not differentiable, no CPU fallback."""
    who = "iterative_closest_point_to_mesh"
    if verbose:
        raise NotImplementedError(f"{who}: verbose=True is not built")
    if not isinstance(meshes, Meshes):
        raise ValueError(f"{who}: meshes must be a Meshes")
    Xt, xc, xl = _clouds_and_lengths(X, who)
    b, dim = Xt.shape[0], Xt.shape[2]
    if b != len(meshes):
        raise ValueError("meshes and pointclouds must be equal sized batches")
    if b < 1:
        raise ValueError(f"{who}: the batch is empty")
    if init_transform is not None:
        try:
            R, T, s = init_transform
            assert tuple(R.shape) == (b, dim, dim) and tuple(T.shape) == (b, dim) and tuple(s.shape) == (b,)
        except Exception:
            raise ValueError("The initial transformation init_transform has to be a named tuple SimilarityTransform "
                             "with elements (R, T, s). R are dim x dim orthonormal matrices of shape "
                             "(minibatch, dim, dim), T is a batch of dim-dimensional translations of shape "
                             "(minibatch, dim) and s is a batch of scalars of shape (minibatch,).") from None

    def nonneg(v, name):
        try:
            f = float(v)
        except (TypeError, ValueError):
            f = float("nan")
        if isinstance(v, bool) or not f >= 0.0:
            raise ValueError(f"{who}: {name} must be a float >= 0")
        return f

    if max_correspondence_distance is not None:
        max_correspondence_distance = nonneg(max_correspondence_distance, "max_correspondence_distance")
    min_triangle_area = nonneg(min_triangle_area, "min_triangle_area")
    if dim != 3:
        raise NotImplementedError(f"{who}: only D = 3 is built")
    if meshes.is_shared():  # one copy of the vertices and faces: every cloud's range is the whole table
        verts = meshes.shared_verts()
        faces, first, count, max_faces = kernels.mesh_face_table([meshes.shared_faces()], (verts.shape[0],))
        first, count = first.expand(b).contiguous(), count.expand(b).contiguous()
    else:
        verts = meshes.verts_packed()
        faces, first, count, max_faces = meshes._face_table()
    _refuse_grad(who, Xt, verts, *(init_transform or ()))
    _require_cuda(Xt, verts, *(init_transform or ()))
    batch = kernels.PointMeshBatch(None, xl, Xt.shape[1], faces, first, count, max_faces)
    converged, iters, rmse, xt, rts, hist = kernels.icp_mesh(Xt, verts, batch, xl, init_transform, max_iterations,
                                                             relative_rmse_thr, max_correspondence_distance,
                                                             min_triangle_area)
    if isinstance(X, Pointclouds):
        xt = X.update_padded(xt)
    return ICPSolution(converged, rmse, xt, _split_rts(rts), [_split_rts(hist[i]) for i in range(iters)])


def _packed_faces(faces_list, Vs):
    """(faces int32 (F,3) over packed vertex ids, per-mesh face counts) of the meshes, checked once against their
    vertex counts on the host and cached on the identity and version of the faces tensors (a steady loop, whose
    Meshes.offset_verts result keeps the source's faces tensors, does no host work here)."""
    key = tuple(id(f) for f in faces_list) + tuple(Vs)
    hit = _FACES_CACHE.get(key)
    if hit is not None and all(r() is f and ver == f._version for r, ver, f in zip(hit[0], hit[1], faces_list)):
        return hit[2]
    out, off = [], 0
    for f, V in zip(faces_list, Vs):
        if f.numel() and (int(f.min()) < 0 or int(f.max()) >= V):
            raise ValueError("sample_points_from_meshes: faces index vertices outside the mesh")
        out.append(f.reshape(-1, 3).to(torch.int32) + off)
        off += V
    if off >= 2 ** 31 // 3:
        raise NotImplementedError("sample_points_from_meshes: the packed batch is too large for 32-bit vertex ids")
    res = (torch.cat(out, 0).contiguous(), [int(f.shape[0]) for f in faces_list])
    if len(_FACES_CACHE) > 64:
        _FACES_CACHE.clear()
    _FACES_CACHE[key] = ([weakref.ref(f) for f in faces_list], [f._version for f in faces_list], res)
    return res


def sample_points_from_meshes(meshes, num_samples: int = 10000, return_normals: bool = False,
                              return_textures: bool = False):
    """pytorch3d.ops.sample_points_from_meshes: (N, num_samples, 3) points drawn uniformly from the surface of each
    mesh (a face in proportion to its area, then uniformly inside it); zeros for a mesh without faces.
    Differentiable w.r.t. the meshes' vertex tensors; a ``Meshes.extend(N)`` batch draws independently per copy and
    its shared vertices take the summed gradient once. Normals and textures are not built."""
    if return_normals or return_textures:
        raise NotImplementedError("sample_points_from_meshes: return_normals / return_textures are not built")
    if meshes.isempty():
        raise ValueError("Meshes are empty.")
    N, S = len(meshes), int(num_samples)
    if meshes.is_shared():  # one copy of the vertices: every mesh of the batch indexes it
        verts = meshes.shared_verts()
        faces, counts = _packed_faces([meshes.shared_faces()], (verts.shape[0],))
        counts, first = counts * N, [0] * N
    else:
        vl = meshes.verts_list()
        verts = torch.cat(vl, 0)
        faces, counts = _packed_faces(meshes.faces_list(), tuple(v.shape[0] for v in vl))
        first = [sum(counts[:i]) for i in range(N)]
    _require_cuda(verts, faces)
    dev = verts.device
    with torch.no_grad():
        areas = face_areas(verts, faces)
        if meshes.is_shared():
            face_idx = torch.multinomial(areas.view(1, -1).expand(N, -1), S, replacement=True)
        elif all(c == counts[0] for c in counts):
            face_idx = torch.multinomial(areas.view(N, -1), S, replacement=True) + \
                torch.tensor(first, device=dev).view(N, 1)
        else:  # padded areas of the meshes that have faces; the others keep the id -1 (rows of zeros)
            valid = [i for i, c in enumerate(counts) if c > 0]
            padded = torch.zeros((len(valid), max(counts)), device=dev)
            for r, i in enumerate(valid):
                padded[r, :counts[i]] = areas[first[i]:first[i] + counts[i]]
            drawn = torch.multinomial(padded, S, replacement=True) + \
                torch.tensor([first[i] for i in valid], device=dev).view(-1, 1)
            if len(valid) == N:
                face_idx = drawn
            else:
                face_idx = torch.full((N, S), -1, dtype=torch.int64, device=dev)
                face_idx[torch.tensor(valid, device=dev)] = drawn
        uv = torch.rand(2, N, S, device=dev)
    return SamplePoints.apply(verts, faces, face_idx, uv)


class _KNN(NamedTuple):
    dists: torch.Tensor
    idx: torch.Tensor
    knn: Optional[torch.Tensor]


def knn_gather(x, idx, lengths=None):
    """x (N,M,U) gathered at idx (N,L,K): (N,L,K,U), out[n,l,k] = x[n, idx[n,l,k]] (a torch gather: differentiable
    w.r.t. x). With ``lengths`` (N,), entries k >= lengths[n] are zero (knn_points pads their idx with 0)."""
    N, M, U = x.shape
    _N, L, K = idx.shape
    if N != _N:
        raise ValueError("x and idx must have same batch dimension.")
    if lengths is not None and tuple(lengths.shape) != (N,):
        raise ValueError("lengths must be of shape (N,)")
    out = x[:, :, None].expand(-1, -1, K, -1).gather(1, idx.long()[..., None].expand(-1, -1, -1, U))
    if lengths is None and M >= K:
        return out
    # nothing is read back from the device: the mask is applied whether or not a length is below K
    lengths = torch.full((N,), M, device=x.device) if lengths is None else lengths.to(x.device)
    pad = torch.arange(K, device=x.device)[None, :] >= lengths[:, None]  # (N,K)
    return out.masked_fill(pad[:, None, :, None].expand(-1, L, -1, U), 0.0)


class PointGrid:
    """A uniform-grid index over the clouds ``points`` (an (N,P,3) tensor with optional ``lengths`` (N,), or a
    ``Pointclouds``, which brings its own lengths), for ``knn_points(p1, points, lengths2=lengths, grid=...)`` and
    ``ball_query(..., grid=...)``, in place of ``Y`` for ``iterative_closest_point`` and
    ``iterative_closest_point_to_plane``, and in place of the cloud for ``estimate_pointcloud_normals`` and
    ``estimate_pointcloud_local_coord_frames``. Built on
    the device in four launches (kernels.point_grid_build, csrc/mr_grid.hip); with a tensor nothing synchronises, and
    build plus search capture into a HIP graph. It holds no gradient and keeps a copy of the coordinates, so it
    remembers what it was built from — the tensor's identity, ``_version`` and shape, and the lengths — and
    ``knn_points`` refuses it for anything else: rebuild it whenever the points change. One grid per cloud, single
    level: a far outlier stretches the box and the search degrades towards the brute-force scan (still correct)."""

    def __init__(self, points, lengths=None):
        self._remember(points, lengths)
        self.buffer = kernels.point_grid_build(self._ref(), self.lengths)

    def _remember(self, points, lengths):
        """What the grid is built from (host only): the padded tensor, by weak reference, with its version and shape;
        the lengths tensor; whether every cloud is known on the host to be full (a call without lengths2 then fits)."""
        self.full = lengths is None
        self._counts = None
        if isinstance(points, Pointclouds):
            if lengths is not None:
                raise ValueError("PointGrid: a Pointclouds brings its own lengths")
            cloud, points = points, points.points_padded()
            self._counts = cloud.counts()
            self.full = all(c == points.shape[1] for c in self._counts)
            lengths = cloud.num_points_per_cloud()
        if not torch.is_tensor(points) or points.dim() != 3:
            raise ValueError("PointGrid: points must be an (N, P, 3) tensor or a Pointclouds")
        if lengths is not None and (not torch.is_tensor(lengths) or tuple(lengths.shape) != (points.shape[0],)):
            raise ValueError("lengths must be of shape (N,)")
        self._ref, self._version, self.shape = weakref.ref(points), points._version, tuple(points.shape)
        self.lengths = lengths
        self._lengths_version = None if lengths is None else lengths._version

    def _check(self, p2, lengths2, who="knn_points"):
        """ValueError unless the grid was built from this p2 (not modified since) with these lengths2."""
        if self._ref() is not p2 or p2._version != self._version or tuple(p2.shape) != self.shape:
            raise ValueError(f"{who}: the grid was not built from this p2 (another tensor, or modified in place "
                             "since); rebuild it with PointGrid(p2, lengths2)")
        if lengths2 is None:
            same = self.lengths is None or self.full
        else:
            same = lengths2 is self.lengths and lengths2._version == self._lengths_version
        if not same:
            raise ValueError(f"{who}: the grid was not built with these lengths2; rebuild it with "
                             "PointGrid(p2, lengths2)")

    def points(self):
        """(padded (N,P,3) tensor, lengths (N,) or None, host-side counts or None) the grid was built from; the counts
        where a ``Pointclouds`` supplied them. ValueError if the tensor has been freed, or it or the lengths were
        modified in place since the build."""
        p = self._ref()
        if p is None:
            raise ValueError("PointGrid: the tensor the grid was built from has been freed; rebuild the grid")
        stale = p._version != self._version or tuple(p.shape) != self.shape
        if stale or (self.lengths is not None and self.lengths._version != self._lengths_version):
            raise ValueError("PointGrid: the points or lengths the grid was built from were modified in place since; "
                             "rebuild the grid")
        return p, self.lengths, None if self._counts is None else list(self._counts)

    def describe(self):
        """(dims (N,3) int32, origin_cell (N,4) = lo xyz and the cell size, max_cell_count (N,) int32) on the host.
        Synchronises: for tests and tools."""
        return kernels.point_grid_describe(self.buffer, self.shape[0], self.shape[1])


def knn_points(p1, p2, lengths1=None, lengths2=None, norm: int = 2, K: int = 1, version: int = -1,
               return_nn: bool = False, return_sorted: bool = True, grid: Optional[PointGrid] = None):
    """``pytorch3d.ops.knn_points``: for every point of p1 (N,P1,3) its K <= 32 nearest points of p2 (N,P2,3), as a
    namedtuple (dists (N,P1,K), idx (N,P1,K) int64, knn (N,P1,K,3) or None). dists is the squared L2 (norm 2) or L1
    (norm 1) distance in float32, ascending; equal distances take the lower index. Entries past min(K, lengths2[n])
    and rows past lengths1[n] are padded with 0 in both. The output is always sorted (a valid answer for
    ``return_sorted=False``); ``version`` is accepted and ignored. dists is differentiable w.r.t. p1 and p2
    (kernels.KnnPoints, csrc/mr_knn.hip), knn through the gather.

    ``grid=PointGrid(p2, lengths2)`` runs the search through that index instead of the brute-force scan
    (kernels.KnnPointsGrid, csrc/mr_grid.hip): the same dists, idx and knn bit for bit and the same backward. A grid
    that was not built from this p2 (the same tensor, not modified in place since) with these lengths2 raises
    ValueError. Without it the call is the brute-force kernel; nothing routes automatically."""
    if p1.dim() != 3 or p2.dim() != 3:
        raise ValueError("pts1 and pts2 must be (N, P, D) tensors.")
    if p1.shape[0] != p2.shape[0]:
        raise ValueError("pts1 and pts2 must have the same batch dimension.")
    if p1.shape[2] != p2.shape[2]:
        raise ValueError("pts1 and pts2 must have the same point dimension.")
    if norm not in (1, 2):
        raise ValueError("Support for 1 or 2 norm.")
    for l in (lengths1, lengths2):
        if l is not None and tuple(l.shape) != (p1.shape[0],):
            raise ValueError("lengths must be of shape (N,)")
    if grid is None:
        dists, idx = kernels.KnnPoints.apply(p1, p2, lengths1, lengths2, K, norm)
    else:
        if not isinstance(grid, PointGrid):
            raise ValueError("knn_points: grid must be a PointGrid or None")
        grid._check(p2, lengths2)
        dists, idx = kernels.KnnPointsGrid.apply(p1, p2, lengths1, lengths2, K, norm, grid.buffer)
    dists = dists.to(p1.dtype)
    idx = idx.clamp(min=0).long()
    return _KNN(dists=dists, idx=idx, knn=knn_gather(p2, idx, lengths2) if return_nn else None)


def masked_gather(points, idx):
    """``pytorch3d.ops.utils.masked_gather``: points (N,P,U) gathered at idx (N,L,K) -> (N,L,K,U), or at idx (N,L) ->
    (N,L,U), with zeros wherever idx < 0 (ball_query's padding). Differentiable w.r.t. points. The indices are
    clamped before torch's gather, so a -1 never reaches it, and nothing is read back from the device."""
    if points.dim() != 3 or idx.dim() not in (2, 3):
        raise ValueError("masked_gather: points must be (N, P, U) and idx (N, L, K) or (N, L)")
    if points.shape[0] != idx.shape[0]:
        raise ValueError("points and idx must have the same batch dimension")
    U = points.shape[2]
    pad = idx < 0
    safe = idx.clamp(min=0).long()
    if idx.dim() == 2:
        out = points.gather(1, safe[..., None].expand(-1, -1, U))
    else:
        out = points[:, :, None].expand(-1, -1, idx.shape[2], -1).gather(1, safe[..., None].expand(-1, -1, -1, U))
    return out.masked_fill(pad[..., None], 0.0)


def ball_query(p1, p2, lengths1=None, lengths2=None, K: int = 500, radius: float = 0.2, return_nn: bool = True, *,
               grid: Optional[PointGrid] = None):
    """``pytorch3d.ops.ball_query``: for every point of p1 (N,P1,3) the first K points of p2 (N,P2,3), in index order,
    that lie inside ``radius``, as a namedtuple (dists (N,P1,K), idx (N,P1,K) int64, knn (N,P1,K,3) or None).

    For query i of cloud n, with L1 = lengths1[n] (or P1), L2 = lengths2[n] (or P2) and r2 = float32(radius)^2 rounded
    once to float32: j = 0 .. L2 - 1 are walked in index order and every j whose float32 squared distance
    (dx*dx + dy*dy) + dz*dz is < r2 (strict) takes the next free slot until K are full. The result is the first K in
    index order, not the K nearest, and is not sorted by distance; dists holds the hits' squared distances. Free slots
    and rows i >= L1 are idx = -1, dists = 0, knn = 0 (knn_points pads idx with 0 instead). radius 0 hits nothing, a
    nan coordinate never hits; a negative or non-finite radius raises ValueError. Coordinates are read as float32;
    dists and knn come back in p1's dtype. Any K >= 1.

    dists is differentiable w.r.t. p1 and p2 (kernels.BallQuery, csrc/mr_ballquery.hip), knn through masked_gather.
    Nothing synchronises; forward and backward capture into a HIP graph.

    ``grid=PointGrid(p2, lengths2)`` runs the search through that index instead of the scan over every target
    (kernels.BallQueryGrid, k_ball_query_grid of csrc/mr_ballquery.hip), for K <= 64 (``NotImplementedError`` above,
    the default K = 500 included): the same dists, idx and knn bit for bit and the same backward. A query walks only
    the cells that can hold a point inside ``radius``, so a small radius in a large cloud is where it pays; a radius
    of the cloud's size visits every target from one lane and loses to the scan. A grid that was not built from this
    p2 (the same tensor, not modified in place since) with these lengths2 raises ValueError. Without it the call is
    the brute-force kernel; nothing routes automatically."""
    if p1.dim() != 3 or p2.dim() != 3:
        raise ValueError("p1 and p2 must be (N, P, D) tensors.")
    if p1.shape[0] != p2.shape[0]:
        raise ValueError("p1 and p2 must have the same batch dimension.")
    if p1.shape[2] != p2.shape[2]:
        raise ValueError("p1 and p2 must have the same point dimension.")
    for l in (lengths1, lengths2):
        if l is not None and tuple(l.shape) != (p1.shape[0],):
            raise ValueError("lengths must be of shape (N,)")
    if grid is None:
        dists, idx = kernels.BallQuery.apply(p1, p2, lengths1, lengths2, K, radius)
    else:
        if not isinstance(grid, PointGrid):
            raise ValueError("ball_query: grid must be a PointGrid or None")
        grid._check(p2, lengths2, "ball_query")
        dists, idx = kernels.BallQueryGrid.apply(p1, p2, lengths1, lengths2, K, radius, grid.buffer)
    idx = idx.long()
    return _KNN(dists=dists.to(p1.dtype), idx=idx, knn=masked_gather(p2, idx).to(p1.dtype) if return_nn else None)


# ``grid`` is this library's keyword-only extension: introspection keeps reporting pytorch3d's own parameter list,
# which tests/test_ball_query_cpu.py holds the wrapper to.
ball_query.__signature__ = inspect.Signature(
    [p for p in inspect.signature(ball_query).parameters.values() if p.name != "grid"])


def sample_farthest_points(points, lengths=None, K=50, random_start_point: bool = False):
    """``pytorch3d.ops.sample_farthest_points``: (selected_points (N,Kmax,3) in ``points``' dtype, selected_idx
    (N,Kmax) int64) of an (N,P,3) tensor with optional ``lengths`` (N,), or of a ``Pointclouds`` (whose lengths are
    then the clouds' own; an explicit ``lengths`` beside it raises ValueError). ``K`` is an int, a list of N ints or an
    (N,) integer tensor, and Kmax = max(K).

    Per cloud n, with L = lengths[n] and k_n = min(K[n], L): the first index is 0, or with ``random_start_point`` a
    draw in [0, L) made on the device from torch's generator (``torch.manual_seed`` reproduces it; the draws are not
    upstream's). Every point p < L carries m[p] = +inf; after each selection s, m[p] = min(m[p], |p - s|^2) in
    float32 with the operation order (dx*dx + dy*dy) + dz*dz, and the next index is the p < L with the largest m[p],
    the lowest index among equal values. A selected point stays in the running with m = 0, so a cloud with fewer
    distinct points than k_n re-selects its lowest duplicate. Slots k >= k_n are -1 in selected_idx and 0 in
    selected_points; Kmax == 0 gives empty tensors. Coordinates are read as float32 (a float64 input is rounded).

    selected_points is differentiable w.r.t. ``points`` (kernels.FarthestPoints); selected_idx is not. Given lengths
    are checked on the host, and a device tensor ``K`` costs one host read for Kmax; with an int ``K``, no
    ``lengths`` and no ``random_start_point`` nothing synchronises and the call captures into a HIP graph. One
    workgroup owns a cloud for all of its rounds: a batch of fewer clouds than the chip has compute units leaves the
    rest idle, and a cloud above 32,768 points is streamed from global memory every round, which is correct and slow
    (kernels.farthest_geometry tells)."""
    if isinstance(points, Pointclouds):
        if lengths is not None:
            raise ValueError("lengths must be None for a Pointclouds input: the lengths are the clouds'")
        padded = points.points_padded()
        if not all(c == padded.shape[1] for c in points.counts()):
            lengths = points.num_points_per_cloud()
        points = padded
    elif not torch.is_tensor(points):
        raise ValueError("sample_farthest_points: points is an (N, P, 3) tensor or a Pointclouds")
    if points.dim() != 3:
        raise ValueError("sample_farthest_points: points must be an (N, P, D) tensor")
    N, P, D = points.shape
    if lengths is not None:
        if tuple(lengths.shape) != (N,):
            raise ValueError("points and lengths must have same batch dimension.")
        if N and int(lengths.max()) > P:  # reads the lengths on the host
            raise ValueError("A value in lengths was too large.")
        if N and int(lengths.min()) < 0:
            raise ValueError("sample_farthest_points: a value in lengths is negative")
    if torch.is_tensor(K):
        if tuple(K.shape) != (N,):
            raise ValueError("K and points must have the same batch dimension")
        if K.dtype.is_floating_point or K.dtype == torch.bool:
            raise ValueError("sample_farthest_points: a tensor K must hold integers")
        kmin, Kmax = (int(K.min()), int(K.max())) if N else (0, 0)  # the host read of a device K
    elif isinstance(K, (list, tuple)):
        if len(K) != N:
            raise ValueError("K and points must have the same batch dimension")
        kmin, Kmax = (min(int(k) for k in K), max(int(k) for k in K)) if N else (0, 0)
    else:
        kmin = Kmax = int(K)
    if kmin < 0:
        raise ValueError("sample_farthest_points: K must be >= 0")
    if D != 3:
        raise NotImplementedError("sample_farthest_points: only D = 3 is built")
    _require_cuda(points, lengths)
    dev = points.device
    if N == 0 or P == 0 or Kmax == 0:
        return points.new_zeros((N, Kmax, 3)), torch.full((N, Kmax), -1, dtype=torch.int64, device=dev)
    if isinstance(K, (list, tuple)):
        K = torch.tensor([int(k) for k in K], dtype=torch.int64, device=dev)
    elif torch.is_tensor(K):
        K = K.to(dev)  # a host tensor K is as good as a list
    else:
        K = Kmax
    start = None
    if random_start_point:
        with torch.no_grad():  # one draw per cloud on the device: floor(u * L), u in [0, 1) float64
            u = torch.rand(N, dtype=torch.float64, device=dev)
            span = torch.full((N,), float(P), dtype=torch.float64, device=dev) if lengths is None else lengths.double()
            start = torch.minimum((u * span).long(), span.long() - 1)
    pts, idx = kernels.FarthestPoints.apply(points, lengths, K, start, Kmax)
    return pts.to(points.dtype), idx.long()


def estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size: int = 50,
                                           disambiguate_directions: bool = True, *,
                                           use_symeig_workaround: bool = True):
    """``pytorch3d.ops.estimate_pointcloud_local_coord_frames``: (curvatures (N,P,3), local_coord_frames (N,P,3,3)) of
    an (N,P,3) tensor or a ``Pointclouds``, in the input's dtype (coordinates are read as float32).

    For point i of a cloud of L points, with K = ``neighborhood_size``: the neighbourhood is its K nearest points of
    the same cloud, itself included (float32 squared distance (dx*dx + dy*dy) + dz*dz, equal distances to the lowest
    index: ``knn_points(p, p, K=K)``). With d_k = p_k - p_i and m their mean, C = (1/K) sum_k (d_k - m)(d_k - m)^T;
    ``curvatures[n,i]`` are C's eigenvalues ascending and ``local_coord_frames[n,i,:,j]`` is the unit eigenvector of
    the j-th: column 0 is the normal, column 2 the main direction. The solve is a fixed-sweep Jacobi in float32 on
    C / trace(C), so a rescaled cloud gives the same frames; C = 0 (K coincident points) gives zero curvatures and
    the identity before the signs.

    With ``disambiguate_directions`` columns 0 and 2 are negated iff fewer than half of the d_k have a positive
    projection on them, and column 1 becomes cross(column 0, column 2). Without, every column's component of largest
    magnitude is positive, the lowest axis among equal magnitudes (a convention of this library; upstream leaves the
    sign to ``eigh``). Rows past a cloud's length are zeros. ``use_symeig_workaround`` is accepted and ignored.

    2 <= K <= 64 (``NotImplementedError`` above); a cloud with L <= K, or D != 3, raises ``ValueError``. Not
    differentiable: an input that requires grad raises ``NotImplementedError`` unless grad mode is off. With a tensor
    input nothing synchronises and the call captures into a HIP graph; a ``Pointclouds``' lengths are checked on the
    host. One launch (kernels.point_frames, csrc/mr_normals.hip).

    ``pointclouds`` may be a ``PointGrid``: it stands for the points it was built from (their padded shape, dtype,
    lengths and host-side counts), every neighbourhood is searched through that index instead of the scan over the
    whole cloud (k_frames_grid), and the result is that of the call with the points, bit for bit, with the same
    errors. A grid whose tensor has been freed or modified in place since the build raises ValueError. Nothing routes
    automatically."""
    if isinstance(pointclouds, PointGrid):
        points, lengths, counts = pointclouds.points()
        return _local_frames(points, None if pointclouds.full else lengths, counts, neighborhood_size,
                             disambiguate_directions, pointclouds.buffer)
    if isinstance(pointclouds, Pointclouds):
        counts = pointclouds.counts()
        points = pointclouds.points_padded()
        lengths = None if all(c == points.shape[1] for c in counts) else pointclouds.num_points_per_cloud()
    elif torch.is_tensor(pointclouds):
        if pointclouds.dim() != 3:
            raise ValueError("estimate_pointcloud_local_coord_frames: pointclouds must be an (N, P, 3) tensor")
        points, lengths, counts = pointclouds, None, None
    else:
        raise ValueError("estimate_pointcloud_local_coord_frames: pointclouds is an (N, P, 3) tensor or a Pointclouds")
    return _local_frames(points, lengths, counts, neighborhood_size, disambiguate_directions)


def _local_frames(points, lengths, counts, neighborhood_size, disambiguate_directions, grid=None):
    """estimate_pointcloud_local_coord_frames on a padded (N,P,3) tensor with its lengths (None: full clouds) and the
    host-side counts (None: the padded size, or with lengths one read of them); ``grid``: the buffer of a PointGrid of
    these points and lengths, to search instead."""
    if counts is None:
        counts = [points.shape[1]] * points.shape[0] if lengths is None else [int(v) for v in lengths.tolist()]
    if points.shape[2] != 3:
        raise ValueError("The pointclouds argument has to be of shape (minibatch, N, 3)")
    K = int(neighborhood_size)
    if K < kernels.FRAMES_MIN_K:
        raise ValueError(f"estimate_pointcloud_local_coord_frames: neighborhood_size must be >= {kernels.FRAMES_MIN_K}")
    if K > kernels.FRAMES_MAX_K:
        raise NotImplementedError(f"estimate_pointcloud_local_coord_frames: neighborhood_size > {kernels.FRAMES_MAX_K} "
                                  "is not built")
    if any(c <= K for c in counts):
        raise ValueError("The neighborhood_size argument has to be smaller than the size of each of the point clouds.")
    _refuse_grad("estimate_pointcloud_local_coord_frames", points)
    _require_cuda(points)
    cur, frm = kernels.point_frames(points, lengths, K, bool(disambiguate_directions), grid=grid)
    return cur.to(points.dtype), frm.to(points.dtype)


def estimate_pointcloud_normals(pointclouds, neighborhood_size: int = 50, disambiguate_directions: bool = True, *,
                                use_symeig_workaround: bool = True):
    """``pytorch3d.ops.estimate_pointcloud_normals``: (N,P,3), column 0 of
    ``estimate_pointcloud_local_coord_frames`` (the unit eigenvector of the smallest eigenvalue of every point's
    neighbourhood covariance), with the same arguments, limits and errors."""
    _, frames = estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size, disambiguate_directions,
                                                       use_symeig_workaround=use_symeig_workaround)
    return frames[..., 0]
