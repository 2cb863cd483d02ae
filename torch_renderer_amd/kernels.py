"""Torch-facing wrappers + autograd Functions over the C ABI (libmi355r.so).

Each function allocates outputs/workspace with torch (HBM), passes raw pointers
and the current HIP stream, and never synchronises. The GPU path is the only
path: CPU tensors raise.
"""
from __future__ import annotations

import ctypes
import weakref
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import MrMesh, MrRasterSettings, MrShadeParams, check, ptr

_ADJ_CACHE: dict = {}
_LAST_RENDER = None  # (weakref to the last fused forward's workspace, its geometry) for render_stats()


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("mi355r: the MI355X path needs HIP device tensors (no CPU fallback)")


def _build_adjacency(faces: torch.Tensor, V: int):
    f = faces.detach().to("cpu", torch.int64).numpy()
    Fn = f.shape[0]
    vert = f.reshape(-1)
    face = np.repeat(np.arange(Fn, dtype=np.int64), 3)
    corner = np.tile(np.arange(3, dtype=np.int64), Fn)
    order = np.lexsort((face, corner, vert))
    counts = np.bincount(vert, minlength=V)
    ptr_ = np.zeros(V + 1, dtype=np.int32)
    np.cumsum(counts, out=ptr_[1:])
    adj = ((face[order] << 2) | corner[order]).astype(np.int32)
    return torch.from_numpy(ptr_).to(faces.device), torch.from_numpy(adj).to(faces.device)


def mesh_topology(faces: torch.Tensor, V: int):
    """(faces int32 (F,3), vadj_ptr (V+1), vadj) of a faces tensor, built once per tensor.

    The CSR lists vertex -> (face << 2 | corner) entries sorted by (corner, face): the
    summation order of Meshes.verts_normals_packed's three index_add calls. Cached on the
    identity and version of the caller's faces tensor (not on a data pointer), so a
    captured HIP graph or a steady-state step does no host work and no host sync here."""
    key = (id(faces), int(V))
    hit = _ADJ_CACHE.get(key)
    if hit is not None and hit[0]() is faces and hit[1] == faces._version:
        return hit[2]
    f32 = faces.detach().to(torch.int32).contiguous()
    vptr, vadj = _build_adjacency(f32, V)
    if len(_ADJ_CACHE) > 64:
        _ADJ_CACHE.clear()
    _ADJ_CACHE[key] = (weakref.ref(faces), faces._version, (f32, vptr, vadj))
    return f32, vptr, vadj


_PRIOR_CACHE: dict = {}


class PriorTopology:
    """What the shape-prior kernels (mr_mesh_priors_*) read of a batch of N meshes, in packed vertex ids and in
    fixed sorted orders: ``edges`` (E,2) unique undirected edges, min first, sorted by min * V + max; ``nbr_ptr``
    (V+1) / ``nbr`` (2E) each vertex's neighbours, ascending; ``pairs`` (P,4) = e0, e1, a, b for every unordered pair
    of faces on edge (e0, e1) with opposite vertices a, b, sorted by (edge, face of a, face of b); ``pair_ptr`` (V+1)
    / ``pair_idx`` (4P) each vertex's entries 4 * pair + role, ascending; the weights ``edge_w`` (E), ``pair_w`` (P)
    and ``vert_w`` (V,2) = (Laplacian weight, edge weight of the vertex's mesh), each 1 / (elements of that kind in
    the mesh * N). Index tensors are int32 on ``device``; the ``*_mesh_idx`` and count tensors int64."""

    __slots__ = ("N", "V", "E", "P", "device", "edges", "edge_w", "nbr_ptr", "nbr", "vert_w", "pairs", "pair_w",
                 "pair_ptr", "pair_idx", "edge_mesh_idx", "vert_mesh_idx", "num_edges_per_mesh", "__weakref__")


def _csr_ptr(owner, n):
    p = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(owner, minlength=n), out=p[1:])
    return p


def _build_prior_topology(faces_list, Vs, device) -> PriorTopology:
    N = len(faces_list)
    Vs = np.asarray(Vs, dtype=np.int64).reshape(N)
    Vt = int(Vs.sum())
    voff = np.cumsum(Vs) - Vs
    fl = []
    for m, f in enumerate(faces_list):
        f = f.detach().to("cpu", torch.int64).numpy().reshape(-1, 3)
        if f.size and (f.min() < 0 or f.max() >= Vs[m]):
            raise ValueError("mesh priors: faces index vertices outside the mesh")
        fl.append(f + voff[m])
    fp = np.concatenate(fl, 0) if fl else np.zeros((0, 3), dtype=np.int64)
    Fn = fp.shape[0]
    if Vt >= 2 ** 31 // 3 or 3 * Fn >= 2 ** 29:
        raise NotImplementedError("mesh priors: the packed batch is too large for 32-bit element ids")
    # half-edges in upstream's order (v1 v2, v2 v0, v0 v1), each with the face's opposite vertex
    ha = np.concatenate([fp[:, 1], fp[:, 2], fp[:, 0]])
    hb = np.concatenate([fp[:, 2], fp[:, 0], fp[:, 1]])
    opp = np.concatenate([fp[:, 0], fp[:, 1], fp[:, 2]])
    key = np.minimum(ha, hb) * max(Vt, 1) + np.maximum(ha, hb)
    ukey, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    edges = np.stack([ukey // max(Vt, 1), ukey % max(Vt, 1)], 1)
    E = edges.shape[0]
    vmesh = np.repeat(np.arange(N, dtype=np.int64), Vs)
    emesh = vmesh[edges[:, 0]]
    e_per = np.bincount(emesh, minlength=N)
    edge_w = 1.0 / (e_per[emesh] * float(N))
    # vertex -> neighbours
    src = np.concatenate([edges[:, 0], edges[:, 1]])
    dst = np.concatenate([edges[:, 1], edges[:, 0]])
    nbr = dst[np.lexsort((dst, src))]
    nbr_ptr = _csr_ptr(src, Vt)
    e_of_v = e_per[vmesh]
    vert_w = np.stack([1.0 / (Vs[vmesh] * float(N)),
                       np.where(e_of_v > 0, 1.0 / (np.maximum(e_of_v, 1) * float(N)), 0.0)], 1)
    # face pairs on each edge: half-edges sorted by (edge, face, corner); an edge with k of them gives k (k - 1) / 2
    hface = np.tile(np.arange(Fn, dtype=np.int64), 3)
    hcorner = np.repeat(np.arange(3, dtype=np.int64), Fn)
    opp_s = opp[np.lexsort((hcorner, hface, inv))]
    cnt = np.bincount(inv, minlength=E)
    start = np.cumsum(cnt) - cnt
    pe, pi, pj = [], [], []
    for i in range(int(cnt.max()) - 1 if E else 0):
        for j in range(i + 1, int(cnt.max())):
            sel = np.nonzero(cnt > j)[0]
            pe.append(sel)
            pi.append(np.full(sel.shape, i, dtype=np.int64))
            pj.append(np.full(sel.shape, j, dtype=np.int64))
    if pe:
        pe, pi, pj = np.concatenate(pe), np.concatenate(pi), np.concatenate(pj)
        o = np.lexsort((pj, pi, pe))
        pe, pi, pj = pe[o], pi[o], pj[o]
        pairs = np.stack([edges[pe, 0], edges[pe, 1], opp_s[start[pe] + pi], opp_s[start[pe] + pj]], 1)
    else:
        pairs = np.zeros((0, 4), dtype=np.int64)
    P = pairs.shape[0]
    pmesh = vmesh[pairs[:, 0]]
    pair_w = 1.0 / (np.bincount(pmesh, minlength=N)[pmesh] * float(N))
    # vertex -> (pair, role), ascending
    pvert = pairs.reshape(-1)
    pair_idx = np.argsort(pvert, kind="stable")
    pair_ptr = _csr_ptr(pvert, Vt)

    t = PriorTopology()
    t.N, t.V, t.E, t.P, t.device = N, Vt, E, P, device

    def dev(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a.astype(dtype))).to(device)

    t.edges, t.edge_w = dev(edges, np.int32), dev(edge_w, np.float32)
    t.nbr_ptr, t.nbr, t.vert_w = dev(nbr_ptr, np.int32), dev(nbr, np.int32), dev(vert_w, np.float32)
    t.pairs, t.pair_w = dev(pairs, np.int32), dev(pair_w, np.float32)
    t.pair_ptr, t.pair_idx = dev(pair_ptr, np.int32), dev(pair_idx, np.int32)
    t.edge_mesh_idx, t.vert_mesh_idx = dev(emesh, np.int64), dev(vmesh, np.int64)
    t.num_edges_per_mesh = dev(e_per, np.int64)
    return t


def mesh_prior_topology(faces_list, Vs) -> PriorTopology:
    """The PriorTopology of the meshes (faces_list[m] (F_m,3) over Vs[m] vertices), built on the host once per
    faces tensors and cached like mesh_topology: on the identity and version of each tensor, so a steady
    deformation loop (whose Meshes.offset_verts result keeps the source's faces tensors) or a captured HIP graph
    does no host work and no sync here."""
    faces_list = list(faces_list)
    Vs = tuple(int(v) for v in Vs)
    key = tuple(id(f) for f in faces_list) + Vs
    hit = _PRIOR_CACHE.get(key)
    if hit is not None and all(r() is f and ver == f._version for r, ver, f in zip(hit[0], hit[1], faces_list)):
        return hit[2]
    device = faces_list[0].device if faces_list else torch.device("cpu")
    topo = _build_prior_topology(faces_list, Vs, device)
    if len(_PRIOR_CACHE) > 64:
        _PRIOR_CACHE.clear()
    _PRIOR_CACHE[key] = ([weakref.ref(f) for f in faces_list], [f._version for f in faces_list], topo)
    return topo


class MeshShapePriors(torch.autograd.Function):
    """(edge, Laplacian, normal-consistency) losses of packed vertices (V,3) over a PriorTopology: two launches
    forward (mr_mesh_priors_forward: one pass over edges, vertices and pairs, then the fixed-order reduction) and
    one backward (mr_mesh_priors_backward: a per-vertex gather scaled by the three upstream scalars on the device).
    ``terms`` (MR_PRIOR_* mask) picks the terms computed; the others come out 0 and carry no gradient."""

    @staticmethod
    def forward(ctx, verts, topo, target_length, terms):
        _require_cuda(verts)
        L = _lib.load()
        v = verts.detach().float().contiguous()
        if tuple(v.shape) != (topo.V, 3):
            raise ValueError(f"mesh priors: verts must be ({topo.V}, 3), got {tuple(v.shape)}")
        if topo.device != v.device:
            raise RuntimeError("mesh priors: faces and vertices live on different devices")
        want = bool(ctx.needs_input_grad[0])
        out = torch.empty(3, device=v.device)
        ws, wsb = _workspace(L.mr_mesh_priors_workspace, v.device, topo.V, topo.E, topo.P)
        check(L.mr_mesh_priors_forward(ptr(v), topo.V, ptr(topo.edges), ptr(topo.edge_w), topo.E, ptr(topo.nbr_ptr),
                                       ptr(topo.nbr), ptr(topo.vert_w), ptr(topo.pairs), ptr(topo.pair_w), topo.P,
                                       float(target_length), int(terms), int(want), ptr(out), ptr(ws), wsb,
                                       _lib.stream_handle(v.device)))
        ctx.set_materialize_grads(False)
        if want:
            ctx.save_for_backward(v, ws)
            ctx.args = (topo, float(target_length), int(terms), verts.dtype)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_edge, g_lap, g_norm):
        if g_edge is None and g_lap is None and g_norm is None:
            return None, None, None, None
        v, ws = ctx.saved_tensors
        topo, target_length, terms, dtype = ctx.args
        gs = [None if g is None else g.detach().float().contiguous() for g in (g_edge, g_lap, g_norm)]
        _require_cuda(*gs)
        gv = torch.empty_like(v)
        check(_lib.load().mr_mesh_priors_backward(ptr(v), topo.V, ptr(topo.nbr_ptr), ptr(topo.nbr), ptr(topo.vert_w),
                                                  ptr(topo.pair_ptr), ptr(topo.pair_idx), topo.E, topo.P, target_length,
                                                  terms, ptr(gs[0]), ptr(gs[1]), ptr(gs[2]), ptr(ws), ptr(gv),
                                                  _lib.stream_handle(v.device)))
        return gv.to(dtype), None, None, None


# --------------------------------------------------------------------------- point clouds (csrc/mr_points.hip)
def _cloud_args(x, y, x_lengths, y_lengths, norm):
    """Contiguous float32 clouds and int64 lengths of a pair of (N,P,3) batches, with their sizes."""
    if x.dim() != 3 or y.dim() != 3:
        raise ValueError("point clouds must be (N, P, D) tensors")
    if x.shape[2] != 3 or y.shape[2] != 3:
        raise NotImplementedError("point clouds: only D = 3 is built")
    if x.shape[0] != y.shape[0]:
        raise ValueError("y does not have the correct shape.")
    if norm not in (1, 2):
        raise ValueError("Support for 1 or 2 norm.")
    N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
    if N < 1 or P1 < 1 or P2 < 1:
        raise ValueError("point clouds: N, P1 and P2 must be >= 1")
    ls = []
    for l in (x_lengths, y_lengths):
        if l is not None:
            if tuple(l.shape) != (N,):
                raise ValueError("lengths must be of shape (N,)")
            l = l.detach().to(torch.int64).contiguous()
        ls.append(l)
    _require_cuda(x, y, x_lengths, y_lengths)
    return x.detach().float().contiguous(), y.detach().float().contiguous(), ls[0], ls[1], N, P1, P2


def nearest_points(x, y, x_lengths=None, y_lengths=None, norm=2):
    """(dist_x, idx_x, dist_y, idx_y): for every point of x (N,P1,3) the distance to and the index of its nearest
    point of y (N,P2,3) (float32 / int32 (N,P1)), and the reverse ((N,P2)). norm 2: squared L2, norm 1: L1, in
    float32 with a fixed operation order; equal distances take the lowest index. Entries past a length, or of a
    cloud whose counterpart has length 0, are 0 / -1. No autograd; one memset and two launches (mr_nearest_points)."""
    xf, yf, xl, yl, N, P1, P2 = _cloud_args(x, y, x_lengths, y_lengths, norm)
    L = _lib.load()
    dev = xf.device
    dx, ix = torch.empty((N, P1), device=dev), torch.empty((N, P1), dtype=torch.int32, device=dev)
    dy, iy = torch.empty((N, P2), device=dev), torch.empty((N, P2), dtype=torch.int32, device=dev)
    ws, wsb = _workspace(L.mr_nearest_points_workspace, dev, N, P1, P2)
    check(L.mr_nearest_points(ptr(xf), ptr(yf), N, P1, P2, ptr(xl), ptr(yl), int(norm), ptr(dx), ptr(ix), ptr(dy),
                              ptr(iy), ptr(ws), wsb, _lib.stream_handle(dev)))
    return dx, ix, dy, iy


class ChamferDistance(torch.autograd.Function):
    """The chamfer loss of x (N,P1,3) and y (N,P2,3) with the MR_CHAMFER_* ``flags`` reductions: one memset and
    three launches forward (nearest neighbours of both directions, per-point reduce, final; mr_chamfer_forward), one
    memset and two launches backward (fixed-point scatter, gradients; mr_chamfer_backward). Returns a 0-dim tensor,
    or (N,) without a batch-reduction flag. Differentiable w.r.t. x and y (``weights`` is a constant)."""

    @staticmethod
    def forward(ctx, x, y, x_lengths, y_lengths, weights, flags, norm):
        xf, yf, xl, yl, N, P1, P2 = _cloud_args(x, y, x_lengths, y_lengths, norm)
        _require_cuda(weights)
        L = _lib.load()
        dev = xf.device
        w = None if weights is None else weights.detach().float().contiguous()
        want = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        single = bool(flags & _lib.MR_CHAMFER_SINGLE)
        per_cloud = not (flags & (_lib.MR_CHAMFER_BATCH_MEAN | _lib.MR_CHAMFER_BATCH_SUM))
        out = torch.empty(N if per_cloud else 1, device=dev)
        ix = torch.empty((N, P1), dtype=torch.int32, device=dev) if want else None
        iy = torch.empty((N, P2), dtype=torch.int32, device=dev) if want and not single else None
        coef = torch.empty((2, N), device=dev) if want else None
        ws, wsb = _workspace(L.mr_chamfer_workspace, dev, N, P1, P2)
        check(L.mr_chamfer_forward(ptr(xf), ptr(yf), N, P1, P2, ptr(xl), ptr(yl), ptr(w), int(norm), int(flags),
                                   ptr(ix), ptr(iy), ptr(coef), ptr(out), ptr(ws), wsb, _lib.stream_handle(dev)))
        ctx.set_materialize_grads(False)
        if want:
            ctx.save_for_backward(xf, yf, ix, iy, coef)
            ctx.args = (int(flags), int(norm), x.dtype, y.dtype)
        return out if per_cloud else out[0]

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 7
        xf, yf, ix, iy, coef = ctx.saved_tensors
        flags, norm, xdt, ydt = ctx.args
        g = g.detach().float().contiguous()
        _require_cuda(g)
        L = _lib.load()
        N, P1, P2 = xf.shape[0], xf.shape[1], yf.shape[1]
        gx, gy = torch.empty_like(xf), torch.empty_like(yf)
        ws, wsb = _workspace(L.mr_chamfer_backward_workspace, xf.device, N, P1, P2)
        check(L.mr_chamfer_backward(ptr(xf), ptr(yf), N, P1, P2, norm, flags, ptr(ix), ptr(iy), ptr(coef), ptr(g),
                                    ptr(gx), ptr(gy), ptr(ws), wsb, _lib.stream_handle(xf.device)))
        return gx.to(xdt), gy.to(ydt), None, None, None, None, None


# --------------------------------------------------------------------------- neighbour searches (csrc/mr_knn.h)
def _geometry(fn, n_out, *args):
    """The ``n_out`` int32 values a host-only ``*_geometry`` entry point reports for ``args``."""
    out = [ctypes.c_int32() for _ in range(n_out)]
    check(fn(*args, *(ctypes.byref(o) for o in out)))
    return tuple(o.value for o in out)


def _neighbour_forward(workspace, launch, scalar, p1f, p2f, l1, l2, N, P1, P2, K):
    """(dists, idx), both (N,P1,K), of mr_knn_points or mr_ball_query: the two entry points take the same arguments
    but for one ``scalar``, the norm or the radius."""
    dev = p1f.device
    dists = torch.empty((N, P1, K), device=dev)
    idx = torch.empty((N, P1, K), dtype=torch.int32, device=dev)
    ws, wsb = _workspace(workspace, dev, N, P1, P2, K)
    check(launch(ptr(p1f), ptr(p2f), N, P1, P2, ptr(l1), ptr(l2), scalar, K, ptr(dists), ptr(idx), ptr(ws), wsb,
                 _lib.stream_handle(dev)))
    return dists, idx


class _NeighbourDists(torch.autograd.Function):
    """What KnnPoints, KnnPointsGrid, BallQuery and BallQueryGrid are: a search ``_search(p1, p2, lengths1, lengths2, K,
    x, *more)`` (``more``: further arguments without a gradient, the grid buffer of the two grid classes) -> (dists, idx, the
    float32 clouds and int64 lengths it ran on, the checked K) with the gradient of ``dists`` w.r.t. p1 and p2 (``idx``
    is not differentiable): three launches backward and no memset, the many-to-one p2 side summed in fixed point, by
    the ``_backward`` entry point, which takes ``x`` as its norm if ``_pass_norm``."""

    @staticmethod
    def forward(ctx, p1, p2, lengths1, lengths2, K, x, *more):
        cls = ctx._forward_cls  # the subclass that was applied
        dists, idx, (p1f, p2f, l1, l2), K = cls._search(p1, p2, lengths1, lengths2, K, x, *more)
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(p1f, p2f, idx, l1, l2)
        ctx.args = (K, (int(x),) if cls._pass_norm else (), p1.dtype, p2.dtype, len(more))
        return dists, idx

    @staticmethod
    def backward(ctx, g, _g_idx):
        if g is None:
            return (None,) * (6 + ctx.args[4])
        p1f, p2f, idx, l1, l2 = ctx.saved_tensors
        K, norm, dt1, dt2, more = ctx.args
        g = g.detach().float().contiguous()
        _require_cuda(g)
        L = _lib.load()
        name = ctx._forward_cls._backward
        N, P1, P2 = p1f.shape[0], p1f.shape[1], p2f.shape[1]
        g1, g2 = torch.empty_like(p1f), torch.empty_like(p2f)
        ws, wsb = _workspace(getattr(L, name + "_workspace"), p1f.device, N, P1, P2, K)
        check(getattr(L, name)(ptr(p1f), ptr(p2f), N, P1, P2, ptr(l1), ptr(l2), *norm, K, ptr(idx), ptr(g), ptr(g1),
                               ptr(g2), ptr(ws), wsb, _lib.stream_handle(p1f.device)))
        return (g1.to(dt1), g2.to(dt2), None, None, None, None) + (None,) * more


# --------------------------------------------------------------------------- K nearest neighbours (csrc/mr_knn.hip)
KNN_MAX_K = 32


def _knn_k(K):
    K = int(K)
    if K < 1:
        raise ValueError("K must be >= 1")
    if K > KNN_MAX_K:
        raise NotImplementedError(f"knn_points: K > {KNN_MAX_K} is not built")
    return K


def knn_geometry(N, P1, P2, K):
    """(queries_per_group, splits, lds_chunk) of the launch mr_knn_points makes for these shapes (host only)."""
    return _geometry(_lib.load().mr_knn_geometry, 3, int(N), int(P1), int(P2), _knn_k(K))


def _knn_search(p1, p2, lengths1, lengths2, K, norm):
    K = _knn_k(K)
    p1f, p2f, l1, l2, N, P1, P2 = _cloud_args(p1, p2, lengths1, lengths2, norm)
    L = _lib.load()
    dists, idx = _neighbour_forward(L.mr_knn_points_workspace, L.mr_knn_points, int(norm), p1f, p2f, l1, l2, N, P1, P2,
                                    K)
    return dists, idx, (p1f, p2f, l1, l2), K


def knn_points(p1, p2, lengths1=None, lengths2=None, K=1, norm=2):
    """(dists (N,P1,K) float32, idx (N,P1,K) int32): for every point of p1 (N,P1,3) its K nearest points of
    p2[n, :lengths2[n]], ascending by (distance, index), with nearest_points' distance; equal distances take the
    lower index. Slots k >= min(K, lengths2[n]) and rows past lengths1[n] are 0 / -1. 1 <= K <= 32. No autograd; one
    launch, or a scan and a merge when the shapes alone cannot fill the chip (mr_knn_points)."""
    return _knn_search(p1, p2, lengths1, lengths2, K, norm)[:2]


class KnnPoints(_NeighbourDists):
    """knn_points with the gradient of ``dists`` w.r.t. p1 and p2 (``idx`` is not differentiable): three launches
    backward and no memset, the many-to-one p2 side summed in fixed point (mr_knn_points_backward)."""
    _search, _backward, _pass_norm = staticmethod(_knn_search), "mr_knn_points_backward", True


# --------------------------------------------------------------------------- point grid (csrc/mr_grid.hip)
def _grid_points(points, lengths):
    """The checked inputs of a grid build: (float32 points, int64 lengths or None, N, P)."""
    if points.dim() != 3:
        raise ValueError("point grid: points must be an (N, P, 3) tensor")
    if points.shape[2] != 3:
        raise NotImplementedError("point grid: only D = 3 is built")
    N, P = points.shape[0], points.shape[1]
    if N < 1 or P < 1:
        raise ValueError("point grid: N and P must be >= 1")
    if lengths is not None:
        if tuple(lengths.shape) != (N,):
            raise ValueError("lengths must be of shape (N,)")
        lengths = lengths.detach().to(torch.int64).contiguous()
    _require_cuda(points, lengths)
    return points.detach().float().contiguous(), lengths, N, P


def point_grid_build(points, lengths=None):
    """The grid buffer (uint8, mr_point_grid_bytes) of points[n, :lengths[n]] (N,P,3): every cloud's points sorted into
    the cells of a uniform grid whose cell size and dims are chosen on the device. Four launches, nothing read back
    (mr_point_grid_build)."""
    pf, l, N, P = _grid_points(points, lengths)
    L = _lib.load()
    grid, gb = _workspace(L.mr_point_grid_bytes, pf.device, N, P, what="point grid: the clouds are too large")
    ws, wsb = _workspace(L.mr_point_grid_build_workspace, pf.device, N, P)
    check(L.mr_point_grid_build(ptr(pf), N, P, ptr(l), ptr(grid), gb, ptr(ws), wsb, _lib.stream_handle(pf.device)))
    return grid


def point_grid_describe(grid, N, P):
    """(dims (N,3) int32, origin_cell (N,4) float32 = lo xyz and the cell size, max_cell_count (N,) int32) of a grid
    buffer of point_grid_build, on the host. Synchronises: for tests and tools (mr_point_grid_describe)."""
    _require_cuda(grid)
    N, P = int(N), int(P)
    L = _lib.load()
    if grid.dtype != torch.uint8 or grid.numel() < _ws_size(L.mr_point_grid_bytes, N, P) or not grid.is_contiguous():
        raise ValueError("point grid: not a grid buffer of these shapes")
    dims, cell, most = torch.empty((N, 3), dtype=torch.int32), torch.empty((N, 4)), torch.empty(N, dtype=torch.int32)
    check(L.mr_point_grid_describe(ptr(grid), N, P, ptr(dims), ptr(cell), ptr(most), _lib.stream_handle(grid.device)))
    return dims, cell, most


def _knn_grid_search(p1, p2, lengths1, lengths2, K, norm, grid, visited=None):
    K = _knn_k(K)
    p1f, p2f, l1, l2, N, P1, P2 = _cloud_args(p1, p2, lengths1, lengths2, norm)
    _require_cuda(grid, visited)
    L = _lib.load()
    gb = _ws_size(L.mr_point_grid_bytes, N, P2)
    if grid.dtype != torch.uint8 or grid.numel() != gb or gb == 0 or not grid.is_contiguous():
        raise ValueError("knn_points: the grid buffer was not built for a target batch of this shape")
    if visited is not None and (visited.dtype != torch.int64 or visited.numel() != 1):
        raise ValueError("knn_points: visited must be one int64")
    dev = p1f.device
    dists = torch.empty((N, P1, K), device=dev)
    idx = torch.empty((N, P1, K), dtype=torch.int32, device=dev)
    ws, wsb = _workspace(L.mr_knn_points_grid_workspace, dev, N, P1, P2, K)
    check(L.mr_knn_points_grid(ptr(p1f), ptr(p2f), N, P1, P2, ptr(l1), ptr(l2), ptr(grid), gb, int(norm), K,
                               ptr(dists), ptr(idx), ptr(visited), ptr(ws), wsb, _lib.stream_handle(dev)))
    return dists, idx, (p1f, p2f, l1, l2), K


def knn_points_grid(p1, p2, grid, lengths1=None, lengths2=None, K=1, norm=2, visited=None):
    """knn_points' (dists, idx), bit for bit, through ``grid`` = point_grid_build(p2, lengths2): a query visits the
    cells around its own in growing cube rings and stops once no unvisited cell can hold a nearer point. ``visited``
    (one int64 on the device, cleared by the caller) gains the number of distances evaluated. A grid of other clouds
    of the same shape gives wrong neighbours, idx still in [-1, P2). No autograd; one launch (mr_knn_points_grid)."""
    return _knn_grid_search(p1, p2, lengths1, lengths2, K, norm, grid, visited)[:2]


class KnnPointsGrid(_NeighbourDists):
    """KnnPoints with the forward search through a grid buffer, ``apply(p1, p2, lengths1, lengths2, K, norm, grid)``:
    the same idx, so the same backward (mr_knn_points_backward)."""
    _search, _backward, _pass_norm = staticmethod(_knn_grid_search), "mr_knn_points_backward", True


# --------------------------------------------------------------------------- radius neighbourhoods (csrc/mr_ballquery.hip)
def _ball_args(K, radius):
    K, radius = int(K), float(radius)
    if K < 1:
        raise ValueError("K must be >= 1")
    if not (0.0 <= radius < float("inf")):
        raise ValueError("ball_query: radius must be finite and >= 0")
    return K, radius


def ball_query_geometry(N, P1, P2, K):
    """(queries_per_group, splits, lds_chunk) of the launches mr_ball_query makes for these shapes (host only)."""
    return _geometry(_lib.load().mr_ball_query_geometry, 3, int(N), int(P1), int(P2), int(K))


def _ball_search(p1, p2, lengths1, lengths2, K, radius):
    K, radius = _ball_args(K, radius)
    p1f, p2f, l1, l2, N, P1, P2 = _cloud_args(p1, p2, lengths1, lengths2, 2)
    L = _lib.load()
    dists, idx = _neighbour_forward(L.mr_ball_query_workspace, L.mr_ball_query, radius, p1f, p2f, l1, l2, N, P1, P2,
                                    K)
    return dists, idx, (p1f, p2f, l1, l2), K


def ball_query(p1, p2, lengths1=None, lengths2=None, K=500, radius=0.2):
    """(dists (N,P1,K) float32, idx (N,P1,K) int32): for every point of p1 (N,P1,3) the first K points of
    p2[n, :lengths2[n]], in index order, whose float32 squared distance (nearest_points') is < float32(radius)^2;
    dists holds those distances, unsorted. Free slots and rows past lengths1[n] are 0 / -1. Any K >= 1. No autograd;
    one launch, or a counting and a writing pass when the shapes alone cannot fill the chip (mr_ball_query)."""
    return _ball_search(p1, p2, lengths1, lengths2, K, radius)[:2]


class BallQuery(_NeighbourDists):
    """ball_query with the gradient of ``dists`` w.r.t. p1 and p2 (``idx`` is not differentiable): three launches
    backward and no memset, the many-to-one p2 side summed in fixed point (mr_ball_query_backward)."""
    _search, _backward, _pass_norm = staticmethod(_ball_search), "mr_ball_query_backward", False


BALL_GRID_MAX_K = 64


def _ball_grid_search(p1, p2, lengths1, lengths2, K, radius, grid, visited=None):
    K, radius = _ball_args(K, radius)
    if K > BALL_GRID_MAX_K:
        raise NotImplementedError(f"ball_query: K > {BALL_GRID_MAX_K} through a grid is not built")
    p1f, p2f, l1, l2, N, P1, P2 = _cloud_args(p1, p2, lengths1, lengths2, 2)
    if not torch.is_tensor(grid):
        raise ValueError("ball_query: grid is the buffer tensor of point_grid_build")
    _require_cuda(grid, visited)
    L = _lib.load()
    gb = _ws_size(L.mr_point_grid_bytes, N, P2)
    if grid.dtype != torch.uint8 or grid.numel() != gb or gb == 0 or not grid.is_contiguous():
        raise ValueError("ball_query: the grid buffer was not built for a target batch of this shape")
    if visited is not None and (visited.dtype != torch.int64 or visited.numel() != 1):
        raise ValueError("ball_query: visited must be one int64")
    dev = p1f.device
    dists = torch.empty((N, P1, K), device=dev)
    idx = torch.empty((N, P1, K), dtype=torch.int32, device=dev)
    ws, wsb = _workspace(L.mr_ball_query_grid_workspace, dev, N, P1, P2, K)
    check(L.mr_ball_query_grid(ptr(p1f), ptr(p2f), N, P1, P2, ptr(l1), ptr(l2), ptr(grid), gb, radius, K, ptr(dists),
                               ptr(idx), ptr(visited), ptr(ws), wsb, _lib.stream_handle(dev)))
    return dists, idx, (p1f, p2f, l1, l2), K


def ball_query_grid(p1, p2, grid, lengths1=None, lengths2=None, K=16, radius=0.2, visited=None):
    """ball_query's (dists, idx), bit for bit, through ``grid`` = point_grid_build(p2, lengths2), for K <= 64: a query
    visits the cells around its own in growing cube rings until no unvisited cell can hold a target inside the radius,
    and keeps its K lowest-indexed hits. ``visited`` (one int64 on the device, cleared by the caller) gains the number
    of distances evaluated. A grid of other clouds of the same shape gives wrong neighbours, idx still in [-1, P2). No
    autograd; one launch (mr_ball_query_grid)."""
    return _ball_grid_search(p1, p2, lengths1, lengths2, K, radius, grid, visited)[:2]


class BallQueryGrid(_NeighbourDists):
    """BallQuery with the forward search through a grid buffer, ``apply(p1, p2, lengths1, lengths2, K, radius, grid)``:
    the same idx, so the same backward (mr_ball_query_backward)."""
    _search, _backward, _pass_norm = staticmethod(_ball_grid_search), "mr_ball_query_backward", False


# --------------------------------------------------------------------------- farthest points (csrc/mr_fps.hip)
def farthest_geometry(N, P, Kmax):
    """(threads, points_per_thread, streamed) of the launch mr_farthest_points makes for these shapes (host only):
    the workgroup size, the points a thread keeps in registers (the bucket 1, 2, 4, ..., 32; for a streamed cloud
    the points a thread walks every round), and whether the cloud is too large for the registers."""
    threads, per_thread, streamed = _geometry(_lib.load().mr_farthest_points_geometry, 3, int(N), int(P), int(Kmax))
    return threads, per_thread, bool(streamed)


def _farthest_args(points, lengths, K, start_idx, Kmax):
    """The checked inputs of a farthest-points call: (float32 points, lengths, K per cloud or None, start, N, P, Kmax)."""
    if points.dim() != 3:
        raise ValueError("farthest points: points must be an (N, P, D) tensor")
    if points.shape[2] != 3:
        raise NotImplementedError("farthest points: only D = 3 is built")
    N, P = points.shape[0], points.shape[1]
    if N < 1 or P < 1:
        raise ValueError("farthest points: N and P must be >= 1")
    kper = None
    if torch.is_tensor(K):
        if tuple(K.shape) != (N,):
            raise ValueError("K and points must have the same batch dimension")
        kper = K
        Kmax = int(K.max()) if Kmax is None else int(Kmax)  # the one host read of a device K
    else:
        Kmax = int(K)
    if Kmax < 1:
        raise ValueError("farthest points: the output width max(K) must be >= 1")
    for name, t in (("lengths", lengths), ("start_idx", start_idx)):
        if t is not None and tuple(t.shape) != (N,):
            raise ValueError(f"farthest points: {name} must be of shape (N,)")
    _require_cuda(points, lengths, kper, start_idx)
    i64 = [None if t is None else t.detach().to(torch.int64).contiguous() for t in (lengths, kper, start_idx)]
    return (points.detach().float().contiguous(), *i64, N, P, Kmax)


def farthest_points(points, lengths=None, K=50, start_idx=None, Kmax=None):
    """(idx (N,Kmax) int32, pts (N,Kmax,3) float32): farthest-point subsampling of points (N,P,3) by the rule of
    mr_farthest_points (include/mi355r.h): cloud n starts at ``start_idx[n]`` (None: 0) and selects min(K[n],
    lengths[n]) points, each the one farthest (float32 squared distance, fixed operation order) from those selected
    so far, the lowest index among equal distances; ``pts`` are their coordinates and the unused slots are -1 / 0.
    ``K`` is an int or an (N,) tensor; ``Kmax`` (the output width) saves the host read of a tensor ``K``'s maximum.
    No autograd; one launch, one workgroup per cloud, nothing synchronises."""
    pf, l, kper, st, N, P, Kmax = _farthest_args(points, lengths, K, start_idx, Kmax)
    L = _lib.load()
    dev = pf.device
    idx = torch.empty((N, Kmax), dtype=torch.int32, device=dev)
    pts = torch.empty((N, Kmax, 3), device=dev)
    ws, wsb = _workspace(L.mr_farthest_points_workspace, dev, N, P, Kmax,
                         what="mi355r: farthest points: clouds too large for 32-bit point ids")
    check(L.mr_farthest_points(ptr(pf), N, P, ptr(l), ptr(kper), Kmax, ptr(st), ptr(idx), ptr(pts), ptr(ws), wsb,
                               _lib.stream_handle(dev)))
    return idx, pts


class FarthestPoints(torch.autograd.Function):
    """farthest_points as an autograd node: (pts, idx), ``idx`` not differentiable, ``pts`` differentiable w.r.t.
    ``points``. The forward returns the coordinates the kernel holds; the backward scatters the upstream gradient
    to the selected rows with torch's ``index_put_(accumulate=True)`` (a row selected more than once takes the sum;
    the padded slots add zeros to row 0). No backward kernel."""

    @staticmethod
    def forward(ctx, points, lengths, K, start_idx, Kmax):
        idx, pts = farthest_points(points, lengths, K, start_idx, Kmax)
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(idx)
            ctx.args = (tuple(points.shape), points.dtype)
        return pts, idx

    @staticmethod
    def backward(ctx, g, _g_idx):
        if g is None:
            return (None,) * 5
        (idx,) = ctx.saved_tensors
        shape, dtype = ctx.args
        g = g.detach().to(dtype).masked_fill((idx < 0)[..., None], 0)
        grad = torch.zeros(shape, dtype=dtype, device=g.device)
        rows = torch.arange(shape[0], device=g.device)[:, None].expand_as(idx)
        grad.index_put_((rows, idx.clamp(min=0).long()), g, accumulate=True)
        return grad, None, None, None, None


# --------------------------------------------------------------------------- local frames (csrc/mr_normals.hip)
FRAMES_MIN_K, FRAMES_MAX_K = 2, 64


def _frames_k(K, P):
    K = int(K)
    if K < FRAMES_MIN_K:
        raise ValueError(f"point frames: the neighbourhood size must be >= {FRAMES_MIN_K}")
    if K > FRAMES_MAX_K:
        raise NotImplementedError(f"point frames: a neighbourhood size > {FRAMES_MAX_K} is not built")
    if P <= K:
        raise ValueError("The neighborhood_size argument has to be smaller than the number of points in each "
                         f"pointcloud (P = {P}, neighbourhood size {K}).")
    return K


def frames_geometry(N, P, K):
    """(bucket, queries_per_group, splits, lds_chunk) of the launch mr_point_frames makes for these shapes (host only)."""
    return _geometry(_lib.load().mr_point_frames_geometry, 4, int(N), int(P), _frames_k(K, int(P)))


def symmetric_eig3_host(cov):
    """(eigenvalues (M,3) ascending, eigenvectors (M,3,3) in columns) of M symmetric 3x3 matrices given as an (M,6)
    float32 CPU tensor of upper triangles xx, xy, xz, yy, yz, zz: the solver of mr_point_frames run on the host
    (mr_symmetric_eig3_host; no GPU). Every column's component of largest magnitude is positive."""
    if cov.dim() != 2 or cov.shape[1] != 6 or cov.dtype != torch.float32 or cov.device.type != "cpu":
        raise ValueError("symmetric_eig3_host: cov must be an (M, 6) float32 CPU tensor")
    cov = cov.contiguous()
    M = cov.shape[0]
    lam, vec = torch.empty((M, 3)), torch.empty((M, 3, 3))
    check(_lib.load().mr_symmetric_eig3_host(ptr(cov), M, ptr(lam), ptr(vec)))
    return lam, vec


def point_frames(points, lengths=None, K=50, disambiguate=True, return_cov=False, grid=None, visited=None):
    """(curvatures (N,P,3), frames (N,P,3,3)[, cov (N,P,6)]) in float32, by the rule of mr_point_frames
    (include/mi355r.h): for every point i < lengths[n] of points (N,P,3), the covariance of its K nearest points of the
    same cloud (itself included; knn_points' distance and tie rule) about their mean, its eigenvalues ascending and
    their unit eigenvectors in the columns of the frame (column 0 the normal). ``disambiguate`` signs columns 0 and 2
    towards the majority of the neighbours and makes column 1 their cross product; otherwise every column's largest
    component is positive. ``cov`` is the covariance's upper triangle xx, xy, xz, yy, yz, zz. Rows past a length, and
    every row of a cloud shorter than K, are zeros; P <= K raises ValueError. 2 <= K <= 64. No autograd; one launch,
    or a scan and a merge when the shapes alone cannot fill the chip; nothing synchronises.

    ``grid`` = point_grid_build(points, lengths) searches every point's neighbourhood through that index instead
    (mr_point_frames_grid, one launch): the same outputs bit for bit. ``visited`` (one int64 on the device, cleared by
    the caller; only with a grid) gains the number of distances evaluated. A grid of other clouds of the same shape
    gives wrong frames and may leave rows unwritten."""
    if points.dim() != 3:
        raise ValueError("point frames: points must be an (N, P, D) tensor")
    if points.shape[2] != 3:
        raise ValueError("point frames: the points must be 3-dimensional (D = 3)")
    N, P = points.shape[0], points.shape[1]
    if N < 1:
        raise ValueError("point frames: N must be >= 1")
    K = _frames_k(K, P)
    if lengths is not None and tuple(lengths.shape) != (N,):
        raise ValueError("lengths must be of shape (N,)")
    if grid is None:
        if visited is not None:
            raise ValueError("point frames: visited counts the distances of a search through a grid")
    elif not torch.is_tensor(grid):
        raise ValueError("point frames: grid is the buffer tensor of point_grid_build")
    _require_cuda(points, lengths, grid, visited)
    pf = points.detach().float().contiguous()
    l = None if lengths is None else lengths.detach().to(torch.int64).contiguous()
    L = _lib.load()
    if grid is not None:
        gb = _ws_size(L.mr_point_grid_bytes, N, P)
        if grid.dtype != torch.uint8 or grid.numel() != gb or gb == 0 or not grid.is_contiguous():
            raise ValueError("point frames: the grid buffer was not built for a batch of this shape")
        if visited is not None and (visited.dtype != torch.int64 or visited.numel() != 1):
            raise ValueError("point frames: visited must be one int64")
    dev = pf.device
    cur, frm = torch.empty((N, P, 3), device=dev), torch.empty((N, P, 3, 3), device=dev)
    cov = torch.empty((N, P, 6), device=dev) if return_cov else None
    flags = _lib.MR_FRAMES_DISAMBIGUATE if disambiguate else 0
    if grid is None:
        ws, wsb = _workspace(L.mr_point_frames_workspace, dev, N, P, K)
        check(L.mr_point_frames(ptr(pf), N, P, ptr(l), K, flags, ptr(cur), ptr(frm), ptr(cov), ptr(ws), wsb,
                                _lib.stream_handle(dev)))
    else:
        ws, wsb = _workspace(L.mr_point_frames_grid_workspace, dev, N, P, K)
        check(L.mr_point_frames_grid(ptr(pf), N, P, ptr(l), ptr(grid), gb, K, flags, ptr(cur), ptr(frm), ptr(cov),
                                     ptr(visited), ptr(ws), wsb, _lib.stream_handle(dev)))
    return (cur, frm, cov) if return_cov else (cur, frm)


def _one_cloud(t, name):
    """A (P,3) or (1,P,3) cloud as a contiguous float32 (P,3) tensor."""
    if t.dim() == 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 2:
        raise ValueError(f"posed chamfer: {name} must be one cloud, (P, 3) or (1, P, 3)")
    if t.shape[1] != 3:
        raise NotImplementedError("posed chamfer: only D = 3 is built")
    if t.shape[0] < 1:
        raise ValueError(f"posed chamfer: {name} is empty")
    return t.detach().float().contiguous()


def _pose_args(R, T, s):
    """(R (S,3,3), T (S,3), s (S,) or None) checked; T may come as (S,1,3)."""
    if R.dim() != 3 or tuple(R.shape[1:]) != (3, 3):
        raise ValueError("posed chamfer: R must be (S, 3, 3)")
    S = R.shape[0]
    if S < 1:
        raise ValueError("posed chamfer: at least one pose is needed")
    if tuple(T.shape) not in ((S, 3), (S, 1, 3)):
        raise ValueError("posed chamfer: T must be (S, 3) or (S, 1, 3) with R's S")
    if s is not None and tuple(s.shape) != (S,):
        raise ValueError("posed chamfer: s must be (S,) with R's S")
    return S


def _pack_rts(R, T, s):
    """(S,13) float32 rows (R row-major, T, s): one cat launch (a non-contiguous R is gathered by it)."""
    S = R.shape[0]
    sc = R.new_ones((S, 1), dtype=torch.float32) if s is None else s.detach().float().reshape(S, 1)
    return torch.cat((R.detach().float().reshape(S, 9), T.detach().float().reshape(S, 3), sc), 1)


def _posed_chamfer_launch(xf, yf, rts, norm, flags, want_idx, want_grad):
    L = _lib.load()
    dev = xf.device
    S, P1, P2 = rts.shape[0], xf.shape[0], yf.shape[0]
    single = bool(flags & _lib.MR_CHAMFER_SINGLE)
    out = torch.empty(S, device=dev)
    ix = torch.empty((S, P1), dtype=torch.int32, device=dev) if want_idx else None
    iy = torch.empty((S, P2), dtype=torch.int32, device=dev) if want_idx and not single else None
    pg = torch.empty((S, 13), device=dev) if want_grad else None
    ws, wsb = _workspace(L.mr_posed_chamfer_workspace, dev, S, P1, P2,
                         what="mi355r: posed chamfer: more than 65535 poses or clouds too large for 32-bit point "
                              "ids")
    check(L.mr_posed_chamfer(ptr(xf), ptr(yf), P1, P2, ptr(rts), S, int(norm), int(flags), ptr(out), ptr(ix), ptr(iy),
                             ptr(pg), ptr(ws), wsb, _lib.stream_handle(dev)))
    return out, ix, iy, pg


def posed_chamfer(x, y, R, T, s=None, norm=2, flags=_lib.MR_CHAMFER_POINT_MEAN, return_idx=False, return_grad=False):
    """The chamfer distance of ONE cloud pair under S poses, x' = s (x R) + T with row vectors (mr_posed_chamfer):
    out (S,) float32, what ``ChamferDistance`` without a batch reduction gives for the materialised clouds
    (x' of pose k, y). ``flags``: MR_CHAMFER_POINT_MEAN | MR_CHAMFER_SINGLE. With ``return_idx`` also the neighbours
    idx_x (S,P1) and idx_y (S,P2; None with MR_CHAMFER_SINGLE) as int32, ties to the lowest index; with
    ``return_grad`` also pose_grad (S,13) = d out[k] / d (R row-major, T, s). No autograd (``PosedChamfer`` is the
    node); two launches after one cat that packs the poses, nothing synchronises.
    Returns out, or (out, idx_x, idx_y[, pose_grad]) / (out, pose_grad)."""
    if norm not in (1, 2):
        raise ValueError("Support for 1 or 2 norm.")
    xf, yf = _one_cloud(x, "x"), _one_cloud(y, "y")
    _pose_args(R, T, s)
    _require_cuda(xf, yf, R, T, s)
    out, ix, iy, pg = _posed_chamfer_launch(xf, yf, _pack_rts(R, T, s), norm, flags, return_idx, return_grad)
    if not return_idx and not return_grad:
        return out
    return (out,) + ((ix, iy) if return_idx else ()) + ((pg,) if return_grad else ())


class PosedChamfer(torch.autograd.Function):
    """``posed_chamfer`` as an autograd node over (R, T, s): the forward leaves d out[k] / d pose k (S,13), computed
    from 13 float64 moments per workgroup in a fixed order, and the backward is that times the upstream (S,)
    gradient: one multiply. The clouds are constants. ``s`` may be None."""

    @staticmethod
    def forward(ctx, x, y, R, T, s, flags, norm):
        xf, yf = _one_cloud(x, "x"), _one_cloud(y, "y")
        _pose_args(R, T, s)
        _require_cuda(xf, yf, R, T, s)
        want = bool(ctx.needs_input_grad[2] or ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
        out, _, _, pg = _posed_chamfer_launch(xf, yf, _pack_rts(R, T, s), norm, flags, False, want)
        ctx.set_materialize_grads(False)
        if want:
            ctx.save_for_backward(pg)
            ctx.args = (R.dtype, T.dtype, tuple(T.shape), None if s is None else s.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 7
        (pg,) = ctx.saved_tensors
        rdt, tdt, tshape, sdt = ctx.args
        need = ctx.needs_input_grad
        gp = g.detach().float()[:, None] * pg
        gR = gp[:, :9].reshape(-1, 3, 3).to(rdt) if need[2] else None
        gT = gp[:, 9:12].reshape(tshape).to(tdt) if need[3] else None
        gs = gp[:, 12].to(sdt) if need[4] and sdt is not None else None
        return None, None, gR, gT, gs, None, None


# --------------------------------------------------------------------------- point to mesh (csrc/mr_pointmesh.hip)
@dataclass
class PointMeshBatch:
    """How N clouds and N meshes lie in the packed arrays the point-to-face kernels read: ``points_first`` /
    ``points_count`` and ``faces_first`` / ``faces_count`` (N) int64 device tensors, ``faces`` (T,3) int32 over packed
    vertex ids, and the host-side bounds ``max_points`` / ``max_faces`` of the counts that size the grids."""
    points_first: torch.Tensor
    points_count: torch.Tensor
    max_points: int
    faces: torch.Tensor
    faces_first: torch.Tensor
    faces_count: torch.Tensor
    max_faces: int

    @property
    def N(self):
        return int(self.points_first.shape[0])


_FACE_TABLE_CACHE: dict = {}


def mesh_face_table(faces_list, Vs):
    """(faces (T,3) int32 over packed vertex ids, faces_first (N), faces_count (N) int64, max_faces) of the meshes
    (faces_list[m] (F_m,3) over Vs[m] vertices), built once per faces tensors and cached like mesh_prior_topology: on
    the identity and version of each tensor, so a steady loop or a captured HIP graph uploads nothing here."""
    faces_list = list(faces_list)
    Vs = tuple(int(v) for v in Vs)
    key = tuple(id(f) for f in faces_list) + Vs
    hit = _FACE_TABLE_CACHE.get(key)
    if hit is not None and all(r() is f and ver == f._version for r, ver, f in zip(hit[0], hit[1], faces_list)):
        return hit[2]
    dev = faces_list[0].device
    counts = [int(f.shape[0]) for f in faces_list]
    voff = np.cumsum((0,) + Vs[:-1])
    packed = torch.cat([f.reshape(-1, 3).to(torch.int32) + int(o) for f, o in zip(faces_list, voff)], 0).contiguous()
    first = torch.tensor(np.cumsum([0] + counts[:-1]), dtype=torch.int64).to(dev)
    table = (packed, first, torch.tensor(counts, dtype=torch.int64).to(dev), max(counts))
    if len(_FACE_TABLE_CACHE) > 64:
        _FACE_TABLE_CACHE.clear()
    _FACE_TABLE_CACHE[key] = ([weakref.ref(f) for f in faces_list], [f._version for f in faces_list], table)
    return table


def _pm_args(points, verts, batch, min_triangle_area):
    """The checked inputs of a point-to-face call: contiguous float32 points and verts, and the C ABI's leading
    arguments (the packed batch)."""
    if points.dim() != 2 or verts.dim() != 2 or batch.faces.dim() != 2 or batch.faces.shape[1] != 3:
        raise ValueError("point-face distance: points (P, D), verts (V, D) and faces (T, 3) are packed 2-D tensors")
    if points.shape[1] != 3 or verts.shape[1] != 3:
        raise NotImplementedError("point-face distance: only D = 3 is built")
    N = batch.N
    for t in (batch.points_count, batch.faces_first, batch.faces_count):
        if tuple(t.shape) != (N,):
            raise ValueError("point-face distance: the first / count tensors must all be of shape (N,)")
    if N < 1:
        raise ValueError("point-face distance: N must be >= 1")
    if not float(min_triangle_area) >= 0.0:
        raise ValueError("point-face distance: min_triangle_area must be >= 0")
    _require_cuda(points, verts, batch.faces, batch.points_first, batch.points_count, batch.faces_first,
                  batch.faces_count)
    pf, vf = points.detach().float().contiguous(), verts.detach().float().contiguous()
    i64 = [t.detach().to(torch.int64).contiguous() for t in (batch.points_first, batch.points_count, batch.faces_first,
                                                             batch.faces_count)]
    faces = batch.faces.detach().to(torch.int32).contiguous()
    P, V, T = pf.shape[0], vf.shape[0], faces.shape[0]
    args = (ptr(pf), P, ptr(i64[0]), ptr(i64[1]), int(batch.max_points), ptr(vf), V, ptr(faces), T, ptr(i64[2]),
            ptr(i64[3]), int(batch.max_faces), N, float(min_triangle_area))
    return pf, vf, args, (pf, vf, faces, *i64)


def _pm_nearest(points, verts, batch, min_triangle_area, want=(True, True, True, True)):
    pf, vf, args, keep = _pm_args(points, verts, batch, min_triangle_area)
    L = _lib.load()
    dev = pf.device
    P, T = pf.shape[0], batch.faces.shape[0]
    outs = [torch.empty(n, dtype=dt, device=dev) if w else None
            for n, dt, w in zip((P, P, T, T), (torch.float32, torch.int32, torch.float32, torch.int32), want)]
    ws, wsb = _workspace(L.mr_point_face_nearest_workspace, dev, batch.N, P, T,
                         what="mi355r: point-face nearest: more than 65535 meshes or a batch too large for 32-bit "
                              "indices")
    check(L.mr_point_face_nearest(*args, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), ptr(ws), wsb,
                                  _lib.stream_handle(dev)))
    return outs, keep


def point_face_nearest(points, points_first, points_count, verts, faces, faces_first, faces_count,
                       min_triangle_area=5e-3, max_points=None, max_faces=None):
    """(dist_p, idx_p, dist_f, idx_f) of a packed batch of N clouds and N meshes that pair up one to one: for every
    point of ``points`` (P,3) the squared distance to and the index (within its mesh) of the nearest face of its own
    mesh (float32 / int32 (P,)), and for every face of ``faces`` (T,3) over ``verts`` (V,3) the nearest point of its
    own cloud ((T,), index within the cloud). ``*_first`` / ``*_count`` (N) give each cloud's and mesh's range of the
    packed arrays; ``max_points`` / ``max_faces`` are host-side bounds of the counts (default: P and T). The
    distance is the one include/mi355r.h states (a face below ``min_triangle_area`` is its three edges), float32 in
    a fixed operation order; equal distances take the lowest index; a point or face without a counterpart gets
    0 / -1. No autograd; one memset and two launches (mr_point_face_nearest), nothing synchronises."""
    batch = PointMeshBatch(points_first, points_count, points.shape[0] if max_points is None else max_points, faces,
                           faces_first, faces_count, faces.shape[0] if max_faces is None else max_faces)
    outs, _ = _pm_nearest(points, verts, batch, min_triangle_area)
    return tuple(outs)


def _pm_backward(keep, batch_args, idx_p, idx_f, coef, g, gdp, gdf):
    pf, vf = keep[0], keep[1]
    L = _lib.load()
    gp, gv = torch.empty_like(pf), torch.empty_like(vf)
    ws, wsb = _workspace(L.mr_point_mesh_face_backward_workspace, pf.device, pf.shape[0], vf.shape[0])
    check(L.mr_point_mesh_face_backward(*batch_args, ptr(idx_p), ptr(idx_f), ptr(coef), ptr(g), ptr(gdp), ptr(gdf),
                                        ptr(gp), ptr(gv), ptr(ws), wsb, _lib.stream_handle(pf.device)))
    return gp, gv


class PointMeshFaceDistance(torch.autograd.Function):
    """The point-to-mesh face loss of packed ``points`` (P,3) and ``verts`` (V,3) over a PointMeshBatch: one memset
    and three launches forward (both directions' nearest primitives, per-element reduce, final;
    mr_point_mesh_face_forward), one memset and two launches backward (mr_point_mesh_face_backward). Returns a 0-dim
    tensor, differentiable w.r.t. points and verts; bitwise reproducible."""

    @staticmethod
    def forward(ctx, points, verts, batch, min_triangle_area):
        pf, vf, args, keep = _pm_args(points, verts, batch, min_triangle_area)
        L = _lib.load()
        dev = pf.device
        N, P, T = batch.N, pf.shape[0], batch.faces.shape[0]
        want = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        out = torch.empty(1, device=dev)
        ip = torch.empty(P, dtype=torch.int32, device=dev) if want else None
        it = torch.empty(T, dtype=torch.int32, device=dev) if want else None
        coef = torch.empty((2, N), device=dev) if want else None
        ws, wsb = _workspace(L.mr_point_mesh_face_workspace, dev, N, P, T,
                             what="mi355r: point-mesh face distance: more than 65535 meshes or a batch too large "
                                  "for 32-bit indices")
        check(L.mr_point_mesh_face_forward(*args, ptr(ip), ptr(it), ptr(coef), ptr(out), ptr(ws), wsb,
                                           _lib.stream_handle(dev)))
        ctx.set_materialize_grads(False)
        if want:
            ctx.save_for_backward(*keep, ip, it, coef)
            ctx.args = (args[4], args[11], N, args[13], points.dtype, verts.dtype)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        pf, vf, faces, p1, pc, f1, fc, ip, it, coef = ctx.saved_tensors
        maxp, maxf, N, area, pdt, vdt = ctx.args
        g = g.detach().float().reshape(1).contiguous()
        _require_cuda(g)
        args = (ptr(pf), pf.shape[0], ptr(p1), ptr(pc), maxp, ptr(vf), vf.shape[0], ptr(faces), faces.shape[0], ptr(f1),
                ptr(fc), maxf, N, area)
        gp, gv = _pm_backward((pf, vf), args, ip, it, coef, g, None, None)
        return gp.to(pdt), gv.to(vdt), None, None


class PointFaceDistances(torch.autograd.Function):
    """The unreduced distances of one direction over the same kernels: ``direction`` 0 every point's squared distance
    to its nearest face (P,), 1 every face's to its nearest point (T,). The backward takes the per-distance upstream
    gradient (mr_point_mesh_face_backward's grad_dist_p / grad_dist_f)."""

    @staticmethod
    def forward(ctx, points, verts, batch, min_triangle_area, direction):
        want = (direction == 0, direction == 0, direction == 1, direction == 1)
        outs, keep = _pm_nearest(points, verts, batch, min_triangle_area, want)
        ctx.set_materialize_grads(False)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(*keep, outs[1 + 2 * direction])
            ctx.args = (int(batch.max_points), int(batch.max_faces), batch.N, float(min_triangle_area), direction,
                        points.dtype, verts.dtype)
        ctx.mark_non_differentiable(outs[1 + 2 * direction])
        return outs[2 * direction], outs[1 + 2 * direction]

    @staticmethod
    def backward(ctx, g, _gi):
        if g is None:
            return None, None, None, None, None
        pf, vf, faces, p1, pc, f1, fc, idx = ctx.saved_tensors
        maxp, maxf, N, area, direction, pdt, vdt = ctx.args
        g = g.detach().float().contiguous()
        _require_cuda(g)
        args = (ptr(pf), pf.shape[0], ptr(p1), ptr(pc), maxp, ptr(vf), vf.shape[0], ptr(faces), faces.shape[0], ptr(f1),
                ptr(fc), maxf, N, area)
        if direction == 0:
            gp, gv = _pm_backward((pf, vf), args, idx, None, None, None, g, None)
        else:
            gp, gv = _pm_backward((pf, vf), args, None, idx, None, None, None, g)
        return gp.to(pdt), gv.to(vdt), None, None, None


# Iterations enqueued between two reads of the device status: a read costs ~14 us, an iteration enqueued after
# convergence ~18 us (tools/icp_bench.py, DESIGN.md §3, ICP)
ICP_STATUS_BATCH = 8


def points_alignment(x, y, lengths=None, weights=None, flags=0, eps=1e-9):
    """rts (N,13) float32 = (R row-major, T, s) per cloud of the similarity transform taking x (N,P,3) to y (N,P,3):
    three launches, nothing read back (mr_points_alignment). weights (N,P) and lengths (N) may be None."""
    xf, yf, xl, _, N, P, _ = _cloud_args(x, y, lengths, None, 2)
    _require_cuda(weights)
    w = None if weights is None else weights.detach().float().contiguous()
    L = _lib.load()
    dev = xf.device
    rts = torch.empty((N, 13), device=dev)
    ws, wsb = _workspace(L.mr_points_alignment_workspace, dev, N, P)
    check(L.mr_points_alignment(ptr(xf), ptr(yf), N, P, ptr(xl), ptr(w), int(flags), float(eps), ptr(rts), ptr(ws),
                                wsb, _lib.stream_handle(dev)))
    return rts


def similarity_transform(x, rts):
    """s (x R) + T for every entry of x (N,P,3) with the library's transform code (mr_icp_transform)."""
    _require_cuda(x, rts)
    xf = x.detach().float().contiguous()
    out = torch.empty_like(xf)
    check(_lib.load().mr_icp_transform(ptr(xf), xf.shape[0], xf.shape[1], ptr(rts), ptr(out),
                                       _lib.stream_handle(xf.device)))
    return out


def _icp_loop(xf, xl, N, P1, P2, init, max_iterations, status_batch, workspace_query, iterate, prepare=None):
    """What icp, icp_plane and icp_mesh share: mr_icp_init on a workspace of ``workspace_query`` bytes,
    ``prepare(ws, wsb, st)`` where the estimator has something to set up once, then
    ``iterate(k, rts, hist, rmse, status, ws, wsb, st)`` (the estimator's entry point for k more iterations) in batches
    of ``status_batch`` with one read of the two device status words after each, then mr_icp_transform."""
    L = _lib.load()
    dev = xf.device
    st = _lib.stream_handle(dev)
    R0 = T0 = s0 = None
    if init is not None:
        _require_cuda(*init)
        R0, T0, s0 = (t.detach().float().contiguous() for t in init)
    max_iterations = int(max_iterations)
    rts = torch.empty((N, 13), device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    ws, wsb = _workspace(workspace_query, dev, N, P1, P2)
    check(L.mr_icp_init(ptr(xf), N, P1, P2, ptr(xl), ptr(R0), ptr(T0), ptr(s0), ptr(rts), ptr(status), ptr(ws), wsb, st))
    if prepare is not None:
        check(prepare(ptr(ws), wsb, st))
    done, iters, rmse = 0, 0, None
    hist = torch.empty((max(max_iterations, 0), N, 13), device=dev)
    if max_iterations > 0:
        rmse = torch.empty(N, device=dev)
        batch = max(int(status_batch or ICP_STATUS_BATCH), 1)
        left = max_iterations
        while left > 0 and not done:
            k = min(batch, left)
            check(iterate(k, ptr(rts), ptr(hist), ptr(rmse), ptr(status), ptr(ws), wsb, st))
            left -= k
            done, iters = status.tolist()  # the one synchronisation of a batch
    xt = torch.empty_like(xf)
    check(L.mr_icp_transform(ptr(xf), N, P1, ptr(rts), ptr(xt), st))
    return bool(done), iters, rmse, xt, rts, hist[:iters]


def _icp_grid_args(who, grid, visited, N, P2):
    """The checked grid arguments of icp / icp_plane: (grid, its size in bytes, visited)."""
    if not torch.is_tensor(grid):
        raise ValueError(f"{who}: grid is the buffer tensor of point_grid_build")
    _require_cuda(grid, visited)
    gb = _ws_size(_lib.load().mr_point_grid_bytes, N, P2)
    if grid.dtype != torch.uint8 or grid.numel() != gb or gb == 0 or not grid.is_contiguous():
        raise ValueError(f"{who}: the grid buffer was not built for a target batch of this shape")
    if visited is not None and (visited.dtype != torch.int64 or visited.numel() != 1):
        raise ValueError(f"{who}: visited must be one int64")
    return grid, gb, visited


def icp(x, y, x_lengths=None, y_lengths=None, init=None, max_iterations=100, relative_rmse_thr=1e-6, flags=0,
        status_batch=None, grid=None, visited=None):
    """The ICP loop on the device (mr_icp_*): (converged, iterations run, rmse (N) or None, Xt (N,P1,3), rts (N,13),
    history (iterations,N,13)). ``init`` = (R (N,3,3), T (N,3), s (N)) or None. The host enqueues ``status_batch``
    iterations at a time (default ICP_STATUS_BATCH) and reads two status words between the batches; the results do
    not depend on that size.

    ``grid`` = point_grid_build(y, y_lengths) runs every iteration's neighbour search through that index
    (mr_icp_iterate_grid) with the same results bit for bit; ``visited`` (one int64 on the device, cleared by the
    caller; only with a grid) gains the number of distances the iterations that ran evaluated. A grid of other
    clouds of the same shape gives wrong correspondences, inside the target."""
    xf, yf, xl, yl, N, P1, P2 = _cloud_args(x, y, x_lengths, y_lengths, 2)
    L = _lib.load()
    head = (ptr(xf), ptr(yf), N, P1, P2, ptr(xl), ptr(yl))
    tail = (int(flags), float(relative_rmse_thr), int(max_iterations))
    if grid is None:
        if visited is not None:
            raise ValueError("icp: visited counts the distances of a search through a grid")

        def iterate(k, *state):
            return L.mr_icp_iterate(*head, *tail, k, *state)
    else:
        grid, gb, visited = _icp_grid_args("icp", grid, visited, N, P2)

        def iterate(k, rts, hist, rmse, status, *ws):
            return L.mr_icp_iterate_grid(*head, ptr(grid), gb, *tail, k, rts, hist, rmse, status, ptr(visited), *ws)

    return _icp_loop(xf, xl, N, P1, P2, init, max_iterations, status_batch, L.mr_icp_workspace, iterate)


def icp_plane(x, y, y_normals, x_lengths=None, y_lengths=None, init=None, max_iterations=100, relative_rmse_thr=1e-6,
              max_correspondence_distance=None, status_batch=None, grid=None, visited=None):
    """The point-to-plane ICP loop on the device (mr_icp_plane_iterate, whose rule include/mi355r.h states), shaped
    like ``icp``: (converged, iterations run, rmse (N) or None, Xt (N,P1,3), rts (N,13), history (iterations,N,13)).
    ``y_normals`` (N,P2,3) are read as float32 and used as given; ``max_correspondence_distance`` d (None: no limit)
    reaches the kernels as float32(d) * float32(d) rounded once to float32. The scale of ``init`` stays fixed. The
    results do not depend on ``status_batch``. ``grid`` and ``visited`` as in ``icp`` (mr_icp_plane_iterate_grid);
    through a grid, a source point's walk also ends where no unvisited cell can hold a target within d."""
    xf, yf, xl, yl, N, P1, P2 = _cloud_args(x, y, x_lengths, y_lengths, 2)
    if tuple(y_normals.shape) != tuple(yf.shape):
        raise ValueError("y_normals must have y's padded shape (N, P2, 3)")
    _require_cuda(y_normals)
    nf = y_normals.detach().float().contiguous()
    r2 = float("inf") if max_correspondence_distance is None else \
        float(np.float32(max_correspondence_distance) * np.float32(max_correspondence_distance))
    L = _lib.load()
    head = (ptr(xf), ptr(yf), ptr(nf), N, P1, P2, ptr(xl), ptr(yl))
    tail = (r2, float(relative_rmse_thr), int(max_iterations))
    if grid is None:
        if visited is not None:
            raise ValueError("icp_plane: visited counts the distances of a search through a grid")

        def iterate(k, *state):
            return L.mr_icp_plane_iterate(*head, *tail, k, *state)
    else:
        grid, gb, visited = _icp_grid_args("icp_plane", grid, visited, N, P2)

        def iterate(k, rts, hist, rmse, status, *ws):
            return L.mr_icp_plane_iterate_grid(*head, ptr(grid), gb, *tail, k, rts, hist, rmse, status, ptr(visited),
                                               *ws)

    return _icp_loop(xf, xl, N, P1, P2, init, max_iterations, status_batch, L.mr_icp_plane_workspace, iterate)


def _icp_mesh_args(x, verts, batch, x_lengths, min_triangle_area, who):
    """The checked inputs of a cloud-to-mesh call: contiguous float32 x (N,P1,3) and verts (V,3), the int64 lengths,
    and the packed mesh arguments of the C ABI taken from ``batch`` (a PointMeshBatch, whose points_* fields are not
    read here)."""
    if x.dim() != 3:
        raise ValueError(f"{who}: x must be an (N, P, D) tensor")
    if verts.dim() != 2 or batch.faces.dim() != 2 or batch.faces.shape[1] != 3:
        raise ValueError(f"{who}: verts (V, D) and faces (T, 3) are packed 2-D tensors")
    if x.shape[2] != 3 or verts.shape[1] != 3:
        raise NotImplementedError(f"{who}: only D = 3 is built")
    N, P1 = int(x.shape[0]), int(x.shape[1])
    if N < 1 or P1 < 1:
        raise ValueError(f"{who}: N and P1 must be >= 1")
    for t in (batch.faces_first, batch.faces_count) + (() if x_lengths is None else (x_lengths,)):
        if tuple(t.shape) != (N,):
            raise ValueError(f"{who}: faces_first, faces_count and the lengths must all be of shape (N,)")
    if not float(min_triangle_area) >= 0.0:
        raise ValueError(f"{who}: min_triangle_area must be >= 0")
    _require_cuda(x, verts, batch.faces, batch.faces_first, batch.faces_count, x_lengths)
    xf, vf = x.detach().float().contiguous(), verts.detach().float().contiguous()
    faces = batch.faces.detach().to(torch.int32).contiguous()
    ff, fc = (t.detach().to(torch.int64).contiguous() for t in (batch.faces_first, batch.faces_count))
    xl = None if x_lengths is None else x_lengths.detach().to(torch.int64).contiguous()
    T = int(faces.shape[0])
    mesh = (T, ptr(ff), ptr(fc), min(max(int(batch.max_faces), 0), T))
    return xf, vf, faces, xl, N, P1, mesh, (ff, fc)


def _icp_mesh_prepare(L, vf, faces, mesh, N, P1, min_triangle_area):
    T, ff, fc, max_faces = mesh
    return lambda ws, wsb, st: L.mr_icp_mesh_prepare(ptr(vf), vf.shape[0], ptr(faces), T, ff, fc, max_faces, N, P1,
                                                     float(min_triangle_area), ws, wsb, st)


def icp_mesh(x, verts, batch, x_lengths=None, init=None, max_iterations=100, relative_rmse_thr=1e-6,
             max_correspondence_distance=None, min_triangle_area=0.0, status_batch=None):
    """The cloud-to-mesh ICP loop on the device (mr_icp_mesh_*, whose rule include/mi355r.h states), shaped like
    ``icp_plane``: (converged, iterations run, rmse (N) or None, Xt (N,P1,3), rts (N,13), history (iterations,N,13)).
    x (N,P1,3) with ``x_lengths``; cloud n registers onto mesh n of ``batch`` (a PointMeshBatch: faces (T,3) over the
    packed ``verts`` (V,3), faces_first / faces_count (N), max_faces; meshes may share faces).
    ``max_correspondence_distance`` d (None: no limit) reaches the kernels as float32(d) * float32(d) rounded once.
    The triangle records are built once per call; the scale of ``init`` stays fixed. The results do not depend on
    ``status_batch``."""
    if max_correspondence_distance is not None and not float(max_correspondence_distance) >= 0.0:
        raise ValueError("icp_mesh: max_correspondence_distance must be >= 0")
    r2 = float("inf") if max_correspondence_distance is None else \
        float(np.float32(max_correspondence_distance) * np.float32(max_correspondence_distance))
    xf, vf, faces, xl, N, P1, mesh, keep = _icp_mesh_args(x, verts, batch, x_lengths, min_triangle_area, "icp_mesh")
    L = _lib.load()
    T = mesh[0]

    def iterate(k, *state):
        return L.mr_icp_mesh_iterate(ptr(xf), N, P1, ptr(xl), *mesh[:4], r2, float(relative_rmse_thr),
                                     int(max_iterations), k, *state)

    # the loop's third size is the face count here (at least 1: mr_icp_init wants a target; the workspace of one face
    # serves a batch without faces)
    return _icp_loop(xf, xl, N, P1, max(T, 1), init, max_iterations, status_batch, L.mr_icp_mesh_workspace, iterate,
                     _icp_mesh_prepare(L, vf, faces, mesh, N, P1, min_triangle_area))


def mesh_closest_points(x, verts, batch, rts=None, min_triangle_area=0.0):
    """(dist (N,P1), face idx (N,P1) int32, q (N,P1,3), n (N,P1,3)) of x (N,P1,3) under ``rts`` (N,13; None: as it is)
    against the meshes of ``batch``: the cloud-to-mesh loop's scan and closest-point code, run once
    (mr_icp_mesh_prepare + mr_icp_mesh_closest). dist / idx are point_face_nearest's for the transformed points; q the
    closest surface point; n the unit gradient direction of the distance function there (zero where p lies on the
    surface); rows past ``batch.points_count`` (None: every row counts) or without a face get 0 / -1 / 0 / 0. For
    tests and tools; nothing synchronises."""
    xf, vf, faces, xl, N, P1, mesh, keep = _icp_mesh_args(x, verts, batch, batch.points_count, min_triangle_area,
                                                          "mesh_closest_points")
    L = _lib.load()
    dev = xf.device
    st = _lib.stream_handle(dev)
    if rts is not None:
        _require_cuda(rts)
        if tuple(rts.shape) != (N, 13):
            raise ValueError("mesh_closest_points: rts must be (N, 13)")
        rts = rts.detach().float().contiguous()
    ws, wsb = _workspace(L.mr_icp_mesh_workspace, dev, N, P1, mesh[0])
    check(_icp_mesh_prepare(L, vf, faces, mesh, N, P1, min_triangle_area)(ptr(ws), wsb, st))
    dist = torch.empty((N, P1), device=dev)
    idx = torch.empty((N, P1), dtype=torch.int32, device=dev)
    q, n = torch.empty((N, P1, 3), device=dev), torch.empty((N, P1, 3), device=dev)
    check(L.mr_icp_mesh_closest(ptr(xf), N, P1, ptr(xl), ptr(rts), *mesh[:4], ptr(dist), ptr(idx), ptr(q), ptr(n),
                                ptr(ws), wsb, st))
    return dist, idx, q, n


def _mesh_args(verts, faces):
    _require_cuda(verts, faces)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("verts must be (V, 3) and faces (F, 3)")
    return verts.detach().float().contiguous(), faces.detach().to(torch.int32).contiguous()


def face_areas(verts, faces):
    """(F,) float32 areas 0.5 |(b - a) x (c - a)| of the packed faces (F,3) over verts (V,3); one launch, no
    autograd (mr_face_areas)."""
    v, f = _mesh_args(verts, faces)
    areas = torch.empty(f.shape[0], device=v.device)
    check(_lib.load().mr_face_areas(ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(areas), _lib.stream_handle(v.device)))
    return areas


class SamplePoints(torch.autograd.Function):
    """Points (N,S,3) on the packed faces (F,3) of verts (V,3): face ``face_idx`` (N,S) (negative: a row of zeros)
    at the barycentric coordinates of ``uv`` (2,N,S) in [0,1) (upstream's _rand_barycentric_coords). One launch
    forward (mr_sample_points_forward); the backward sums into the vertices with fixed-point integer atomics
    (mr_sample_points_backward: a memset and two launches, bitwise reproducible). Differentiable w.r.t. verts."""

    @staticmethod
    def forward(ctx, verts, faces, face_idx, uv):
        v, f = _mesh_args(verts, faces)
        _require_cuda(face_idx, uv)
        if face_idx.dim() != 2 or tuple(uv.shape) != (2,) + tuple(face_idx.shape):
            raise ValueError("face_idx must be (N, S) and uv (2, N, S)")
        fi = face_idx.detach().to(torch.int32).contiguous()
        uvf = uv.detach().float().contiguous()
        M = fi.numel()
        pts = torch.empty(tuple(fi.shape) + (3,), device=v.device)
        check(_lib.load().mr_sample_points_forward(ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(fi), ptr(uvf), M,
                                                   ptr(pts), _lib.stream_handle(v.device)))
        ctx.set_materialize_grads(False)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(f, fi, uvf)
            ctx.args = (v.shape[0], verts.dtype)
        return pts

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        f, fi, uvf = ctx.saved_tensors
        V, dtype = ctx.args
        g = g.detach().float().contiguous()
        _require_cuda(g)
        L = _lib.load()
        gv = torch.empty((V, 3), device=g.device)
        ws, wsb = _workspace(L.mr_sample_points_backward_workspace, g.device, V)
        check(L.mr_sample_points_backward(V, ptr(f), f.shape[0], ptr(fi), ptr(uvf), fi.numel(), ptr(g), ptr(gv),
                                          ptr(ws), wsb, _lib.stream_handle(g.device)))
        return gv.to(dtype), None, None, None


def raster_settings_struct(H, W, K=1, blur=0.0, persp=True, clip=False, cull=False, max_faces_per_bin=None,
                           z_clip=None):
    """mr_raster_settings_t; z_clip = z_clip_value of the near-plane clip (None: no clipping)."""
    s = MrRasterSettings()
    s.H, s.W, s.faces_per_pixel = int(H), int(W), int(K)
    s.blur_radius = float(blur)
    s.perspective_correct = int(bool(persp))
    s.clip_barycentric_coords = int(bool(clip))
    s.cull_backfaces = int(bool(cull))
    s.max_faces_per_bin = int(max_faces_per_bin or 0)
    s.clip_z = 0 if z_clip is None else 1
    s.z_clip_value = 0.0 if z_clip is None else float(z_clip)
    return s


# --------------------------------------------------------------------------- rasterize (PyTorch3D _C boundary)
def rasterize_meshes_fwd(face_verts, first, count, H, W, K=1, blur=0.0, persp=True, clip=False, cull=False,
                         max_faces_per_bin=None, z_clip=None):
    _require_cuda(face_verts, first, count)
    L = _lib.load()
    fv = face_verts.detach().float().contiguous()
    first = first.to(torch.int64).contiguous()
    count = count.to(torch.int64).contiguous()
    N = first.numel()
    Ftot = fv.shape[0]
    s = raster_settings_struct(H, W, K, blur, persp, clip, cull, max_faces_per_bin, z_clip)
    dev = fv.device
    p2f = torch.empty((N, H, W, K), dtype=torch.int64, device=dev)
    zbuf = torch.empty((N, H, W, K), dtype=torch.float32, device=dev)
    bary = torch.empty((N, H, W, K, 3), dtype=torch.float32, device=dev)
    dists = torch.empty((N, H, W, K), dtype=torch.float32, device=dev)
    wsb = L.mr_rasterize_meshes_workspace(N, max(Ftot, 1), H, W, s.max_faces_per_bin)
    ws = torch.empty(int(wsb), dtype=torch.uint8, device=dev)
    check(L.mr_rasterize_meshes(ptr(fv), ptr(first), ptr(count), N, Ftot, ctypes.byref(s), ptr(p2f), ptr(zbuf),
                                ptr(bary), ptr(dists), ptr(ws), wsb, _lib.stream_handle(dev)))
    return p2f, zbuf, bary, dists


def rasterize_meshes_bwd(face_verts, p2f, gz, gb, gd, H, W, K=1, persp=True, clip=False, blur=0.0, cull=False,
                         z_clip=None):
    L = _lib.load()
    fv = face_verts.detach().float().contiguous()
    N = p2f.shape[0]
    s = raster_settings_struct(H, W, K, blur, persp, clip, cull, None, z_clip)
    g = torch.empty_like(fv)
    # a gradient PyTorch passed as None goes down as NULL (zero) instead of a zero-filled tensor
    gz, gb, gd = (None if t is None else t.float().contiguous() for t in (gz, gb, gd))
    check(L.mr_rasterize_meshes_backward(ptr(fv), ptr(p2f.contiguous()), ptr(gz), ptr(gb), ptr(gd),
                                         N, fv.shape[0], ctypes.byref(s), ptr(g), _lib.stream_handle(fv.device)))
    return g


class RasterizeFaceVerts(torch.autograd.Function):
    """Drop-in for PyTorch3D's _RasterizeFaceVerts (upstream mesh/rasterize_meshes.py)."""

    @staticmethod
    def forward(ctx, face_verts, first, count, H, W, K, blur, persp, clip, cull, mfpb, z_clip=None):
        ctx.set_materialize_grads(False)  # no zero-filled int64 grad for pix_to_face, none for unused outputs
        p2f, zbuf, bary, dists = rasterize_meshes_fwd(face_verts, first, count, H, W, K, blur, persp, clip, cull,
                                                      mfpb, z_clip)
        ctx.save_for_backward(face_verts, p2f)
        ctx.cfg = (H, W, K, persp, clip, blur, cull, z_clip)
        ctx.mark_non_differentiable(p2f)
        return p2f, zbuf, bary, dists

    @staticmethod
    def backward(ctx, _gp, gz, gb, gd):
        fv, p2f = ctx.saved_tensors
        H, W, K, persp, clip, blur, cull, z_clip = ctx.cfg
        g = rasterize_meshes_bwd(fv, p2f, gz, gb, gd, H, W, K, persp, clip, blur, cull, z_clip)
        return (g,) + (None,) * 11


# --------------------------------------------------------------------------- projection
def make_views(R, T, intr):
    """(N,16) view records: R (N,3,3) row-vector convention, T (N,3), intr (N,4) = ax,bx,ay,by."""
    return torch.cat([R.reshape(-1, 9), T.reshape(-1, 3), intr.reshape(-1, 4)], dim=1).float().contiguous()


def _batch_stride(t):
    """(float tensor whose per-view rows are contiguous, elements between views; 0 = broadcast)."""
    t = t.float()
    if t.stride(-1) != 1 or (t.dim() == 3 and t.stride(-2) != 3):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else 0)


def views_from_opencv(R_cv, t_cv, intr, N):
    """mr_views_from_opencv: (N,16) view records straight from OpenCV poses (one launch instead
    of the transpose/sign multiplies and the packing concatenation)."""
    R, sR = _batch_stride(R_cv.detach().reshape(-1, 3, 3))
    t, sT = _batch_stride(t_cv.detach().reshape(-1, 3))
    it, sI = _batch_stride(intr.reshape(-1, 4))
    views = torch.empty((N, 16), device=R.device)
    sp = _lib.strided_ptr
    check(_lib.load().mr_views_from_opencv(sp(R), sR, sp(t), sT, sp(it), sI, N, ptr(views),
                                           _lib.stream_handle(R.device)))
    return views


def _project_backward(v, f, vptr, vadj, views, gfv, vert_first=None, max_verts=0):
    """(grad verts, grad R, grad T) of the projection from the face_verts gradient: mr_project_faces_backward, or
    with vert_first (each view's first union vertex) mr_project_faces_meshes_backward."""
    L = _lib.load()
    N = views.shape[0]
    gv = torch.empty_like(v)
    gviews = torch.empty((N, 12), device=v.device)
    mesh = (ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(vptr), ptr(vadj))
    tail = (ptr(views), N, ptr(gfv.float().contiguous()), ptr(gv), ptr(gviews), _lib.stream_handle(v.device))
    if vert_first is None:
        check(L.mr_project_faces_backward(*mesh, *tail))
    else:
        check(L.mr_project_faces_meshes_backward(*mesh, ptr(vert_first), max_verts, *tail))
    return gv, gviews[:, :9].reshape(N, 3, 3), gviews[:, 9:12]


class ProjectFaces(torch.autograd.Function):
    """MeshRasterizer.transform + verts_packed()[faces_packed] for one mesh shared by N views."""

    @staticmethod
    def forward(ctx, verts, R, T, faces, intr):
        _require_cuda(verts, R, T, faces)
        L = _lib.load()
        v = verts.detach().float().contiguous()
        f, vptr, vadj = mesh_topology(faces, v.shape[0])
        views = make_views(R.detach(), T.detach(), intr)
        N = views.shape[0]
        out = torch.empty((N * f.shape[0], 3, 3), device=v.device, dtype=torch.float32)
        check(L.mr_project_faces(ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(views), N, ptr(out),
                                 _lib.stream_handle(v.device)))
        ctx.save_for_backward(v, f, views, vptr, vadj)
        return out

    @staticmethod
    def backward(ctx, g):
        v, f, views, vptr, vadj = ctx.saved_tensors
        return _project_backward(v, f, vptr, vadj, views, g) + (None, None)


class ProjectFacesMeshes(torch.autograd.Function):
    """MeshRasterizer.transform for a batch of N distinct meshes (view n projects mesh n): verts /
    faces are the meshes' union, face_verts rows are the packed face ids; one launch each way
    (mr_project_faces_meshes / _backward)."""

    @staticmethod
    def forward(ctx, verts, R, T, faces, intr, face_first, max_faces, vert_first, max_verts):
        _require_cuda(verts, R, T, faces)
        L = _lib.load()
        v = verts.detach().float().contiguous()
        f, vptr, vadj = mesh_topology(faces, v.shape[0])
        views = make_views(R.detach(), T.detach(), intr)
        N = views.shape[0]
        out = torch.empty((f.shape[0], 3, 3), device=v.device, dtype=torch.float32)
        check(L.mr_project_faces_meshes(ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(face_first), int(max_faces),
                                        ptr(views), N, ptr(out), _lib.stream_handle(v.device)))
        ctx.save_for_backward(v, f, views, vptr, vadj, vert_first)
        ctx.max_verts = int(max_verts)
        return out

    @staticmethod
    def backward(ctx, g):
        v, f, views, vptr, vadj, vert_first = ctx.saved_tensors
        return _project_backward(v, f, vptr, vadj, views, g, vert_first, ctx.max_verts) + (None,) * 6


def _poses_struct(R, T, intr):
    """mr_poses_t over (N,3,3) R, (N,3) T, (N,4) intr (a batch stride of 0 broadcasts one row);
    returns the struct and the tensors it points into (keep them alive for the call)."""
    R, sR = _batch_stride(R.detach().reshape(-1, 3, 3))
    T, sT = _batch_stride(T.detach().reshape(-1, 3))
    it, sI = _batch_stride(intr.reshape(-1, 4))
    sp = _lib.strided_ptr
    return _lib.MrPoses(sp(R).value, sR, sp(T).value, sT, sp(it).value, sI), (R, T, it)


def _world_inputs(verts, R, T, faces, intr, N, H, W, K, blur, persp, clip, cull, mfpb, z_clip):
    """What a *World forward passes down: v float (V,3), the topology (f, vptr, vadj), mr_poses_t and the tensors it
    points into, mr_raster_settings_t, and the views (N,16) / face_verts (N F,3,3) buffers the call writes."""
    _require_cuda(verts, R, T, faces, intr)
    v = verts.detach().float().contiguous()
    f, vptr, vadj = mesh_topology(faces, v.shape[0])
    ps, keep = _poses_struct(R, T, intr)
    s = raster_settings_struct(H, W, K, blur, persp, clip, cull, mfpb, z_clip)
    views = torch.empty((N, 16), device=v.device)
    fv = torch.empty((N * f.shape[0], 3, 3), device=v.device)
    return v, f, vptr, vadj, ps, keep, s, views, fv


class RasterizeMeshesWorld(torch.autograd.Function):
    """MeshRasterizer.transform + _RasterizeFaceVerts for one mesh shared by N views, in one
    native call (mr_rasterize_meshes_world): the projection runs inside the binning's first launch,
    which also writes face_verts (saved for the backward) and the view records. Results are bitwise
    those of ProjectFaces.apply followed by RasterizeFaceVerts.apply; the backward is
    mr_rasterize_meshes_backward followed by mr_project_faces_backward."""

    @staticmethod
    def forward(ctx, verts, R, T, faces, intr, N, H, W, K, blur, persp, clip, cull, mfpb, z_clip=None):
        ctx.set_materialize_grads(False)  # no zero-filled int64 grad for pix_to_face, none for unused outputs
        L = _lib.load()
        N = int(N)
        v, f, vptr, vadj, ps, keep, s, views, fv = _world_inputs(verts, R, T, faces, intr, N, H, W, K, blur, persp,
                                                                 clip, cull, mfpb, z_clip)
        Fn, dev = f.shape[0], v.device
        p2f = torch.empty((N, H, W, K), dtype=torch.int64, device=dev)
        zbuf = torch.empty((N, H, W, K), dtype=torch.float32, device=dev)
        bary = torch.empty((N, H, W, K, 3), dtype=torch.float32, device=dev)
        dists = torch.empty((N, H, W, K), dtype=torch.float32, device=dev)
        wsb = L.mr_rasterize_meshes_world_workspace(N, Fn, H, W, s.max_faces_per_bin)
        ws = torch.empty(int(wsb), dtype=torch.uint8, device=dev)
        check(L.mr_rasterize_meshes_world(ptr(v), v.shape[0], ptr(f), Fn, ctypes.byref(ps), N, ctypes.byref(s),
                                          ptr(views), ptr(fv), ptr(p2f), ptr(zbuf), ptr(bary), ptr(dists), ptr(ws),
                                          wsb, _lib.stream_handle(dev)))
        del keep
        ctx.save_for_backward(v, f, views, vptr, vadj, fv, p2f)
        ctx.cfg = (H, W, K, persp, clip, blur, cull, z_clip)
        ctx.mark_non_differentiable(p2f)
        return p2f, zbuf, bary, dists

    @staticmethod
    def backward(ctx, _gp, gz, gb, gd):
        v, f, views, vptr, vadj, fv, p2f = ctx.saved_tensors
        H, W, K, persp, clip, blur, cull, z_clip = ctx.cfg
        gfv = rasterize_meshes_bwd(fv, p2f, gz, gb, gd, H, W, K, persp, clip, blur, cull, z_clip)
        return _project_backward(v, f, vptr, vadj, views, gfv) + (None,) * 12


class SoftSilhouetteWorld(torch.autograd.Function):
    """MeshRenderer(MeshRasterizer(faces_per_pixel = K > 1), SoftSilhouetteShader) for one mesh shared by N
    views in one native pass (mr_soft_silhouette_forward / _backward; deform_mesh_with_color.py:153-165):
    the K-deep fragments are blended as the raster produces them and never written. Bitwise
    RasterizeMeshesWorld + ShadeFragments(silhouette) in the forward; the backward chains the blend's
    distance gradients straight into the rasterizer's backward (no fragment-gradient tensors), then
    mr_project_faces_backward as RasterizeMeshesWorld does. Returns rgba (N,H,W,4)."""

    @staticmethod
    def forward(ctx, verts, R, T, faces, intr, N, H, W, K, blur, persp, clip, cull, mfpb, z_clip, sigma):
        L = _lib.load()
        N = int(N)
        v, f, vptr, vadj, ps, keep, s, views, fv = _world_inputs(verts, R, T, faces, intr, N, H, W, K, blur, persp,
                                                                 clip, cull, mfpb, z_clip)
        Fn, dev = f.shape[0], v.device
        rgba = torch.tensor([1.0, 1.0, 1.0, 0.0], device=dev).expand(N, H, W, 4).contiguous()  # background
        wsb = L.mr_soft_silhouette_workspace(N, Fn, H, W, K, s.max_faces_per_bin)
        ws = torch.empty(int(wsb), dtype=torch.uint8, device=dev)
        check(L.mr_soft_silhouette_forward(ptr(v), v.shape[0], ptr(f), Fn, ctypes.byref(ps), N, ctypes.byref(s),
                                           float(sigma), ptr(views), ptr(fv), ptr(rgba), ptr(ws), wsb,
                                           _lib.stream_handle(dev)))
        del keep
        ctx.save_for_backward(v, f, views, vptr, vadj, fv, ws)
        ctx.cfg = (H, W, K, persp, clip, blur, cull, mfpb, z_clip, float(sigma))
        return rgba

    @staticmethod
    def backward(ctx, g):
        v, f, views, vptr, vadj, fv, ws = ctx.saved_tensors
        H, W, K, persp, clip, blur, cull, mfpb, z_clip, sigma = ctx.cfg
        L = _lib.load()
        N = views.shape[0]
        dev = v.device
        s = raster_settings_struct(H, W, K, blur, persp, clip, cull, mfpb, z_clip)
        gfv = torch.empty_like(fv)
        check(L.mr_soft_silhouette_backward(ptr(fv), N, f.shape[0], ctypes.byref(s), sigma,
                                            ptr(g.float().contiguous()), ptr(ws), ptr(gfv), _lib.stream_handle(dev)))
        return _project_backward(v, f, vptr, vadj, views, gfv) + (None,) * 13


def vertex_normals(verts, faces):
    """(normals, raw sums) — Meshes.verts_normals_packed on the GPU (no autograd)."""
    _require_cuda(verts, faces)
    v = verts.detach().float().contiguous()
    f, vptr, vadj = mesh_topology(faces, v.shape[0])
    return _vertex_normals(v, f, vptr, vadj)


def _vertex_normals(v, f, vptr, vadj):
    L = _lib.load()
    vn = torch.empty_like(v)
    raw = torch.empty_like(v)
    check(L.mr_vertex_normals(ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(vptr), ptr(vadj), ptr(vn), ptr(raw),
                              _lib.stream_handle(v.device)))
    return vn, raw


# --------------------------------------------------------------------------- fused render
_STRUCT_CACHE: dict = {}  # ShadeConfig values -> its ctypes structs' bytes (per-call host work of the eager loops)
_WS_CACHE: dict = {}      # workspace-size queries by their arguments


def _ws_size(fn, *args):
    k = (fn.__name__,) + args
    v = _WS_CACHE.get(k)
    if v is None:
        if len(_WS_CACHE) > 256:
            _WS_CACHE.clear()
        v = _WS_CACHE[k] = int(fn(*args))
    return v


def _workspace(fn, device, *shape, what=None):
    """(ws, wsb): a uint8 workspace of the ``fn(*shape)`` bytes on ``device``, and that size. With ``what``, a size of
    0 (the library's answer to shapes it does not take) raises NotImplementedError(what)."""
    wsb = _ws_size(fn, *shape)
    if what is not None and wsb == 0:
        raise NotImplementedError(what)
    return torch.empty(wsb, dtype=torch.uint8, device=device), wsb


@dataclass
class ShadeConfig:
    """Static (non-differentiable) configuration of one fused render call."""
    H: int
    W: int
    persp: bool = True
    blur: float = 0.0
    clip: bool = False
    cull: bool = False
    max_faces_per_bin: int | None = None
    light_kind: int = 0  # 0 point, 1 ambient
    light_location: tuple = (0.0, 0.0, -3.0)
    light_ambient: tuple = (0.5, 0.5, 0.5)
    light_diffuse: tuple = (0.3, 0.3, 0.3)
    light_specular: tuple = (0.2, 0.2, 0.2)
    mat_ambient: tuple = (1.0, 1.0, 1.0)
    mat_diffuse: tuple = (1.0, 1.0, 1.0)
    mat_specular: tuple = (1.0, 1.0, 1.0)
    shininess: float = 64.0
    sigma_rgb: float = 1e-4
    gamma: float = 1e-4
    background: tuple = (1.0, 1.0, 1.0)
    znear: float = 1.0
    zfar: float = 100.0
    sigma_sil: float = 1e-4
    want_depth: bool = True
    want_sil: bool = True
    want_rgb: bool = True
    rgb_channels: int = 3
    want_p2f: bool = False  # also return the (N,H,W) int32 packed face ids (tests / tools)
    hard: bool = False  # hard_rgb_blend (HardPhongShader): fragment-shader path only
    sil_rgba: bool = False  # silhouette as SoftSilhouetteShader's (N,H,W,4) RGBA, written by the kernels
    z_clip: float | None = None  # near clip plane (view z) of FoVPerspectiveCameras: znear / 2
    frag_sorted: bool = False  # fragment shading: empty slots follow the filled ones (MR_FRAG_SORTED)
    zbuf: bool = False  # depth output = zbuf[..., 0] of K = 1 fragments (background -1), not relu of it

    def key(self):
        """The configuration's values (field order is the dataclass's): the struct caches' key."""
        return tuple(self.__dict__.values())

    def struct_bytes(self, kind, key=None):
        """The bytes of the configuration's mr_raster_settings_t ("r") or mr_shade_params_t ("s"), cached by its
        values (key: self.key() when the caller already has it)."""
        k = (kind, self.key() if key is None else key)
        hit = _STRUCT_CACHE.get(k)
        if hit is None:
            if len(_STRUCT_CACHE) > 256:
                _STRUCT_CACHE.clear()
            hit = _STRUCT_CACHE[k] = bytes(self._shade_struct() if kind == "s" else raster_settings_struct(
                self.H, self.W, 1, self.blur, self.persp, self.clip, self.cull, self.max_faces_per_bin, self.z_clip))
        return hit

    def raster_struct(self):
        return MrRasterSettings.from_buffer_copy(self.struct_bytes("r"))  # a copy: callers set flags on it

    def shade_struct(self):
        return MrShadeParams.from_buffer_copy(self.struct_bytes("s"))

    def _shade_struct(self):
        sp = MrShadeParams()
        sp.light_kind = int(self.light_kind)
        for name in ("light_location", "light_ambient", "light_diffuse", "light_specular", "mat_ambient",
                     "mat_diffuse", "mat_specular", "background"):
            getattr(sp, name)[:] = [float(x) for x in getattr(self, name)]
        sp.shininess = float(self.shininess)
        sp.sigma_rgb = float(self.sigma_rgb)
        sp.gamma = float(self.gamma)
        sp.znear = float(self.znear)
        sp.zfar = float(self.zfar)
        sp.sigma_sil = float(self.sigma_sil)
        sp.out_flags = ((_lib.MR_OUT_DEPTH if self.want_depth else 0) | (_lib.MR_OUT_SIL if self.want_sil else 0) |
                        (_lib.MR_OUT_RGB if self.want_rgb else 0) | (_lib.MR_OUT_HARD if self.hard else 0) |
                        (_lib.MR_OUT_SIL_RGBA if self.want_sil and self.sil_rgba else 0) |
                        (_lib.MR_OUT_ZBUF if self.want_depth and self.zbuf else 0))
        sp.rgb_channels = int(self.rgb_channels)
        return sp


@dataclass
class TextureArgs:
    kind: int = 0  # 0 white, 1 vertex colours, 2 uv
    verts_uvs: torch.Tensor | None = None
    faces_uvs: torch.Tensor | None = None
    tex_rgba: torch.Tensor | None = None  # (Ht,Wt,4) float32
    tex_u8: torch.Tensor | None = None    # optional exact 8-bit copy (TexturesUV.u8_map)
    tex_lut: torch.Tensor | None = None


def _mesh_struct(v, f, vptr, vadj, vn, tex: TextureArgs, vcol, ranges=None):
    """mr_mesh_t; ranges = (view_face_first (N+1), view_face_count (N), max faces) int64 device
    tensors + int for a batch of distinct meshes (v, f their union), None for one shared mesh."""
    m = MrMesh()
    if ranges is not None:
        m.view_face_first, m.view_face_count, m.max_view_faces = ranges[0].data_ptr(), ranges[1].data_ptr(), ranges[2]
    m.verts = v.data_ptr()
    m.V = v.shape[0]
    m.faces = f.data_ptr()
    m.F = f.shape[0]
    m.vadj_ptr = vptr.data_ptr()
    m.vadj = vadj.data_ptr()
    m.vnormals = vn.data_ptr() if vn is not None else None
    m.tex_kind = tex.kind
    m.vcolors = vcol.data_ptr() if vcol is not None else None
    m.verts_uvs = tex.verts_uvs.data_ptr() if tex.verts_uvs is not None else None
    m.faces_uvs = tex.faces_uvs.data_ptr() if tex.faces_uvs is not None else None
    m.tex_rgba = tex.tex_rgba.data_ptr() if tex.tex_rgba is not None else None
    if tex.tex_rgba is not None:
        m.tex_h, m.tex_w = int(tex.tex_rgba.shape[0]), int(tex.tex_rgba.shape[1])
    if tex.tex_u8 is not None and tex.tex_lut is not None:
        m.tex_u8, m.tex_lut = tex.tex_u8.data_ptr(), tex.tex_lut.data_ptr()
    return m


# One raster, several shadings (camera_pose_optimizer.py:244,248,250: the rasterizer's zbuf, the silhouette
# and the Phong renders of the same meshes / R / T / cameras / settings in one step): the last fused
# forward's workspace, kept while its geometry's tensors are alive and unchanged, so that a following call
# with the same geometry but a different shading only re-shades (mr_render_reshade: no projection, binning
# or rasterization). An entry serves each shading configuration once (a repeated identical call — a
# benchmark loop, a second step — rasterizes again).
# The workspace is held by a weak reference: the forward's autograd node keeps it alive while a backward
# can still run; an inference render (no_grad, nothing requiring grad, discarded outputs) lets it go, so
# the entry never pins a workspace. The key includes the launch stream (a reshade on another stream would
# read the workspace unordered).
_RESHADE = {"entry": None, "enabled": True}


def _tsig(t):
    return (t.data_ptr(), t._version, t.shape, t.stride(), t.device, t.dtype)


def _geom_sig(v, f, R, T, intr, cfg, pose_cv, ranges, stream):
    return (_tsig(v), _tsig(f), _tsig(R), _tsig(T), _tsig(intr), cfg.H, cfg.W, cfg.persp, cfg.blur, cfg.clip, cfg.cull,
            cfg.max_faces_per_bin, cfg.z_clip, bool(pose_cv), ranges is None, stream)


def render_views(verts, R, T, faces, intr, cam_centers, cfg: ShadeConfig, tex: TextureArgs | None = None,
                 vcolors=None, pose_cv=False, ranges=None):
    """Functional entry: returns dict(depth, sil, rgb[, pix_to_face32 when cfg.want_p2f]).

    One raster pass over N views of one mesh -> (depth, silhouette, rgb): replaces DepthRender.render
    (2 raster passes, torch_renderer.py:110-121) + ColorRender.render (torch_renderer.py:155-159) with a
    single fused launch sequence, and their autograd backward with one fused launch + vertex gathers.
    Differentiable inputs: verts (V,3), R (N,3,3), T (N,3), vcolors (V,3). The autograd node is C++
    (``_mr_torch``, csrc/mr_torch.cpp): the forward's and the backward's host work around the C ABI run
    without Python, the backward inside autograd's device thread.
    pose_cv: R, T are OpenCV camera poses (converted on the GPU, gradients returned in kind).
    ranges: (view_face_first, view_face_count, max faces) when verts / faces are the union of N
    distinct meshes, view n rendering mesh n (one launch for the batch); None: one shared mesh."""
    tex = tex or TextureArgs()
    _require_cuda(verts, R, T, faces)
    if not cfg.want_rgb and cfg.light_kind != 1:
        # lights only shape the Phong colours: depth / silhouette renders need no vertex normals
        cfg = ShadeConfig(**{**cfg.__dict__, "light_kind": 1})
    dev = verts.device
    f, vptr, vadj = mesh_topology(faces, verts.shape[0])
    ssig = cfg.key()  # the shading signature and the struct cache's key
    rsb = cfg.struct_bytes("r", ssig)
    spb = cfg.struct_bytes("s", ssig)
    stream = _lib.stream_handle(dev).value
    geom = _geom_sig(verts, f, R, T, intr, cfg, pose_cv, ranges, stream)
    ent = _RESHADE["entry"]
    ws = views = None
    slot = 0
    if (_RESHADE["enabled"] and ent is not None and ent["geom"] == geom and ssig not in ent["served"] and
            len(ent["served"]) < 4 and not cfg.want_p2f):
        ws = ent["ws"]()  # None once the workspace's last autograd node is gone
    if ws is not None:  # same raster, another shading: the entry's workspace and view records, a new ShadeRec slot
        views = ent["views"]
        slot = len(ent["served"])
        ent["served"].add(ssig)
    rr = ranges if ranges is not None else (None, None, 0)
    outs = _lib.torch_ext().render_views(
        verts, R, T, vcolors, f, vptr, vadj, intr, cam_centers, tex.kind, tex.verts_uvs, tex.faces_uvs,
        tex.tex_rgba, tex.tex_u8, tex.tex_lut, rr[0], rr[1], int(rr[2]), rsb, spb,
        (1 if pose_cv else 0) | (2 if cfg.want_p2f else 0), ws, views, slot)
    ws_out, views_out = outs[-2], outs[-1]
    if ws is None:
        # a new raster: the entry holds the (small) geometry tensors, so their storage cannot be reused while
        # it lives, and the workspace only weakly (the forward's autograd node keeps it while a backward can
        # run; an inference render lets it go)
        # (detached aliases: same storage and version counters, but no autograd graph kept alive — a kept
        # graph holds the leaves' AccumulateGrad nodes, whose stream then mismatches a later HIP-graph capture)
        _RESHADE["entry"] = {"geom": geom, "refs": tuple(x.detach() for x in (verts, f, R, T, intr)),
                             "ws": weakref.ref(ws_out), "views": views_out, "served": {ssig}}
    global _LAST_RENDER
    nrec = f.shape[0] if ranges is not None else views_out.shape[0] * f.shape[0]
    _LAST_RENDER = (weakref.ref(ws_out), (views_out.shape[0], nrec, cfg.H, cfg.W, int(cfg.max_faces_per_bin or 0)))
    res = {}
    i = 0
    for name, want in (("depth", cfg.want_depth), ("sil", cfg.want_sil), ("rgb", cfg.want_rgb)):
        if want:
            res[name] = outs[i]
            i += 1
    if cfg.want_p2f:
        res["pix_to_face32"] = outs[i]
    return res


def render_stats():
    """Work counters of the most recent fused forward whose workspace is still alive (kept by
    autograd until backward): dict(entries, units, tiles, covered). Synchronises; for tools."""
    if _LAST_RENDER is None or _LAST_RENDER[0]() is None:
        raise RuntimeError("no live fused-render workspace")
    ws = _LAST_RENDER[0]()
    N, Ft, H, W, mfpb = _LAST_RENDER[1]
    out = (ctypes.c_int64 * 4)()
    check(_lib.load().mr_workspace_stats(ptr(ws), N, Ft, H, W, mfpb, ctypes.cast(out, ctypes.c_void_p),
                                         _lib.stream_handle(ws.device)))
    return {"entries": out[0], "units": out[1], "tiles": out[2], "covered": out[3]}


# --------------------------------------------------------------------------- soft shading of stored fragments
def _padded_rgba(tex_map):
    """(Ht, Wt, 4) float32 copy of a (Ht, Wt, C) map as the kernels sample it (16-B texels)."""
    Ht, Wt, C = tex_map.shape
    rgba = torch.zeros((Ht, Wt, 4), dtype=torch.float32, device=tex_map.device)
    rgba[..., :min(C, 3)] = tex_map.detach()[..., :3].float()
    return rgba


def _frag_shade_struct(cfg):
    """cfg's mr_shade_params_t as mr_shade_fragments_forward / _backward take it: exactly one of the silhouette
    (not cfg.want_rgb) and RGB outputs, RGBA pixels."""
    sil = not cfg.want_rgb
    sp = cfg.shade_struct()
    sp.out_flags = _lib.MR_OUT_SIL if sil else (_lib.MR_OUT_RGB | (_lib.MR_OUT_HARD if cfg.hard else 0))
    sp.out_flags |= _lib.MR_FRAG_SORTED if cfg.frag_sorted else 0
    sp.rgb_channels = 4
    if sil:
        sp.light_kind = 1  # the silhouette blend reads no lighting (no vertex normals needed)
    return sp


class ShadeFragments(torch.autograd.Function):
    """SoftPhongShader / SoftSilhouetteShader over stored Fragments of ONE mesh shared by the N
    views (pix_to_face = n*F + f), any faces_per_pixel: mr_shade_fragments_forward / _backward
    (upstream mesh/shader.py, shading.py, blending.py).

    Differentiable inputs: zbuf, bary, dists (gradients go to the rasterizer's backward), verts
    (interpolated world positions and vertex normals), vcolors (TexturesVertex), tex_map and
    verts_uvs (TexturesUV)."""

    @staticmethod
    def forward(ctx, zbuf, bary, dists, verts, vcolors, tex_map, verts_uvs, p2f, faces, faces_uvs, cam_centers,
                cfg: ShadeConfig, ranges=None):
        """ranges (as render_views): verts / faces are the union of N distinct meshes and
        pix_to_face holds union face ids (PyTorch3D's packed ids of the batch)."""
        _require_cuda(zbuf, bary, dists, verts, p2f, faces)
        L = _lib.load()
        dev = verts.device
        N, H, W, K = p2f.shape
        v = verts.detach().float().contiguous()
        f, vptr, vadj = mesh_topology(faces, v.shape[0])
        sil = not cfg.want_rgb
        vn = raw = None
        if cfg.light_kind == 0 and not sil:
            vn, raw = _vertex_normals(v, f, vptr, vadj)
        vcol = vcolors.detach().float().contiguous() if vcolors is not None else None
        tex = TextureArgs(0)
        if vcol is not None:
            tex = TextureArgs(1)
        elif tex_map is not None:
            tex = TextureArgs(2, verts_uvs.detach().float().contiguous(), faces_uvs.to(torch.int32).contiguous(),
                              _padded_rgba(tex_map))
        mesh = _mesh_struct(v, f, vptr, vadj, vn, tex, vcol, ranges)
        sp = _frag_shade_struct(cfg)
        cc = cam_centers.float().contiguous().reshape(-1, 3)
        frag = [t.contiguous() for t in (p2f, zbuf.detach().float(), bary.detach().float(), dists.detach().float())]
        wsb = L.mr_shade_fragments_workspace(f.shape[0])
        ws = torch.empty(int(wsb), dtype=torch.uint8, device=dev)
        rgba = torch.empty((N, H, W, 4), device=dev)
        check(L.mr_shade_fragments_forward(ctypes.byref(mesh), *(ptr(t) for t in frag), N, H, W, K, ptr(cc),
                                           cc.shape[0], ctypes.byref(sp), ptr(rgba), ptr(ws), wsb,
                                           _lib.stream_handle(dev)))
        keep = [v, f, vptr, vadj, cc, ws] + frag + [t if t is not None else torch.empty(0, device=dev)
                                                    for t in (vn, raw, vcol, tex.verts_uvs, tex.faces_uvs,
                                                              tex.tex_rgba)]
        ctx.save_for_backward(*keep)
        ctx.cfg, ctx.tex_kind, ctx.ranges = cfg, tex.kind, ranges
        ctx.map_shape = None if tex_map is None else tuple(tex_map.shape)
        ctx.n_uv = 0 if verts_uvs is None else int(verts_uvs.shape[0])
        return rgba

    @staticmethod
    def backward(ctx, g):
        (v, f, vptr, vadj, cc, ws, p2f, zbuf, bary, dists, vn, raw, vcol, vuv, fuv, rgba_map) = ctx.saved_tensors
        cfg = ctx.cfg
        L = _lib.load()
        dev = v.device
        N, H, W, K = p2f.shape
        e = lambda t: t if t.numel() else None  # noqa: E731
        tex = TextureArgs(ctx.tex_kind, e(vuv), e(fuv), e(rgba_map))
        mesh = _mesh_struct(v, f, vptr, vadj, e(vn), tex, e(vcol), ctx.ranges)
        sp = _frag_shade_struct(cfg)
        bwb = L.mr_shade_fragments_backward_workspace(v.shape[0], f.shape[0])
        bws = torch.empty(int(bwb), dtype=torch.uint8, device=dev)
        # gradients that are zero by construction stay None (NULL): the silhouette blend reads only the
        # distances, hard_rgb_blend neither depths nor distances (no GB-sized zero tensors at K = 50)
        sil, hard = not cfg.want_rgb, cfg.want_rgb and cfg.hard
        gz = None if (sil or hard) else torch.empty_like(zbuf)
        gd = None if hard else torch.empty_like(dists)
        gb = None if sil else torch.empty_like(bary)
        gv = torch.empty_like(v)
        gc = torch.empty_like(vcol) if vcol.numel() else None
        need_map = ctx.tex_kind == 2 and ctx.needs_input_grad[5]
        need_uv = ctx.tex_kind == 2 and ctx.needs_input_grad[6]
        gmap = torch.empty_like(rgba_map) if need_map else None
        guv = torch.empty((ctx.n_uv, 2), device=dev) if need_uv else None
        check(L.mr_shade_fragments_backward(ctypes.byref(mesh), ptr(e(raw)), ptr(p2f), ptr(zbuf), ptr(bary), ptr(dists),
                                            N, H, W, K, ptr(cc), cc.shape[0], ctypes.byref(sp),
                                            ptr(g.float().contiguous()), ptr(ws), ptr(bws), bwb, ptr(gz), ptr(gb),
                                            ptr(gd), ptr(gv), ptr(gc), ptr(gmap), ptr(guv), ctx.n_uv,
                                            _lib.stream_handle(dev)))
        gm = gmap[..., :ctx.map_shape[-1]] if gmap is not None else None
        if gm is not None and ctx.map_shape[-1] > 3:
            gm = torch.cat([gmap[..., :3], torch.zeros(ctx.map_shape[:2] + (ctx.map_shape[-1] - 3,), device=dev)], -1)
        return gz, gb, gd, gv, gc, gm, guv, None, None, None, None, None, None


# --------------------------------------------------------------------------- point clouds: project, rasterize, composite
def point_raster_chunk() -> int:
    """Points the point rasterizer stages per pass (its results do not depend on it; tests size clouds around it)."""
    return int(_lib.load().mr_point_raster_chunk())


def _radius_args(radius, rows, what):
    """(float radius, per-point tensor or None) of a radius given as a number or a (rows,) tensor."""
    if not torch.is_tensor(radius):
        return float(radius), None
    if radius.requires_grad:
        raise NotImplementedError(f"{what}: a per-point radius that requires grad is not supported")
    _require_cuda(radius)
    if radius.dim() != 1 or radius.shape[0] != rows:
        raise ValueError(f"{what}: a per-point radius must have shape ({rows},)")
    return 0.0, radius.detach().float().contiguous()


def _points_ndc_args(points_ndc, first, count, idx_base):
    if points_ndc.dim() != 2 or points_ndc.shape[1] != 3:
        raise NotImplementedError("rasterize_points: points must be (P, 3)")
    _require_cuda(points_ndc, first, count, idx_base)
    p = points_ndc.detach().float().contiguous()
    i64 = lambda t: None if t is None else t.to(torch.int64).contiguous()  # noqa: E731
    return p, i64(first), i64(count), i64(idx_base)


def rasterize_points_fwd(points_ndc, first, count, H, W, radius, K, idx_base=None):
    p, first, count, idx_base = _points_ndc_args(points_ndc, first, count, idx_base)
    r0, rpp = _radius_args(radius, p.shape[0], "rasterize_points")
    N, dev = first.numel(), p.device
    H, W, K = int(H), int(W), int(K)
    idx = torch.empty((N, H, W, K), dtype=torch.int64, device=dev)
    zbuf = torch.empty((N, H, W, K), dtype=torch.float32, device=dev)
    dists = torch.empty((N, H, W, K), dtype=torch.float32, device=dev)
    check(_lib.load().mr_rasterize_points(ptr(p), ptr(first), ptr(count), ptr(idx_base), N, p.shape[0], H, W, r0,
                                          ptr(rpp), K, ptr(idx), ptr(zbuf), ptr(dists), _lib.stream_handle(dev)))
    return idx, zbuf, dists


def rasterize_points_bwd(points_ndc, first, idx, gz, gd, idx_base=None):
    L = _lib.load()
    p = points_ndc.detach().float().contiguous()
    N, H, W, K = idx.shape
    g = torch.empty_like(p)
    gz, gd = (None if t is None else t.float().contiguous() for t in (gz, gd))
    ws, wsb = _workspace(L.mr_rasterize_points_backward_workspace, p.device, p.shape[0])
    check(L.mr_rasterize_points_backward(ptr(p), ptr(first), ptr(idx_base), N, p.shape[0], H, W, K,
                                         ptr(idx.contiguous()), ptr(gz), ptr(gd), ptr(g), ptr(ws), wsb,
                                         _lib.stream_handle(p.device)))
    return g


class RasterizePoints(torch.autograd.Function):
    """Drop-in for PyTorch3D's _RasterizePoints (upstream points/rasterize_points.py), naive semantics."""

    @staticmethod
    def forward(ctx, points_ndc, first, count, H, W, radius, K, idx_base=None):
        ctx.set_materialize_grads(False)
        idx, zbuf, dists = rasterize_points_fwd(points_ndc, first, count, H, W, radius, K, idx_base)
        ctx.save_for_backward(points_ndc, first.to(torch.int64).contiguous(), idx,
                              torch.empty(0) if idx_base is None else idx_base.to(torch.int64).contiguous())
        ctx.mark_non_differentiable(idx)
        return idx, zbuf, dists

    @staticmethod
    def backward(ctx, _gi, gz, gd):
        p, first, idx, idx_base = ctx.saved_tensors
        g = rasterize_points_bwd(p, first, idx, gz, gd, idx_base if idx_base.numel() else None)
        return (g.to(p.dtype),) + (None,) * 7


def rasterize_points(points_ndc, first, count, H, W, radius, K, idx_base=None):
    """pytorch3d._C.rasterize_points, naive semantics (mr_rasterize_points): packed points (sum P, 3) of NDC x, NDC y
    and view z, per-cloud ``first`` / ``count`` (N), ``radius`` in NDC units (a float, or a (sum P,) tensor), K points
    per pixel. Returns idx (N,H,W,K) int64 (the packed index, or ``idx_base[n]`` + the index within cloud n), zbuf and
    dists = squared NDC distance to the pixel centre, -1 where empty; differentiable w.r.t. the points."""
    return RasterizePoints.apply(points_ndc, first, count, H, W, radius, K, idx_base)


class ProjectPoints(torch.autograd.Function):
    """PointsRasterizer.transform: view n projects rows src_first[n] .. + count[n] - 1 of the world points (P,3) to
    rows dst_first[n] .. of the (total_out, 3) result (mr_project_points); views that share a cloud name the same
    rows, and the cloud is read in place. Gradients to the points (summed over the views), R and T."""

    @staticmethod
    def forward(ctx, points, R, T, intr, src_first, dst_first, count, total_out, max_count):
        _require_cuda(points, R, T, intr, src_first, dst_first, count)
        p = points.detach().float().contiguous()
        views = make_views(R.detach(), T.detach(), intr)
        N = views.shape[0]
        out = torch.empty((int(total_out), 3), device=p.device)
        check(_lib.load().mr_project_points(ptr(p), ptr(src_first), ptr(dst_first), ptr(count), N, int(max_count),
                                            ptr(views), ptr(out), _lib.stream_handle(p.device)))
        ctx.save_for_backward(p, views, src_first, dst_first, count)
        ctx.dtype = points.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        p, views, src_first, dst_first, count = ctx.saved_tensors
        L = _lib.load()
        N = views.shape[0]
        gp = torch.empty_like(p)
        gviews = torch.empty((N, 12), device=p.device)
        ws, wsb = _workspace(L.mr_project_points_backward_workspace, p.device, p.shape[0])
        check(L.mr_project_points_backward(ptr(p), ptr(src_first), ptr(dst_first), ptr(count), N, p.shape[0], ptr(views),
                                           ptr(g.float().contiguous()), ptr(gp), ptr(gviews), ptr(ws), wsb,
                                           _lib.stream_handle(p.device)))
        return (gp.to(ctx.dtype), gviews[:, :9].reshape(N, 3, 3), gviews[:, 9:12]) + (None,) * 6


class CompositePoints(torch.autograd.Function):
    """alpha_composite / norm_weighted_sum (``flags``: MR_COMPOSITE_NORM) over fragments idx / vals (N,H,W,K) and
    features (P,C) -> (N,H,W,C) (mr_composite_points_*). With MR_COMPOSITE_DISTS ``vals`` are the rasterizer's dists
    and alpha = 1 - dists / r^2 is formed in the kernel (``radius``: a float, or a tensor indexed by idx). The
    feature row of a slot is idx - feat_sub[n]; ``background``: a (C,) device tensor or None. Gradients to vals and
    the features."""

    @staticmethod
    def forward(ctx, idx, vals, feats, flags, radius, feat_sub, background):
        _require_cuda(idx, vals, feats, feat_sub, background)
        N, H, W, K = idx.shape
        f = feats.detach().float().contiguous()
        P, C = f.shape
        ix = idx.to(torch.int64).contiguous()
        v = vals.detach().float().contiguous()
        if torch.is_tensor(radius):
            r0, rpp = _radius_args(radius, radius.shape[0] if radius.dim() == 1 else -1, "compositing")
        else:
            r0, rpp = float(radius), None
        out = torch.empty((N, H, W, C), device=f.device)
        ctx.sizes = (N, H, W, K, C, P, int(flags), r0)
        check(_lib.load().mr_composite_points_forward(ptr(ix), ptr(v), ptr(f), *ctx.sizes, ptr(rpp),
                                                      0 if rpp is None else rpp.shape[0], ptr(feat_sub),
                                                      ptr(background), ptr(out), _lib.stream_handle(f.device)))
        e = lambda t: torch.empty(0) if t is None else t  # noqa: E731
        ctx.save_for_backward(ix, v, f, e(rpp), e(feat_sub), e(background))
        ctx.dtypes = (vals.dtype, feats.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        ix, v, f, rpp, feat_sub, background = ctx.saved_tensors
        e = lambda t: t if t.numel() else None  # noqa: E731
        L = _lib.load()
        P, C = f.shape
        gv = torch.empty_like(v)
        gf = torch.empty_like(f)
        ws, wsb = _workspace(L.mr_composite_points_backward_workspace, f.device, P, C)
        check(L.mr_composite_points_backward(ptr(ix), ptr(v), ptr(f), *ctx.sizes, ptr(e(rpp)), rpp.shape[0],
                                             ptr(e(feat_sub)), ptr(e(background)), ptr(g.float().contiguous()),
                                             ptr(gv), ptr(gf), ptr(ws), wsb, _lib.stream_handle(f.device)))
        return None, gv.to(ctx.dtypes[0]), gf.to(ctx.dtypes[1]), None, None, None, None
