"""PyTorch3D's point-cloud rendering API on the MI355X kernels.

The reference's point renderers (torch_renderer.py:162-207) are built on ``PointsRasterizationSettings``,
``PointsRasterizer`` -> fragments, ``AlphaCompositor`` / ``NormWeightedCompositor`` and ``PointsRenderer``. This
module mirrors their constructors, argument meaning and outputs:

* ``PointsRasterizer(point_clouds)`` projects the clouds as the mesh path projects vertices (``mr_project_points``,
  view z kept as the depth) and rasterizes them with upstream's naive semantics (``mr_rasterize_points``): a point
  covers a pixel iff the squared NDC distance to the pixel centre is below radius^2, and a pixel keeps the
  ``points_per_pixel`` nearest of them in (z, index) order. Returns ``PointFragments(idx, zbuf, dists)``,
  differentiable w.r.t. the points and R, T.
* ``PointsRenderer`` composites features over the fragments with alpha = 1 - dists / radius^2
  (``mr_composite_points_*``), differentiable w.r.t. the features and, through the distances, the points and poses.

One deviation from upstream: ``Pointclouds`` here holds no features, so ``PointsRenderer.forward`` takes them itself
(``features=``). Everything runs on the HIP kernels; CPU tensors raise.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple

import torch

from . import _lib
from .cameras import view_batch
from .kernels import CompositePoints, ProjectPoints, RasterizePoints, _require_cuda
from .structures import Pointclouds


@dataclass
class PointsRasterizationSettings:
    """upstream points/rasterizer.py PointsRasterizationSettings (image_size int -> square). ``radius`` is in NDC
    units: a float, or a tensor with one radius per packed point. ``bin_size`` and ``max_points_per_bin`` are
    accepted and have no effect: the rasterizer here keeps no bins. Every (view, tile) streams its view's whole
    cloud, so there is no capacity to size, nothing can overflow, and the result is the naive rasterizer's at every
    setting."""
    image_size: int | tuple = 256
    radius: float | torch.Tensor = 0.01
    points_per_pixel: int = 8
    bin_size: int | None = None
    max_points_per_bin: int | None = None

    def hw(self):
        s = self.image_size
        if isinstance(s, int):
            return s, s
        return int(s[0]), int(s[1])


class PointFragments(NamedTuple):
    """upstream points/rasterizer.py PointFragments: idx (N,H,W,K) int64 packed point indices (for one cloud shared
    by the views n * P + p), zbuf (view z) and dists (squared NDC distance to the pixel centre); -1 where empty."""
    idx: torch.Tensor
    zbuf: torch.Tensor
    dists: torch.Tensor


_INDEX_CACHE: dict = {}


def _layout(counts, n_views, shared, device):
    """Device index arrays of one batch: (src_first, dst_first, count, total_out, max_count). Cached by value, so a
    repeated call uploads nothing (and a captured graph sees no host copy)."""
    key = (tuple(counts), n_views, shared, str(device))
    v = _INDEX_CACHE.get(key)
    if v is None:
        if len(_INDEX_CACHE) > 64:
            _INDEX_CACHE.clear()
        cnt = [counts[0]] * n_views if shared else list(counts)
        dst = [0]
        for c in cnt[:-1]:
            dst.append(dst[-1] + c)
        src = [0] * n_views if shared else dst
        dev = lambda a: torch.tensor(a, dtype=torch.int64, device=device)  # noqa: E731
        v = _INDEX_CACHE[key] = (dev(src), dev(dst), dev(cnt), sum(cnt), max(cnt) if cnt else 0)
    return v


def _batch(point_clouds, cameras, hw, kwargs):
    """(world points (P,3), shared, R, T, intr, layout) of a call: one cloud (a batch of one, or extend(N)) is shared
    by the N views and read in place; N clouds under N (or one broadcast) cameras render pairwise."""
    if not isinstance(point_clouds, Pointclouds):
        raise ValueError("point_clouds must be a Pointclouds")
    if cameras is None:
        raise ValueError("Cameras must be specified either at initialization or in the forward pass")
    for k in ("lights", "materials"):
        if kwargs.get(k) is not None:
            raise NotImplementedError(f"point rendering takes no {k}")
    if len(point_clouds) == 0:
        raise ValueError("point_clouds is empty")
    R, T = kwargs.get("R", None), kwargs.get("T", None)
    n_cam = max(cameras.R.reshape(-1, 3, 3).shape[0] if R is None else R.reshape(-1, 3, 3).shape[0],
                cameras.T.reshape(-1, 3).shape[0] if T is None else T.reshape(-1, 3).shape[0])
    n_pc = len(point_clouds)
    shared = point_clouds.is_shared() or n_pc == 1
    if shared and point_clouds.is_shared() and n_cam not in (1, n_pc):
        raise ValueError(f"Pointclouds batch ({n_pc}) and camera batch ({n_cam}) differ")
    if not shared and n_cam not in (1, n_pc):
        raise ValueError(f"Pointclouds batch ({n_pc}) and camera batch ({n_cam}) differ")
    n_views = max(n_pc, n_cam)
    R, T, intr = view_batch(cameras, hw, R, T, n_views=n_views)
    pts = point_clouds.points_list()[0] if shared else point_clouds.points_packed()
    if pts.dim() != 2 or pts.shape[-1] != 3:
        raise NotImplementedError("point clouds must have 3 coordinates per point")
    _require_cuda(pts, R, T)
    return pts, shared, R, T, intr, _layout(point_clouds.counts(), n_views, shared, pts.device)


class PointsRasterizer(torch.nn.Module):
    """upstream points/rasterizer.py PointsRasterizer."""

    def __init__(self, cameras=None, raster_settings=None):
        super().__init__()
        self.cameras = cameras
        self.raster_settings = raster_settings or PointsRasterizationSettings()

    def _project(self, point_clouds, kwargs):
        cameras = kwargs.get("cameras", self.cameras)
        rs = kwargs.get("raster_settings", self.raster_settings)
        if torch.is_tensor(rs.radius) and rs.radius.requires_grad:
            raise NotImplementedError("a per-point radius that requires grad is not supported")
        pts, shared, R, T, intr, lay = _batch(point_clouds, cameras, rs.hw(), kwargs)
        src, dst, cnt, total, pmax = lay
        ndc = ProjectPoints.apply(pts, R, T, intr.contiguous(), src, dst, cnt, total, pmax)
        return ndc, pts, shared, lay

    def transform(self, point_clouds, **kwargs):
        """Packed (sum P, 3) NDC x, NDC y and view z of every (view, point), view by view: the mesh path's
        projection (a point projects bitwise as a mesh vertex at the same position)."""
        return self._project(point_clouds, kwargs)[0]

    def forward(self, point_clouds, **kwargs) -> PointFragments:
        rs = kwargs.get("raster_settings", self.raster_settings)
        H, W = rs.hw()
        ndc, pts, shared, (src, dst, cnt, total, pmax) = self._project(point_clouds, kwargs)
        radius = _packed_radius(rs.radius, pts.shape[0], total, shared)
        idx, zbuf, dists = RasterizePoints.apply(ndc, dst, cnt, H, W, radius, int(rs.points_per_pixel))
        return PointFragments(idx=idx, zbuf=zbuf, dists=dists)


def _packed_radius(radius, n_points, total, shared):
    """The settings' radius for the packed (view, point) rows: a float, or per point (a shared cloud's repeated
    for every view)."""
    if not torch.is_tensor(radius):
        return float(radius)
    if radius.requires_grad:
        raise NotImplementedError("a per-point radius that requires grad is not supported")
    if radius.dim() != 1 or radius.shape[0] != n_points:
        raise ValueError(f"a per-point radius must have shape ({n_points},)")
    r = radius.detach().float()
    return r.repeat(total // n_points) if shared and n_points and total != n_points else r


# --------------------------------------------------------------------------- compositors
_BG_CACHE: dict = {}


def _background(background_color, C, device):
    """(C,) device tensor of a compositor's background (None: none). A 3-entry colour with C = 4 gets alpha 1."""
    if background_color is None:
        return None
    if torch.is_tensor(background_color):
        bg = background_color.detach().float().reshape(-1).to(device)
    else:
        vals = tuple(float(v) for v in background_color)
        key = (vals, C, str(device))
        bg = _BG_CACHE.get(key)
        if bg is None:
            if len(_BG_CACHE) > 64:
                _BG_CACHE.clear()
            bg = _BG_CACHE[key] = torch.tensor(vals, dtype=torch.float32, device=device)
    if C == 4 and bg.shape[0] == 3:
        bg = torch.cat([bg, bg.new_ones(1)])
    if bg.shape[0] != C:
        raise ValueError(f"background color has {bg.shape[0]} channels not {C}")
    return bg.contiguous()


def _composite_upstream(pointsidx, alphas, pt_clds, flags, background_color=None):
    """Upstream's layout: pointsidx / alphas (N,K,H,W), pt_clds (C,P) -> (N,C,H,W)."""
    if pointsidx.dim() != 4 or tuple(alphas.shape) != tuple(pointsidx.shape) or pt_clds.dim() != 2:
        raise ValueError("pointsidx and alphas must be (N, K, H, W) and the features (C, P)")
    _require_cuda(pointsidx, alphas, pt_clds)
    bg = _background(background_color, pt_clds.shape[0], pt_clds.device)
    out = CompositePoints.apply(pointsidx.permute(0, 2, 3, 1), alphas.permute(0, 2, 3, 1), pt_clds.t(), flags, 0.0,
                                None, bg)
    return out.permute(0, 3, 1, 2)


def alpha_composite(pointsidx, alphas, pt_clds):
    """upstream compositing.alpha_composite: out[n,c,y,x] = sum_k f[c, idx_k] alpha_k prod_{j<k} (1 - alpha_j)."""
    return _composite_upstream(pointsidx, alphas, pt_clds, 0)


def norm_weighted_sum(pointsidx, alphas, pt_clds):
    """upstream compositing.norm_weighted_sum: out[n,c,y,x] = sum_k f[c, idx_k] alpha_k / max(sum_k alpha_k, 1e-4)."""
    return _composite_upstream(pointsidx, alphas, pt_clds, _lib.MR_COMPOSITE_NORM)


class _Compositor(torch.nn.Module):
    flags = 0

    def __init__(self, background_color=None):
        super().__init__()
        self.background_color = background_color

    def forward(self, fragments, alphas, ptclds, **kwargs):
        """upstream layout: fragments (idx) and alphas (N,K,H,W), ptclds (C,P) -> (N,C,H,W)."""
        return _composite_upstream(fragments, alphas, ptclds, self.flags,
                                   kwargs.get("background_color", self.background_color))


class AlphaCompositor(_Compositor):
    """upstream points/compositor.py AlphaCompositor."""


class NormWeightedCompositor(_Compositor):
    """upstream points/compositor.py NormWeightedCompositor."""
    flags = _lib.MR_COMPOSITE_NORM


# --------------------------------------------------------------------------- renderer
def _packed_features(features, point_clouds, shared):
    """(P, C) feature rows in the clouds' packed order from a list of (P_i, C) tensors or a padded (N, P, C) one."""
    if features is None:
        raise ValueError("PointsRenderer: pass the points' features as features= (a list of (P_i, C) tensors or a "
                         "padded (N, P, C) tensor): Pointclouds here holds no features")
    counts = point_clouds.counts()
    n = 1 if shared else len(counts)
    if torch.is_tensor(features):
        if features.dim() == 2 and n == 1:
            features = features[None]
        if features.dim() != 3 or features.shape[0] not in (n, len(counts)):
            raise ValueError("features must be a list of (P_i, C) tensors or a padded (N, P, C) tensor")
        flist = [features[i, :counts[i]] for i in range(n)]
    else:
        flist = list(features)[:n] if shared and len(features) == len(counts) else list(features)
        if len(flist) != n:
            raise ValueError(f"features has {len(flist)} entries for {n} clouds")
    for f, c in zip(flist, counts):
        if f.dim() != 2 or f.shape[0] != c:
            raise ValueError("every cloud's features must be (P_i, C)")
    return flist[0] if n == 1 else torch.cat(flist, 0)


class PointsRenderer(torch.nn.Module):
    """upstream points/renderer.py PointsRenderer: rasterize, alpha = 1 - dists / radius^2, composite -> (N,H,W,C).
    ``forward(point_clouds, features=..., **kwargs)``: the features come with the call (see the module docstring)."""

    def __init__(self, rasterizer, compositor):
        super().__init__()
        self.rasterizer = rasterizer
        self.compositor = compositor

    def forward(self, point_clouds, features=None, **kwargs) -> torch.Tensor:
        rs = kwargs.get("raster_settings", self.rasterizer.raster_settings)
        shared = isinstance(point_clouds, Pointclouds) and (point_clouds.is_shared() or len(point_clouds) == 1)
        feats = _packed_features(features, point_clouds, shared) if isinstance(point_clouds, Pointclouds) else None
        fragments = self.rasterizer(point_clouds, **kwargs)
        _require_cuda(feats)
        N = fragments.idx.shape[0]
        n_points = feats.shape[0]
        radius = _packed_radius(rs.radius, n_points, N * n_points if shared else n_points, shared)
        comp = self.compositor
        if not isinstance(comp, _Compositor):  # a compositor of the caller's, in upstream's layout
            r = radius if not torch.is_tensor(radius) else radius[fragments.idx.clamp(min=0)]
            alphas = 1.0 - fragments.dists / (r * r)
            f = feats.repeat(N, 1) if shared and N > 1 else feats
            return comp(fragments.idx.permute(0, 3, 1, 2), alphas.permute(0, 3, 1, 2), f.t(), **kwargs).permute(0, 2, 3, 1)
        bg = _background(kwargs.get("background_color", comp.background_color), feats.shape[1], feats.device)
        sub = _layout(point_clouds.counts(), N, True, feats.device)[1] if shared else None
        return CompositePoints.apply(fragments.idx, fragments.dists, feats, comp.flags | _lib.MR_COMPOSITE_DISTS,
                                     radius, sub, bg)
