"""Reference for the point renderer (no GPU): upstream rasterize_points with naive semantics, the mesh path's
projection, alpha_composite and norm_weighted_sum, restated.

Rasterization. Packed points (sum P, 3) of NDC x, NDC y and view z, per-cloud first / count, radius in NDC units (a
float or one per point, r2 = r * r in float32). Pixel centres are the mesh rasterizer's (x and y flipped, the longer
side of a non-square image ranging over +-(long / short)). Point p of cloud n covers pixel (n, yi, xi) iff z >= 0 and
d2 = dx*dx + dy*dy < r2 with dx = px - xf, dy = py - yf, in float32 in this operand order, strictly. The pixel keeps
the K covering points of smallest (z, packed index), ascending; idx = idx_base[n] + index within the cloud
(idx_base None: the packed index), zbuf = z, dists = d2, -1 where empty. NaN coordinates are never drawn.

* rasterize_ref     vectorised NumPy, float32, a stable sort by (z, index)
* rasterize_loop    the plain triple loop (cross-check on tiny inputs only)
* raster_values     zbuf / dists for GIVEN idx as torch ops in the points' dtype (float64: the shadow; autograd)
* project_ref       world -> NDC with the operand order of oracle.project_faces_torch
* alphas_ref, composite_ref   1 - dists / r^2 and the two compositors as torch ops (autograd)
* render_case / render_ref    the inputs and the whole pipeline of the value-and-gradient tests
"""
import math

import numpy as np
import torch


# --------------------------------------------------------------------------- pixel centres
def pix_ndc(i, S1, S2, f=np.float32):
    """rasterization_utils.h PixToNonSquareNdc in precision f (operation by operation)."""
    rng = f(2.0)
    if S1 > S2:
        rng = (f(S1) * rng) / f(S2)
    off = rng / f(2.0)
    return -off + (rng * np.asarray(i).astype(f) + off) / f(S1)


def pixel_centres(H, W, f=np.float32):
    """(xf (W,), yf (H,)): NDC of output column xi / row yi (+x is left, +y is up)."""
    xf = pix_ndc(W - 1 - np.arange(W), W, H, f)
    yf = pix_ndc(H - 1 - np.arange(H), H, W, f)
    return xf, yf


def _np(t, dtype):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(dtype)


def _radius2(radius, total):
    r = np.full(total, radius, np.float32) if not (torch.is_tensor(radius) or isinstance(radius, np.ndarray)) \
        else _np(radius, np.float32)
    return r * r


# --------------------------------------------------------------------------- rasterization
def rasterize_ref(points, first, count, H, W, radius, K, idx_base=None):
    """Vectorised float32 reference. Returns torch idx (N,H,W,K) int64, zbuf, dists float32."""
    pts = _np(points, np.float32).reshape(-1, 3)
    first, count = _np(first, np.int64), _np(count, np.int64)
    base = first if idx_base is None else _np(idx_base, np.int64)
    r2 = _radius2(radius, pts.shape[0])
    xf, yf = pixel_centres(H, W)
    N = first.shape[0]
    idx = np.full((N, H, W, K), -1, np.int64)
    zbuf = np.full((N, H, W, K), -1.0, np.float32)
    dists = np.full((N, H, W, K), -1.0, np.float32)
    for n in range(N):
        p = pts[first[n]:first[n] + count[n]]
        if p.shape[0] == 0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            dx = p[None, None, :, 0] - xf[None, :, None]
            dy = p[None, None, :, 1] - yf[:, None, None]
            d2 = dx * dx + dy * dy                                   # (H, W, P) float32, two products then one sum
            z = p[:, 2]
            cover = (d2 < r2[first[n]:first[n] + count[n]]) & (z >= 0)[None, None, :]   # NaN: False
        zk = np.where(z == 0, np.float32(0.0), z)                    # -0.0 sorts with +0.0
        zkey = np.where(cover, zk[None, None, :], np.float32(0.0))
        order = np.lexsort((np.broadcast_to(np.arange(p.shape[0]), d2.shape), zkey, ~cover), axis=-1)[..., :K]
        kept = np.take_along_axis(cover, order, -1)
        k = order.shape[-1]
        idx[n, ..., :k] = np.where(kept, order + base[n], -1)
        zbuf[n, ..., :k] = np.where(kept, zk[order], np.float32(-1.0))
        dists[n, ..., :k] = np.where(kept, np.take_along_axis(d2, order, -1), np.float32(-1.0))
    return torch.from_numpy(idx), torch.from_numpy(zbuf), torch.from_numpy(dists)


def rasterize_loop(points, first, count, H, W, radius, K, idx_base=None):
    """The definition, loop by loop (tiny inputs only)."""
    pts = _np(points, np.float32).reshape(-1, 3)
    first, count = _np(first, np.int64), _np(count, np.int64)
    base = first if idx_base is None else _np(idx_base, np.int64)
    r2 = _radius2(radius, pts.shape[0])
    xf, yf = pixel_centres(H, W)
    N = first.shape[0]
    idx = np.full((N, H, W, K), -1, np.int64)
    zbuf = np.full((N, H, W, K), -1.0, np.float32)
    dists = np.full((N, H, W, K), -1.0, np.float32)
    for n in range(N):
        for yi in range(H):
            for xi in range(W):
                found = []
                for j in range(int(count[n])):
                    px, py, pz = pts[first[n] + j]
                    if pz < 0 or np.isnan(px) or np.isnan(py) or np.isnan(pz):
                        continue
                    dx = np.float32(px - xf[xi])
                    dy = np.float32(py - yf[yi])
                    d2 = np.float32(np.float32(dx * dx) + np.float32(dy * dy))
                    if d2 < r2[first[n] + j]:
                        found.append((float(pz) + 0.0, j, d2))
                found.sort(key=lambda t: (t[0], t[1]))
                for k, (z, j, d2) in enumerate(found[:K]):
                    idx[n, yi, xi, k] = base[n] + j
                    zbuf[n, yi, xi, k] = z
                    dists[n, yi, xi, k] = d2
    return torch.from_numpy(idx), torch.from_numpy(zbuf), torch.from_numpy(dists)


def raster_values(points, idx, first, H, W, idx_base=None):
    """(zbuf, dists) (N,H,W,K) of the decisions `idx`, as torch ops in points' dtype (autograd to the points):
    float32 points give the reference's own values, float64 points its shadow."""
    dt = points.dtype
    f = np.float64 if dt == torch.float64 else np.float32
    xf, yf = pixel_centres(H, W, f)
    xf, yf = torch.from_numpy(xf)[None, None, :, None], torch.from_numpy(yf)[None, :, None, None]
    first = torch.as_tensor(first, dtype=torch.int64)
    base = first if idx_base is None else torch.as_tensor(idx_base, dtype=torch.int64)
    src = (idx - base[:, None, None, None] + first[:, None, None, None]).clamp(min=0)
    filled = idx >= 0
    p = points[src]                                                  # (N,H,W,K,3)
    dx, dy = p[..., 0] - xf, p[..., 1] - yf
    minus1 = torch.full((), -1.0, dtype=dt)
    return torch.where(filled, p[..., 2], minus1), torch.where(filled, dx * dx + dy * dy, minus1)


# --------------------------------------------------------------------------- projection
def project_ref(points, R, T, intr):
    """(N, P, 3) NDC x, NDC y, view z of points (P,3) or (N,P,3) under N views; operand order of
    oracle.project_faces_torch."""
    X = points if points.dim() == 3 else points[None]
    Rb, Tb = R[:, None], T[:, None]
    vx = ((X[..., 0] * Rb[..., 0, 0] + X[..., 1] * Rb[..., 1, 0]) + X[..., 2] * Rb[..., 2, 0]) + Tb[..., 0]
    vy = ((X[..., 0] * Rb[..., 0, 1] + X[..., 1] * Rb[..., 1, 1]) + X[..., 2] * Rb[..., 2, 1]) + Tb[..., 1]
    vz = ((X[..., 0] * Rb[..., 0, 2] + X[..., 1] * Rb[..., 1, 2]) + X[..., 2] * Rb[..., 2, 2]) + Tb[..., 2]
    ax, bx, ay, by = (intr[:, i][:, None] for i in range(4))
    return torch.stack([ax * (vx / vz) + bx, ay * (vy / vz) + by, vz], dim=-1)


# --------------------------------------------------------------------------- compositing
NORM_EPS = 1e-4


def alphas_ref(dists, idx, radius):
    """PointsRenderer: 1 - dists / r^2, r the point's own radius (float32 r * r, then the dists' dtype)."""
    if torch.is_tensor(radius):
        r = radius.float()[idx.clamp(min=0)]
        r2 = (r * r).to(dists.dtype)
    else:
        r2 = torch.tensor(float(np.float32(radius) * np.float32(radius)), dtype=dists.dtype)
    return 1.0 - dists / r2


def composite_ref(idx, alphas, feats, mode, background=None, feat_sub=None):
    """idx / alphas (N,H,W,K), feats (P,C) -> (N,H,W,C); mode "alpha" or "norm". Slots with idx < 0 are skipped; a
    pixel whose first slot is empty gets `background` (3 entries with C = 4: alpha 1 appended)."""
    filled = idx >= 0
    row = idx if feat_sub is None else idx - torch.as_tensor(feat_sub, dtype=torch.int64)[:, None, None, None]
    f = feats[row.clamp(min=0)]                                      # (N,H,W,K,C)
    a = torch.where(filled, alphas, torch.zeros((), dtype=alphas.dtype))
    if mode == "alpha":
        T = torch.cumprod(torch.cat([torch.ones_like(a[..., :1]), 1.0 - a[..., :-1]], -1), -1)
        out = (f * (a * T)[..., None]).sum(-2)
    elif mode == "norm":
        out = (f * a[..., None]).sum(-2) / a.sum(-1, keepdim=True).clamp(min=NORM_EPS)
    else:
        raise ValueError(mode)
    if background is not None:
        C = feats.shape[1]
        bg = torch.as_tensor(background, dtype=out.dtype).reshape(-1)
        if C == 4 and bg.numel() == 3:
            bg = torch.cat([bg, bg.new_ones(1)])
        if bg.numel() != C:
            raise ValueError(f"background color has {bg.numel()} channels not {C}")
        out = torch.where(idx[..., :1] < 0, bg, out)
    return out


# --------------------------------------------------------------------------- the value-and-gradient cases
def ball_cloud(P, seed, radius=0.5):
    """P points in a ball (float32): well spread in depth, no two alike."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(P, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    return (d * radius * torch.rand(P, 1, generator=g) ** (1.0 / 3.0)).float()


# (mode, shared, C): both compositors, both batch kinds, every channel count
RENDER_CASES = [("alpha", True, 3), ("norm", True, 1), ("alpha", False, 4), ("norm", False, 3), ("alpha", False, 1),
                ("norm", True, 4)]
RENDER_H, RENDER_W, RENDER_K, RENDER_N, RENDER_RADIUS = 24, 32, 6, 3, 0.2
RENDER_BG = (0.25, 0.5, 0.75)


def render_case(mode, shared, C):
    """Inputs of one value-and-gradient case (CPU float32): clouds, features, canonical views, output weights."""
    from tests.helpers import canonical_views

    seed = 100 + 10 * ["alpha", "norm"].index(mode) + C + (5 if shared else 0)
    sizes = [230] if shared else [150, 1, 97][:RENDER_N]
    clouds = [ball_cloud(p, seed + i) for i, p in enumerate(sizes)]
    g = torch.Generator().manual_seed(seed + 50)
    feats = [torch.rand(p, C, generator=g) for p in sizes]
    R, T, intr, _ = canonical_views(torch.cat(clouds, 0), RENDER_N, RENDER_H, RENDER_W, dist=1.6)
    wt = torch.rand(RENDER_N, RENDER_H, RENDER_W, C, generator=g)
    bg = RENDER_BG[:C] if C <= 3 else RENDER_BG   # C = 4: three entries, alpha 1 appended
    return dict(mode=mode, shared=shared, C=C, clouds=clouds, feats=feats, R=R, T=T, intr=intr, wt=wt, bg=bg)


def _case_layout(case):
    sizes = [c.shape[0] for c in case["clouds"]]
    if case["shared"]:
        cnt = sizes * RENDER_N
        first = [i * sizes[0] for i in range(RENDER_N)]
        sub = first
    else:
        cnt = sizes
        first = [sum(sizes[:i]) for i in range(len(sizes))]
        sub = None
    return first, cnt, sub


def case_ndc(case, dtype=torch.float32, leaves=None):
    """Packed NDC points (sum over views, 3) of a case (and the layout), in `dtype`."""
    first, cnt, sub = _case_layout(case)
    pts = leaves["points"] if leaves else [c.to(dtype) for c in case["clouds"]]
    R = leaves["R"] if leaves else case["R"].to(dtype)
    T = leaves["T"] if leaves else case["T"].to(dtype)
    intr = case["intr"].to(dtype)
    if case["shared"]:
        ndc = project_ref(pts[0], R, T, intr).reshape(-1, 3)
    else:
        ndc = torch.cat([project_ref(p, R[i:i + 1], T[i:i + 1], intr[i:i + 1])[0] for i, p in enumerate(pts)], 0)
    return ndc, first, cnt, sub


def case_radius(case, per_point):
    """(the settings' radius, the radius of every packed (view, point) row): RENDER_RADIUS, or with per_point one of
    three radii per point of the clouds (a shared cloud's repeated for every view)."""
    if not per_point:
        return RENDER_RADIUS, RENDER_RADIUS
    n = sum(c.shape[0] for c in case["clouds"])
    g = torch.Generator().manual_seed(n)
    r = torch.tensor([0.5, 1.0, 1.5])[torch.randint(0, 3, (n,), generator=g)] * RENDER_RADIUS
    return r, (r.repeat(RENDER_N) if case["shared"] else r)


def case_idx(case, per_point_radius=False):
    """The float32 reference's decisions for a case."""
    ndc, first, cnt, _ = case_ndc(case)
    return rasterize_ref(ndc, first, cnt, RENDER_H, RENDER_W, case_radius(case, per_point_radius)[1], RENDER_K)[0]


def render_ref(case, idx, dtype, per_point_radius=False):
    """The pipeline with the decisions `idx` fixed, in `dtype`: (image, grad points (packed), grad features
    (packed), grad R, grad T) for the loss sum(image * wt)."""
    leaf = lambda t: t.detach().clone().to(dtype).requires_grad_(True)  # noqa: E731
    leaves = dict(points=[leaf(c) for c in case["clouds"]], R=leaf(case["R"]), T=leaf(case["T"]))
    feats = [leaf(f) for f in case["feats"]]
    ndc, first, _, sub = case_ndc(case, dtype, leaves)
    _, dists = raster_values(ndc, idx, first, RENDER_H, RENDER_W)
    radius = case_radius(case, per_point_radius)[1]
    img = composite_ref(idx, alphas_ref(dists, idx, radius), torch.cat(feats, 0), case["mode"], case["bg"], sub)
    (img * case["wt"].to(dtype)).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731
    return (img.detach(), torch.cat([zero(p) for p in leaves["points"]], 0), torch.cat([zero(f) for f in feats], 0),
            zero(leaves["R"]), zero(leaves["T"]))


def boundary_clouds(chunk, seed=0):
    """The raster-boundary batch: clouds of [0, 1, chunk - 1, chunk, chunk + 1, 2 chunk + 1] points in NDC, some
    outside the image, with z < 0, z = 0 and z = -0.0 present. Returns (points (sum P, 3), first, count)."""
    g = torch.Generator().manual_seed(seed)
    counts = [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    pts = []
    for c in counts:
        xy = (torch.rand(c, 2, generator=g) * 2 - 1) * 1.9          # beyond the widest range used (40 / 24 = 1.67)
        z = torch.rand(c, 1, generator=g) * 3 + 0.5
        p = torch.cat([xy, z], 1)
        if c >= 8:
            p[1, 2] = -0.5
            p[2, 2] = 0.0
            p[3, 2] = -0.0
            p[5, 2] = 0.0
        pts.append(p)
    first = [sum(counts[:i]) for i in range(len(counts))]
    return torch.cat(pts, 0).float(), torch.tensor(first), torch.tensor(counts)


BWD_H, BWD_W, BWD_K = 24, 40, 3


def boundary_backward_case(chunk):
    """The raster boundary's backward: the boundary batch at 24x40, K = 3, a few pixels' radius, random upstream
    gradients for zbuf and dists."""
    pts, first, count = boundary_clouds(chunk)
    g = torch.Generator().manual_seed(2)
    shape = (first.numel(), BWD_H, BWD_W, BWD_K)
    return dict(pts=pts, first=first, count=count, radius=boundary_radii(BWD_H, BWD_W, pts.shape[0])["mid"],
                gz=torch.rand(shape, generator=g) - 0.5, gd=torch.rand(shape, generator=g) - 0.5)


def boundary_backward_ref(case, idx, dtype):
    """grad of sum(zbuf gz) + sum(dists gd) w.r.t. the points, decisions fixed, in `dtype`."""
    p = case["pts"].detach().clone().to(dtype).requires_grad_(True)
    z, d = raster_values(p, idx, case["first"], BWD_H, BWD_W)
    ((z * case["gz"].to(dtype)).sum() + (d * case["gd"].to(dtype)).sum()).backward()
    return p.grad


def composite_layout_case(C):
    """Random fragments in upstream's layout: idx / alphas (N,K,H,W) with empty slots anywhere, features (C,P)."""
    g = torch.Generator().manual_seed(5 + C)
    N, K, H, W, P = 2, 4, 5, 7, 11
    return (torch.randint(-1, P, (N, K, H, W), generator=g), torch.rand(N, K, H, W, generator=g),
            torch.rand(C, P, generator=g))


def composite_layout_ref(case, mode, dtype):
    """(out (N,C,H,W), grad alphas, grad features) of sum(out^2) in upstream's layout, in `dtype`."""
    idx, al, f = case
    a, ff = al.clone().to(dtype).requires_grad_(True), f.clone().to(dtype).requires_grad_(True)
    o = composite_ref(idx.permute(0, 2, 3, 1), a.permute(0, 2, 3, 1), ff.t(), mode).permute(0, 3, 1, 2)
    o.square().sum().backward()
    return o.detach(), a.grad, ff.grad


def pitch(H, W):
    """NDC distance between neighbouring pixel centres."""
    return 2.0 / min(H, W)


def boundary_radii(H, W, total, seed=1):
    """{name: radius}: below half a pixel pitch, a few pixels, larger than the image, and a per-point mix."""
    g = torch.Generator().manual_seed(seed)
    small, mid, big = 0.3 * pitch(H, W), 2.5 * pitch(H, W), 2.0 * math.hypot(2.0 * max(H, W) / min(H, W), 2.0)
    mix = torch.tensor([small, mid, big])[torch.randint(0, 3, (total,), generator=g)].float()
    return {"small": small, "mid": mid, "big": big, "mix": mix}
