"""Plain-torch restatement of the point-to-triangle distance of include/mi355r.h (PyTorch3D point_mesh_face_distance):
the yardstick of test_point_mesh_cpu.py / test_gpu_point_mesh.py, and ``loss_composed`` is the baseline
tools/point_mesh_bench.py times on the device.

``pair_dist`` keeps the kernel's operation order with one torch op per operation (no FMA; dot products as
(x*x' + y*y') + z*z'), so that in float32 ``nearest_ref`` (first minimum in both directions) is bitwise what the
kernels define; in float64 it is the reference. ``tri_dist_voronoi`` is a second, independent float64 formulation of
the true triangle distance (closest point by Voronoi region) that serves only to check the first.
"""
import numpy as np
import torch

EPS = 1e-8


class _Sqrt(torch.autograd.Function):
    """A correctly rounded square root on the CPU. torch's vectorised CPU sqrt is not: in float32 it differs from the
    IEEE result in 0.6 % to 20 % of random entries depending on the machine, which moves a plane distance by a few
    ulp; numpy's is the hardware instruction, as the kernel's sqrtf is correctly rounded."""

    @staticmethod
    def forward(ctx, x):
        y = torch.from_numpy(np.sqrt(x.detach().numpy()))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return g * 0.5 / y


def _sqrt(x):
    return x.sqrt() if x.is_cuda else _Sqrt.apply(x.contiguous())


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _seg(p, a, b, ab, l2, eps):
    """Squared distance of p to the segment a -> b and the parameter t of the closest point a + t ab."""
    short = l2 <= eps
    t = (_dot(p - a, ab) / torch.where(short, torch.ones_like(l2), l2)).clamp(0.0, 1.0)
    d = p - (a + t[..., None] * ab)
    db = p - b
    return torch.where(short, _dot(db, db), _dot(d, d)), torch.where(short, torch.ones_like(t), t)


def pair_terms(p, tris, min_triangle_area=5e-3):
    """p (..., 3) against tris (..., 3, 3), broadcast: (d, bary (..., 3) of the closest point, inside: the plane
    branch was taken), in the inputs' dtype and the kernel's operation order."""
    dt = p.dtype
    eps, amin = torch.tensor(EPS, dtype=dt), torch.tensor(min_triangle_area, dtype=dt)
    v0, v1, v2 = tris[..., 0, :], tris[..., 1, :], tris[..., 2, :]
    e01, e12, e20 = v1 - v0, v2 - v1, v0 - v2
    w = -e20
    l01, l12, l20 = _dot(e01, e01), _dot(e12, e12), _dot(e20, e20)
    d01 = _dot(e01, w)
    n = torch.stack((e01[..., 1] * w[..., 2] - e01[..., 2] * w[..., 1], e01[..., 2] * w[..., 0] - e01[..., 0] * w[..., 2],
                     e01[..., 0] * w[..., 1] - e01[..., 1] * w[..., 0]), -1)
    nn = _dot(n, n)
    one = torch.ones_like(nn)
    ln = torch.where(nn > 0, _sqrt(torch.where(nn > 0, nn, one)), torch.zeros_like(nn))  # sqrt(nn), no NaN gradient at 0
    plane = (0.5 * ln >= amin) & (ln > eps)
    nhat = torch.where(plane[..., None], n / torch.where(plane, ln, one)[..., None], torch.zeros_like(n))
    nns = torch.where(plane, nn, one)
    q = p - v0
    d20, d21 = _dot(q, e01), _dot(q, w)
    b1 = (l20 * d20 - d01 * d21) / nns
    b2 = (l01 * d21 - d01 * d20) / nns
    b0 = (1.0 - b1) - b2
    inside = plane & (b0 >= 0) & (b0 <= 1) & (b1 >= 0) & (b1 <= 1) & (b2 >= 0) & (b2 <= 1)
    h = _dot(v0 - p, nhat)
    s0, t0 = _seg(p, v0, v1, e01, l01, eps)
    s1, t1 = _seg(p, v1, v2, e12, l12, eps)
    s2, t2 = _seg(p, v2, v0, e20, l20, eps)
    use1 = s1 < s0  # the winning edge: the first minimum in the order (01, 12, 20)
    use2 = s2 < torch.minimum(s0, s1)
    # min(s0, s1, s2) by selection: autograd then follows the winning edge alone, as the kernel's backward does (torch's
    # minimum would split the gradient between equal operands)
    d = torch.where(inside, h * h, torch.where(use2, s2, torch.where(use1, s1, s0)))
    z = torch.zeros_like(t0)
    be = torch.where(use2[..., None], torch.stack((t2, z, 1 - t2), -1),
                     torch.where(use1[..., None], torch.stack((z, 1 - t1, t1), -1), torch.stack((1 - t0, t0, z), -1)))
    bary = torch.where(inside[..., None], torch.stack((b0, b1, b2), -1), be)
    return d, bary, inside


def pair_dist(points, tris, min_triangle_area=5e-3, dtype=torch.float32):
    """(P, T) matrix of d(point, triangle) for points (P,3) and tris (T,3,3), computed in ``dtype``."""
    p, t = points.detach().to(dtype), tris.detach().to(dtype)
    return pair_terms(p[:, None, :], t[None], min_triangle_area)[0]


def tri_dist_voronoi(points, tris):
    """(P, T) true squared point-to-triangle distances in float64 by the Voronoi-region closest-point method (the
    three vertex regions, the three edge regions, the interior): independent of pair_terms."""
    p = points.detach().double()[:, None, :]
    a, b, c = (tris.detach().double()[None, :, k, :] for k in range(3))
    dot = lambda u, v: (u * v).sum(-1)  # noqa: E731
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = p - b
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = p - c
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    safe = lambda x: torch.where(x == 0, torch.ones_like(x), x)  # noqa: E731
    den = safe(va + vb + vc)
    close = a + ab * (vb / den)[..., None] + ac * (vc / den)[..., None]  # interior
    w = (d4 - d3) / safe((d4 - d3) + (d5 - d6))
    close = torch.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[..., None], b + w[..., None] * (c - b), close)
    w = d2 / safe(d2 - d6)
    close = torch.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], a + w[..., None] * ac, close)
    close = torch.where(((d6 >= 0) & (d5 <= d6))[..., None], c.expand_as(close), close)
    v = d1 / safe(d1 - d3)
    close = torch.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + v[..., None] * ab, close)
    close = torch.where(((d3 >= 0) & (d4 <= d3))[..., None], b.expand_as(close), close)
    close = torch.where(((d1 <= 0) & (d2 <= 0))[..., None], a.expand_as(close), close)
    return ((p - close) ** 2).sum(-1)


def nearest_ref(points_list, verts_list, faces_list, min_triangle_area=5e-3, dtype=torch.float32):
    """Packed (dist_p (P,) dtype, idx_p (P,) int32, dist_f (T,), idx_f (T,)) of a batch given as lists, on the CPU:
    the first minimum in both directions, indices within the mesh / cloud, 0 / -1 without a counterpart."""
    out = [[], [], [], []]
    for pts, v, f in zip(points_list, verts_list, faces_list):
        P, T = pts.shape[0], f.shape[0]
        dp, ip = torch.zeros(P, dtype=dtype), torch.full((P,), -1, dtype=torch.int32)
        df, it = torch.zeros(T, dtype=dtype), torch.full((T,), -1, dtype=torch.int32)
        if P and T:
            d = pair_dist(pts.cpu(), v.detach().cpu()[f.cpu().long()], min_triangle_area, dtype)
            i = d.argmin(dim=1)  # the first minimum
            dp, ip = d.gather(1, i[:, None])[:, 0], i.to(torch.int32)
            j = d.argmin(dim=0)
            df, it = d.gather(0, j[None, :])[0], j.to(torch.int32)
        for o, t in zip(out, (dp, ip, df, it)):
            o.append(t)
    return tuple(torch.cat(o) for o in out)


def split(t, counts):
    return list(t.split([int(c) for c in counts]))


def loss_ref(points_list, verts_list, faces_list, idx_p, idx_f, min_triangle_area=5e-3):
    """The loss in the inputs' dtype for GIVEN nearest primitives (packed idx_p / idx_f as nearest_ref returns them;
    -1: no term); differentiable w.r.t. the points and the vertices by autograd."""
    N = len(points_list)
    ips = split(idx_p, [p.shape[0] for p in points_list])
    its = split(idx_f, [f.shape[0] for f in faces_list])
    total = 0.0
    for pts, v, f, ip, it in zip(points_list, verts_list, faces_list, ips, its):
        P, T = pts.shape[0], f.shape[0]
        if not (P and T):
            continue
        tris = v[f.long()]
        dp = pair_terms(pts, tris[ip.long()], min_triangle_area)[0]
        df = pair_terms(pts[it.long()], tris, min_triangle_area)[0]
        total = total + dp.sum() / P + df.sum() / T
    return total / N


def loss_composed(points, verts, faces, min_triangle_area=5e-3):
    """point_mesh_face_distance of ONE cloud and ONE mesh composed from torch ops on the tensors' device: broadcast
    (P, T) pair distances -> min -> gather -> autograd through the winners. Materialises several (P, T, 3) tensors."""
    tris = verts[faces.long()]
    with torch.no_grad():
        d = pair_terms(points[:, None, :], tris[None], min_triangle_area)[0]
        ip, it = d.argmin(dim=1), d.argmin(dim=0)
    dp = pair_terms(points, tris[ip], min_triangle_area)[0]
    df = pair_terms(points[it], tris, min_triangle_area)[0]
    return dp.mean() + df.mean()
