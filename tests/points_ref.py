"""Plain-torch restatements of the point-cloud functions (PyTorch3D's chamfer_distance with its K = 1 nearest
neighbours, sample_points_from_meshes' point construction, face areas): the yardstick of test_points_cpu.py /
test_gpu_points.py, and ``chamfer_composed`` is the baseline tools/chamfer_bench.py times on the device.

The distance keeps the kernels' operation order, norm 2: (dx*dx + dy*dy) + dz*dz, norm 1: (|dx| + |dy|) + |dz|, one
torch op per operation (no FMA), and ``argmin`` returns the first minimum, so that in float32 ``nearest_ref`` is
bitwise what the kernels define. Entries past a length, or of a cloud whose counterpart has length 0: 0 / -1.
"""
import torch


def pair_dist(q, t, norm=2):
    """(Pq, Pt) distances of q (Pq,3) to t (Pt,3) in their dtype, in the fixed operation order."""
    dx = q[:, None, 0] - t[None, :, 0]
    dy = q[:, None, 1] - t[None, :, 1]
    dz = q[:, None, 2] - t[None, :, 2]
    if norm == 2:
        return (dx * dx + dy * dy) + dz * dz
    return (dx.abs() + dy.abs()) + dz.abs()


def _lengths(l, N, P):
    return [P] * N if l is None else [int(v) for v in l.tolist()]


def nearest_ref(x, y, x_lengths=None, y_lengths=None, norm=2, dtype=torch.float32):
    """(dist_x (N,P1) dtype, idx_x (N,P1) int32, dist_y (N,P2), idx_y (N,P2)) on the CPU."""
    x, y = x.detach().cpu().to(dtype), y.detach().cpu().to(dtype)
    N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
    lx, ly = _lengths(x_lengths, N, P1), _lengths(y_lengths, N, P2)
    out = []
    for q, t, lq, lt in ((x, y, lx, ly), (y, x, ly, lx)):
        dist = torch.zeros(q.shape[:2], dtype=dtype)
        idx = torch.full(q.shape[:2], -1, dtype=torch.int32)
        for n in range(N):
            if lq[n] == 0 or lt[n] == 0:
                continue
            d = pair_dist(q[n, :lq[n]], t[n, :lt[n]], norm)
            i = d.argmin(dim=1)  # the first minimum
            dist[n, :lq[n]] = d.gather(1, i[:, None])[:, 0]
            idx[n, :lq[n]] = i.to(torch.int32)
        out += [dist, idx]
    return tuple(out)


def chamfer_from_idx(x, y, idx_x, idx_y, x_lengths=None, y_lengths=None, weights=None, batch_reduction="mean",
                     point_reduction="mean", norm=2, single_directional=False):
    """The chamfer loss (upstream's reductions) of x, y in their dtype for GIVEN neighbour indices (-1: no term);
    differentiable w.r.t. x and y."""
    N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
    lx = torch.tensor(_lengths(x_lengths, N, P1), dtype=x.dtype)
    ly = torch.tensor(_lengths(y_lengths, N, P2), dtype=x.dtype)

    def side(q, t, idx, lq):
        has = (idx >= 0)
        nn = t.gather(1, idx.clamp(min=0).long()[..., None].expand(-1, -1, 3))
        df = q - nn
        d = (df[..., 0] ** 2 + df[..., 1] ** 2) + df[..., 2] ** 2 if norm == 2 else \
            (df[..., 0].abs() + df[..., 1].abs()) + df[..., 2].abs()
        c = (d * has.to(q.dtype)).sum(1)
        if weights is not None:
            c = c * weights.to(q.dtype)
        if point_reduction == "mean":
            c = c / lq.clamp(min=1)
        return c

    c = side(x, y, idx_x, lx)
    if not single_directional:
        c = c + side(y, x, idx_y, ly)
    if batch_reduction is None:
        return c
    c = c.sum()
    if batch_reduction == "mean":
        div = weights.to(x.dtype).sum() if weights is not None else max(N, 1)
        c = c / div
    return c


def chamfer_ref(x, y, idx=None, dtype=torch.float64, grad_out=None, **kw):
    """(loss, grad_x, grad_y) on the CPU in `dtype`. ``idx`` = (idx_x, idx_y) fixes the neighbours (the float32
    ones for a float64 gradient: a float64 argmin may pick another neighbour at a near tie, which is another
    function); None computes them in `dtype`. ``grad_out``: the upstream gradient (ones when None)."""
    xr = x.detach().cpu().to(dtype).requires_grad_(True)
    yr = y.detach().cpu().to(dtype).requires_grad_(True)
    if idx is None:
        _, ix, _, iy = nearest_ref(xr, yr, kw.get("x_lengths"), kw.get("y_lengths"), kw.get("norm", 2), dtype)
    else:
        ix, iy = idx
    w = kw.pop("weights", None)
    loss = chamfer_from_idx(xr, yr, ix, iy, weights=None if w is None else w.detach().cpu(), **kw)
    go = torch.ones_like(loss) if grad_out is None else grad_out.detach().cpu().to(dtype)
    gx, gy = torch.autograd.grad(loss, (xr, yr), go, allow_unused=True)
    return loss.detach(), torch.zeros_like(xr) if gx is None else gx, torch.zeros_like(yr) if gy is None else gy


def sample_ref(verts, faces, face_idx, uv):
    """Points (N,S,3) in verts' dtype: s = sqrt(u), w0 = 1 - s, w1 = s (1 - v), w2 = s v, p = (w0 a + w1 b) + w2 c
    over face face_idx's corners; zeros for a negative id. Differentiable w.r.t. verts."""
    u, v = uv[0].to(verts.dtype), uv[1].to(verts.dtype)
    s = u.sqrt()
    w0, w1, w2 = 1.0 - s, s * (1.0 - v), s * v
    has = face_idx >= 0
    tri = verts[faces.long()[face_idx.clamp(min=0).long()]]  # (N,S,3,3)
    p = (w0[..., None] * tri[..., 0, :] + w1[..., None] * tri[..., 1, :]) + w2[..., None] * tri[..., 2, :]
    return p * has[..., None].to(verts.dtype)


def face_areas_ref(verts, faces):
    a, b, c = (verts[faces[:, k].long()] for k in range(3))
    return 0.5 * torch.cross(b - a, c - a, dim=1).norm(dim=1)


def chamfer_composed(x, y):
    """chamfer_distance(x, y) with the default reductions composed from torch ops on the tensors' device: cdist ->
    min -> gather -> mean (the neighbour search carries no gradient; the gathers do). Materialises (N, P1, P2)."""
    with torch.no_grad():
        d = torch.cdist(x, y)
        ix, iy = d.argmin(dim=2), d.argmin(dim=1)
    cx = ((x - y.gather(1, ix[..., None].expand(-1, -1, 3))) ** 2).sum(-1).mean(1)
    cy = ((y - x.gather(1, iy[..., None].expand(-1, -1, 3))) ** 2).sum(-1).mean(1)
    return (cx + cy).mean()


def sample_composed(verts, faces, num_samples):
    """One mesh's sample_points_from_meshes composed from torch ops on the tensors' device: (1, S, 3)."""
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    with torch.no_grad():
        areas = 0.5 * torch.cross(b - a, c - a, dim=1).norm(dim=1)
        fi = torch.multinomial(areas[None], num_samples, replacement=True)[0]
        u, v = torch.rand(2, num_samples, device=verts.device)
        s = u.sqrt()
        w0, w1, w2 = 1.0 - s, s * (1.0 - v), s * v
    return (w0[:, None] * a[fi] + w1[:, None] * b[fi] + w2[:, None] * c[fi])[None]
