"""Plain-torch restatement of loss.posed_chamfer_distance (one cloud pair under S poses): the yardstick of
test_pose_chamfer_cpu.py / test_gpu_pose_chamfer.py, built on tests/points_ref.py.

``posed_points`` keeps the kernels' transform order, x'_c = s * ((x_0 R_0c + x_1 R_1c) + x_2 R_2c) + T_c, one torch op
per operation (no FMA), so that in float32 on the CPU it is bitwise what the library's transform code gives, and
``posed_nearest_ref`` what the kernel's neighbour search defines (ties to the first index). ``pose_moments`` /
``pose_grad_from_moments`` restate the moment form of the backward: 13 sums per direction, combined into d loss /
d (R, T, s).
"""
import torch

from tests.points_ref import chamfer_from_idx, nearest_ref


def _pose(R, T, s, dtype):
    S = R.shape[0]
    s = torch.ones(S, dtype=dtype) if s is None else s.to(dtype)
    return R.to(dtype), T.reshape(S, 3).to(dtype), s


def _cloud(c, dtype):
    return c.reshape(-1, 3).to(dtype)


def posed_points(x, R, T, s=None, dtype=torch.float32):
    """(S,P,3) = s (x R) + T for row vectors, in `dtype`, in the kernels' operation order. Differentiable."""
    x = _cloud(x, dtype)
    R, T, s = _pose(R, T, s, dtype)
    cols = []
    for c in range(3):
        v = (x[None, :, 0] * R[:, None, 0, c] + x[None, :, 1] * R[:, None, 1, c]) + x[None, :, 2] * R[:, None, 2, c]
        cols.append(s[:, None] * v + T[:, None, c])
    return torch.stack(cols, -1)


def posed_nearest_ref(x, y, R, T, s=None, norm=2, dtype=torch.float32):
    """(dist_x (S,P1), idx_x, dist_y (S,P2), idx_y) of the S transformed copies of x against y, on the CPU."""
    xt = posed_points(x.detach().cpu(), R.detach().cpu(), T.detach().cpu(), None if s is None else s.detach().cpu(),
                      dtype)
    ye = _cloud(y.detach().cpu(), dtype)[None].expand(xt.shape[0], -1, -1)
    return nearest_ref(xt, ye, norm=norm, dtype=dtype)


def posed_chamfer_from_idx(x, y, R, T, s, idx_x, idx_y, norm=2, point_reduction="mean", single_directional=False):
    """(S,) loss in R's dtype for GIVEN neighbours; differentiable w.r.t. R, T and s."""
    dtype = R.dtype
    xt = posed_points(x, R, T, s, dtype)
    ye = _cloud(y, dtype)[None].expand(xt.shape[0], -1, -1)
    return chamfer_from_idx(xt, ye, idx_x, idx_y, batch_reduction=None, point_reduction=point_reduction, norm=norm,
                            single_directional=single_directional)


def posed_chamfer_ref(x, y, R, T, s=None, idx=None, dtype=torch.float64, grad_out=None, **kw):
    """(loss (S,), grad_R, grad_T (S,3), grad_s) on the CPU in `dtype` by torch autograd. ``idx`` = (idx_x, idx_y)
    fixes the neighbours (the GPU's, for a float64 gradient of the same function); None computes them in `dtype`."""
    S = R.shape[0]
    Rr = R.detach().cpu().to(dtype).requires_grad_(True)
    Tr = T.detach().cpu().reshape(S, 3).to(dtype).requires_grad_(True)
    sr = (torch.ones(S) if s is None else s.detach().cpu()).to(dtype).requires_grad_(True)
    xc, yc = x.detach().cpu(), y.detach().cpu()
    if idx is None:
        _, ix, _, iy = posed_nearest_ref(xc, yc, Rr, Tr, sr, kw.get("norm", 2), dtype)
    else:
        ix, iy = (None if i is None else i.detach().cpu() for i in idx)
    loss = posed_chamfer_from_idx(xc, yc, Rr, Tr, sr, ix, iy, **kw)
    go = torch.ones_like(loss) if grad_out is None else grad_out.detach().cpu().to(dtype)
    gR, gT, gs = torch.autograd.grad(loss, (Rr, Tr, sr), go)
    return loss.detach(), gR, gT, gs


def pose_moments(x, y, R, T, s, idx_x, idx_y, norm=2, dtype=torch.float64):
    """(2,S,13) pose moments per direction: sum g (3), sum x^T g (9, row = x component), sum (x R).g, with
    g = x' - y of every (source point, target point) pair (its sign for norm 1) and x the pair's untransformed
    source point. Direction 0 pairs (x_i, y_nn(i)), direction 1 pairs (x_nn(j), y_j). idx_y None: zeros there."""
    xs, ys = _cloud(x, dtype), _cloud(y, dtype)
    Rd, Td, sd = _pose(R, T, s, dtype)
    S = Rd.shape[0]
    xt = posed_points(xs, Rd, Td, sd, dtype)
    xr = torch.einsum("pa,sab->spb", xs, Rd)
    out = torch.zeros(2, S, 13, dtype=dtype)
    for d, idx in enumerate((idx_x, idx_y)):
        if idx is None:
            continue
        i = idx.long()
        if d == 0:
            src = xs[None].expand(S, -1, -1)
            g = xt - ys[i]
            r = xr
        else:
            src = xs[i]
            g = xt.gather(1, i[..., None].expand(-1, -1, 3)) - ys[None]
            r = xr.gather(1, i[..., None].expand(-1, -1, 3))
        if norm == 1:
            g = torch.sign(g)
        out[d, :, 0:3] = g.sum(1)
        out[d, :, 3:12] = torch.einsum("spa,spb->sab", src, g).reshape(S, 9)
        out[d, :, 12] = (r * g).sum((1, 2))
    return out


def pose_grad_from_moments(mom, s, P1, P2, norm=2, point_reduction="mean", single_directional=False):
    """(S,13) = d loss[k] / d (R row-major, T, s) of pose k from ``pose_moments``."""
    S = mom.shape[1]
    k = 2.0 if norm == 2 else 1.0
    c = [1.0 / max(P1, 1), 1.0 / max(P2, 1)] if point_reduction == "mean" else [1.0, 1.0]
    m = c[0] * mom[0] + (0.0 if single_directional else c[1]) * mom[1]
    sc = torch.ones(S, dtype=mom.dtype) if s is None else s.to(mom.dtype)
    return torch.cat((k * sc[:, None] * m[:, 3:12], k * m[:, 0:3], k * m[:, 12:13]), 1)
