"""A plain-torch restatement, on the CPU, of ops.iterative_closest_point_to_plane's rule (include/mi355r.h): the
yardstick of test_icp_plane_cpu.py / test_gpu_icp_plane.py, and ``icp_plane_composed`` is the baseline
tools/icp_plane_bench.py times on the device.

What the rule fixes in float32 is float32 here too, one torch op per operation: the transform s (x R) + T in
sim_apply's order, the squared distance of points_ref.pair_dist with the first minimum, the validity test against
r2 = float32(d) * float32(d), the stored transform and the rmse. The normal equations (c, r, J, A, b) are formed in
``dtype``: float64 is the restatement, float32 the conditioning probe (the same run with moments of float32 accuracy).
The 6x6 solve (numpy-free: torch.linalg.solve on A + lam I), Rodrigues and the update are always float64.
``icp_plane_ref`` returns every iteration's transform, neighbour indices, validity and squared distances, so that two
runs can be compared decision by decision.
"""
import math
from typing import NamedTuple

import torch

from tests.icp_ref import RTs, rotations
from tests.points_ref import pair_dist

RADII = (1.0, 0.7, 0.5)


def sim_apply_ref(X, R, T, s):
    """s (x R) + T of X (N,P,3) in X's dtype with the kernels' operation order (no FMA: one torch op each)."""
    out = []
    for b in range(3):
        acc = (X[..., 0] * R[:, None, 0, b] + X[..., 1] * R[:, None, 1, b]) + X[..., 2] * R[:, None, 2, b]
        out.append(s[:, None] * acc + T[:, None, b])
    return torch.stack(out, dim=-1)


def skew(w):
    K = torch.zeros(3, 3, dtype=w.dtype)
    K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
    return K


def rodrigues(w):
    """exp([w]x) (3,3) in float64; the series below |w| = 1e-4, as the rule has it."""
    w = w.double()
    th2 = float((w * w).sum())
    th = math.sqrt(th2)
    if th < 1e-4:
        ka, kb = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        ka, kb = math.sin(th) / th, (1.0 - math.cos(th)) / th2
    K = skew(w)
    return torch.eye(3, dtype=torch.float64) + ka * K + kb * (K @ K)


def plane_step_ref(A, b, R, T, c):
    """Steps 3 and 4 on one cloud in float64: (R', T') float64 before the rounding to float32. A (6,6), b (6), R (3,3)
    and T (3) the float32 transform's values, c (3). trace(A) == 0: the transform as it is."""
    A, b, R, T, c = (t.double() for t in (A, b, R, T, c))
    tr = float(torch.diagonal(A).sum())
    if not tr > 0.0:
        return R.clone(), T.clone()
    lam = 1e-9 * tr / 6.0
    xi = torch.linalg.solve(A + lam * torch.eye(6, dtype=torch.float64), -b)
    E = rodrigues(xi[:3])
    return R @ E.T, (T - c) @ E.T + c + xi[3:]


class ICPPlaneRef(NamedTuple):
    converged: bool
    rmse: object
    Xt: torch.Tensor
    RTs: RTs
    t_history: list
    nn_history: list      # per iteration (N, P1) int64: the neighbour of every source point, -1 past the length
    valid_history: list   # per iteration (N, P1) bool
    d2_history: list      # per iteration (N, P1) float32 squared distances to the neighbour (0 past the length)
    rel_history: list     # per iteration (N,) float32: the relative rmse drop the status test saw


def icp_plane_ref(X, Y, Yn, x_lengths=None, y_lengths=None, init=None, max_iterations=100, relative_rmse_thr=1e-6,
                  max_correspondence_distance=None, dtype=torch.float64):
    X, Y, Yn = X.detach().cpu().float(), Y.detach().cpu().float(), Yn.detach().cpu().float()
    N, P1, _ = X.shape
    P2 = Y.shape[1]
    lx = [P1] * N if x_lengths is None else [int(v) for v in x_lengths.tolist()]
    ly = [P2] * N if y_lengths is None else [int(v) for v in y_lengths.tolist()]
    if init is None:
        R, T, s = torch.eye(3)[None].repeat(N, 1, 1), torch.zeros(N, 3), torch.ones(N)
    else:
        R, T, s = (t.detach().cpu().float().clone() for t in init)
    r2 = None
    if max_correspondence_distance is not None:
        d = torch.tensor(max_correspondence_distance, dtype=torch.float32)
        r2 = d * d
    mx = torch.stack([X[n, :lx[n]].double().mean(0) if lx[n] else torch.zeros(3, dtype=torch.float64) for n in range(N)])
    thr = torch.tensor(relative_rmse_thr, dtype=torch.float32)
    prev, rmse, converged = None, None, False
    hist, nns, valids, d2s, rels = [], [], [], [], []
    for _ in range(max_iterations):
        P = sim_apply_ref(X, R, T, s)  # float32
        idx = torch.full((N, P1), -1, dtype=torch.int64)
        valid = torch.zeros(N, P1, dtype=torch.bool)
        d2 = torch.zeros(N, P1)
        Rn, Tn = R.clone(), T.clone()
        m = torch.zeros(N)
        for n in range(N):
            if lx[n] and ly[n]:
                dm = pair_dist(P[n, :lx[n]], Y[n, :ly[n]])
                i = dm.argmin(dim=1)  # the first minimum
                idx[n, :lx[n]] = i
                d2[n, :lx[n]] = dm.gather(1, i[:, None])[:, 0]
                valid[n, :lx[n]] = True if r2 is None else d2[n, :lx[n]] <= r2
            v = valid[n]
            m[n] = float(v.sum())
            c64 = s[n].double() * (mx[n] @ R[n].double()) + T[n].double()
            p, q, nn = P[n, v].to(dtype), Y[n, idx[n, v]].to(dtype), Yn[n, idx[n, v]].to(dtype)
            c = c64.to(dtype)
            r = ((p - q) * nn).sum(1)
            J = torch.cat([torch.cross(p - c, nn, dim=1), nn], dim=1)  # (m, 6)
            A, b = J.T @ J, J.T @ r
            R64, T64 = plane_step_ref(A, b, R[n], T[n], c64)
            Rn[n], Tn[n] = R64.float(), T64.float()
        R, T = Rn, Tn
        hist.append(RTs(R.clone(), T.clone(), s.clone()))
        nns.append(idx)
        valids.append(valid)
        d2s.append(d2)
        P2_ = sim_apply_ref(X, R, T, s)
        sq = torch.zeros(N, dtype=torch.float64)
        for n in range(N):
            v = valid[n]
            rr = ((P2_[n, v].double() - Y[n, idx[n, v]].double()) * Yn[n, idx[n, v]].double()).sum(1)
            sq[n] = (rr * rr).sum()
        rmse = (sq / m.double().clamp(min=1.0)).sqrt().float()
        rel = torch.ones(N) if prev is None else (prev - rmse) / prev
        rels.append(rel)
        done = (rel <= thr) | (m == 0)
        prev = rmse
        if bool(done.all()):
            converged = True
            break
    Xt = sim_apply_ref(X, R, T, s)
    return ICPPlaneRef(converged, rmse, Xt, RTs(R, T, s), hist, nns, valids, d2s, rels)


def ellipsoid(P, generator):
    """(points (P,3), unit normals (P,3)) float32 on the ellipsoid of RADII: uniform directions scaled by the radii,
    the normal along the gradient x / a^2."""
    u = torch.randn(P, 3, generator=generator, dtype=torch.float64)
    u = u / u.norm(dim=1, keepdim=True)
    rad = torch.tensor(RADII, dtype=torch.float64)
    pts = u * rad
    nrm = pts / (rad * rad)
    return pts.float(), (nrm / nrm.norm(dim=1, keepdim=True)).float()


def plane_pair(N, P1, P2, x_lengths=None, y_lengths=None, seed=0, noise=1e-3, scale=1.0, min_deg=10.0, max_deg=25.0):
    """Seeded float32 (X (N,P1,3), Y (N,P2,3), Yn (N,P2,3), truth RTs taking X onto Y). Y: `scale` times a sample of
    the ellipsoid, with its analytic normals. X: another sample plus `noise` N(0,1), moved by a rotation of
    min_deg..max_deg degrees about a random axis and a translation of length 0.05..0.1. Rows past a length are zero."""
    g = torch.Generator().manual_seed(seed)
    X, Y, Yn = torch.zeros(N, P1, 3), torch.zeros(N, P2, 3), torch.zeros(N, P2, 3)
    ang = torch.deg2rad(min_deg + (max_deg - min_deg) * torch.rand(N, generator=g))
    Rm = rotations(torch.randn(N, 3, generator=g), ang)  # float64
    d = torch.randn(N, 3, generator=g, dtype=torch.float64)
    Tm = d / d.norm(dim=1, keepdim=True) * (0.05 + 0.05 * torch.rand(N, 1, generator=g, dtype=torch.float64))
    for n in range(N):
        l1 = P1 if x_lengths is None else int(x_lengths[n])
        l2 = P2 if y_lengths is None else int(y_lengths[n])
        yp, yn = ellipsoid(l2, g)
        Y[n, :l2], Yn[n, :l2] = scale * yp, yn
        xp, _ = ellipsoid(l1, g)
        xp = xp.double() + noise * torch.randn(l1, 3, generator=g, dtype=torch.float64)
        X[n, :l1] = (xp @ Rm[n] + Tm[n]).float()
    Rt = Rm.transpose(1, 2)  # y = scale ((x - Tm) Rm^T)
    truth = RTs(Rt.float(), (-scale * torch.bmm(Tm[:, None], Rt)[:, 0]).float(), torch.full((N,), scale))
    return X, Y, Yn, truth


# name -> (N, P1, P2, x_lengths, y_lengths, seed, data options, call options): the GPU suite's inputs
# (test_gpu_icp_plane.py), whose condition test_icp_plane_cpu.py checks. Every case runs at relative_rmse_thr = THR =
# 1e-4. Once a registration stagnates, the float32 rmse moves by about +-1e-6 of itself from one iteration to the next
# (the transform's rounding), so at the default 1e-6 the iteration that stops the loop is decided by rounding: the run
# with float32 moments stopped after 9 iterations on one CPU and 6 on another. At 1e-4 every drop of every case lies at
# least 5x above or below the threshold (asserted in test_icp_plane_cpu.py).
THR = 1e-4
_HET = (3, 300, 400, (300, 150, 64), (400, 257, 300))
CASES = {
    "het": (*_HET, 1, {}, {"relative_rmse_thr": THR}),
    "chunks": (2, 600, 1100, None, (1100, 1030), 2, {}, {"relative_rmse_thr": THR}),
    "tiles": (1, 2049, 1100, None, None, 3, {}, {"relative_rmse_thr": THR}),
    "init": (*_HET, 4, {}, {"relative_rmse_thr": THR, "init": True}),
    "scaled": (*_HET, 5, {"scale": 0.9}, {"relative_rmse_thr": THR, "init_scale": 0.9}),
    "maxd": (1, 300, 400, None, None, 6, {"displace": 40}, {"relative_rmse_thr": THR, "max_correspondence_distance": 0.15}),
    "capped": (*_HET, 7, {}, {"relative_rmse_thr": THR, "max_iterations": 2}),
}
DISPLACED = 40   # "maxd": 40 source points are moved by (0.6, 0.6, 0.6)
_CACHE: dict = {}


def displaced(x, k=DISPLACED):
    """The indices of the k points of x (P,3) with the largest x + y + z, ascending."""
    return torch.topk(x.double().sum(1), k).indices.sort().values


def case(name):
    """(X, Y, Yn, x_lengths, y_lengths, keyword arguments of icp_plane_ref) of a case, on the CPU, computed once and
    never modified. "init" starts 4 degrees and a 0.02 shift off the truth; "scaled" from (I, 0, 0.9) with the target
    scaled by 0.9; "maxd" is a 10-12 degree motion, so that the bulk of the pairs starts inside the distance."""
    if ("case", name) not in _CACHE:
        N, P1, P2, xl, yl, seed, data, opts = CASES[name]
        data = dict(data)
        displace = data.pop("displace", 0)
        if displace:
            data.update(min_deg=10.0, max_deg=12.0)
        X, Y, Yn, truth = plane_pair(N, P1, P2, xl, yl, seed=seed, **data)
        if displace:  # the points furthest along (1, 1, 1): moved outwards, away from every part of the surface
            X = X.clone()
            for n in range(N):
                X[n, displaced(X[n], displace)] += 0.6
        kw = dict(opts)
        if kw.pop("init", False):
            g = torch.Generator().manual_seed(99)
            dR = rotations(torch.randn(N, 3, generator=g), torch.full((N,), math.radians(4.0))).float()
            kw["init"] = RTs(torch.bmm(truth.R, dR), truth.T + 0.02 * (2 * torch.rand(N, 3, generator=g) - 1), truth.s)
        if "init_scale" in kw:
            kw["init"] = RTs(torch.eye(3)[None].repeat(N, 1, 1), torch.zeros(N, 3), torch.full((N,), kw.pop("init_scale")))
        _CACHE["case", name] = (X, Y, Yn, None if xl is None else torch.tensor(xl),
                                None if yl is None else torch.tensor(yl), kw)
    return _CACHE["case", name]


def restated(name, dtype):
    """icp_plane_ref of a case with moments in `dtype`, computed once."""
    if (name, dtype) not in _CACHE:
        X, Y, Yn, xl, yl, kw = case(name)
        _CACHE[name, dtype] = icp_plane_ref(X, Y, Yn, xl, yl, dtype=dtype, **kw)
    return _CACHE[name, dtype]


def plane_rmse(Xt, Y, Yn, y_lengths=None):
    """(N,) point-to-plane rmse of Xt (N,P1,3) against its nearest points of Y with normals Yn, on Xt's device, every
    source point counted: the common measure tools/icp_plane_bench.py reports for both estimators."""
    d = torch.cdist(Xt, Y)
    if y_lengths is not None:
        d = d.masked_fill(torch.arange(Y.shape[1], device=Y.device)[None, None, :] >= y_lengths[:, None, None], float("inf"))
    j = d.argmin(dim=2)[..., None].expand(-1, -1, 3)
    return (((Xt - Y.gather(1, j)) * Yn.gather(1, j)).sum(2) ** 2).mean(1).sqrt()


def icp_plane_composed(X, Y, Yn, y_lengths=None, init=None, max_iterations=100, relative_rmse_thr=1e-6):
    """The same estimator composed from torch ops on the tensors' device, full source clouds, float32: cdist ->
    argmin -> gather -> normal equations -> torch.linalg.solve, the convergence test every iteration (one host read).
    Materialises (N, P1, P2). Returns (converged, rmse, Xt, (R, T, s), iterations)."""
    N, P1, _ = X.shape
    dev, dt = X.device, X.dtype
    R = torch.eye(3, device=dev, dtype=dt)[None].repeat(N, 1, 1)
    T, s = torch.zeros(N, 3, device=dev, dtype=dt), torch.ones(N, device=dev, dtype=dt)
    if init is not None:
        R, T, s = init
    pad = None
    if y_lengths is not None:
        pad = torch.arange(Y.shape[1], device=dev)[None, None, :] >= y_lengths[:, None, None]
    eye6 = torch.eye(6, device=dev, dtype=dt)[None]
    Xt = s[:, None, None] * torch.bmm(X, R) + T[:, None, :]
    prev, rmse, converged, it = None, None, False, 0
    for it in range(1, max_iterations + 1):
        d = torch.cdist(Xt, Y)
        if pad is not None:
            d = d.masked_fill(pad, float("inf"))
        j = d.argmin(dim=2)[..., None].expand(-1, -1, 3)
        q, n = Y.gather(1, j), Yn.gather(1, j)
        c = Xt.mean(1, keepdim=True)
        r = ((Xt - q) * n).sum(2)
        J = torch.cat([torch.cross(Xt - c, n, dim=2), n], dim=2)
        A = torch.bmm(J.transpose(1, 2), J)
        b = torch.bmm(J.transpose(1, 2), r[..., None])[..., 0]
        lam = 1e-9 * torch.diagonal(A, dim1=1, dim2=2).sum(1) / 6.0
        xi = torch.linalg.solve(A + lam[:, None, None] * eye6, -b)
        w, t = xi[:, :3], xi[:, 3:]
        K = torch.zeros(N, 3, 3, device=dev, dtype=dt)
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -w[:, 2], w[:, 1], w[:, 2]
        K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 0], -w[:, 1], w[:, 0]
        E = torch.linalg.matrix_exp(K)
        Et = E.transpose(1, 2)
        c = c[:, 0]
        R = torch.bmm(R, Et)
        T = torch.bmm((T - c)[:, None], Et)[:, 0] + c + t
        Xt = s[:, None, None] * torch.bmm(X, R) + T[:, None, :]
        rmse = (((Xt - q) * n).sum(2) ** 2).mean(1).sqrt()
        rel = torch.ones_like(rmse) if prev is None else (prev - rmse) / prev
        if bool((rel <= relative_rmse_thr).all()):
            converged = True
            break
        prev = rmse
    return converged, rmse, Xt, (R, T, s), it
