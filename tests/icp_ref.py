"""Plain-torch restatements, on the CPU and in any float dtype, of PyTorch3D's corresponding_points_alignment and
iterative_closest_point as torch_renderer_amd.ops builds them: the yardstick of test_icp_cpu.py / test_gpu_icp.py, and
``icp_composed`` is the baseline tools/icp_bench.py times on the device.

The alignment is Umeyama's: weighted means over max(sum w, eps), cov = Xc^T (w Yc) / sum w = U S V^T
(torch.linalg.svd), R = U E V^T with E = diag(1, 1, det(U V^T)) unless reflections are allowed, s = tr(E S) /
max(sum w |Xc|^2 / sum w, eps) or 1, T = Ymu - s Xmu R. The ICP loop searches the nearest target with
points_ref.pair_dist's operation order (first minimum), aligns the INITIAL source to the neighbours with the source
mask as weights, and stops when every cloud's relative rmse drop is <= the threshold. ``icp_ref`` also returns each
iteration's neighbour indices, so that two dtypes can be compared decision by decision.
"""
from typing import NamedTuple

import torch

from tests.points_ref import pair_dist


class RTs(NamedTuple):
    R: torch.Tensor
    T: torch.Tensor
    s: torch.Tensor


def apply_ref(X, R, T, s):
    return s[:, None, None] * torch.bmm(X, R) + T[:, None, :]


def align_ref(X, Y, weights=None, estimate_scale=False, allow_reflection=False, eps=1e-9, dtype=torch.float64):
    """RTs of X (N,P,3) -> Y (N,P,3) in `dtype`; weights (N,P) or None. A cloud without weight: the identity."""
    X, Y = X.detach().cpu().to(dtype), Y.detach().cpu().to(dtype)
    N, P, _ = X.shape
    w = torch.ones(N, P, dtype=dtype) if weights is None else weights.detach().cpu().to(dtype)
    tot = w.sum(1).clamp(min=eps)
    Xmu = (X * w[..., None]).sum(1) / tot[:, None]
    Ymu = (Y * w[..., None]).sum(1) / tot[:, None]
    Xc, Yc = X - Xmu[:, None], Y - Ymu[:, None]
    cov = torch.bmm(Xc.transpose(1, 2), Yc * w[..., None]) / tot[:, None, None]
    U, S, Vh = torch.linalg.svd(cov)
    E = torch.eye(3, dtype=dtype)[None].repeat(N, 1, 1)
    if not allow_reflection:
        E[:, 2, 2] = torch.det(torch.bmm(U, Vh))
    R = torch.bmm(torch.bmm(U, E), Vh)
    if estimate_scale:
        xcov = (w * (Xc ** 2).sum(2)).sum(1) / tot
        s = (torch.diagonal(E, dim1=1, dim2=2) * S).sum(1) / xcov.clamp(min=eps)
    else:
        s = torch.ones(N, dtype=dtype)
    T = Ymu - s[:, None] * torch.bmm(Xmu[:, None], R)[:, 0]
    empty = w.sum(1) <= 0
    if empty.any():
        R[empty], T[empty], s[empty] = torch.eye(3, dtype=dtype), 0.0, 1.0
    return RTs(R, T, s)


class ICPRef(NamedTuple):
    converged: bool
    rmse: object
    Xt: torch.Tensor
    RTs: RTs
    t_history: list
    nn_history: list   # per iteration (N, P1) int64 neighbour indices, -1 past the source length


def icp_ref(X, Y, x_lengths=None, y_lengths=None, init=None, max_iterations=100, relative_rmse_thr=1e-6,
            estimate_scale=False, allow_reflection=False, dtype=torch.float64):
    X, Y = X.detach().cpu().to(dtype), Y.detach().cpu().to(dtype)
    N, P1, _ = X.shape
    P2 = Y.shape[1]
    lx = [P1] * N if x_lengths is None else [int(v) for v in x_lengths.tolist()]
    ly = [P2] * N if y_lengths is None else [int(v) for v in y_lengths.tolist()]
    mask = (torch.arange(P1)[None] < torch.tensor(lx)[:, None]).to(dtype)
    if init is None:
        cur = RTs(torch.eye(3, dtype=dtype)[None].repeat(N, 1, 1), torch.zeros(N, 3, dtype=dtype),
                  torch.ones(N, dtype=dtype))
    else:
        cur = RTs(*(t.detach().cpu().to(dtype) for t in init))
    Xt = apply_ref(X, *cur)
    prev, rmse, converged, hist, nns = None, None, False, [], []
    for _ in range(max_iterations):
        idx = torch.full((N, P1), -1, dtype=torch.int64)
        nn = torch.zeros_like(X)
        for n in range(N):
            if lx[n] and ly[n]:
                i = pair_dist(Xt[n, :lx[n]], Y[n, :ly[n]]).argmin(dim=1)  # the first minimum
                idx[n, :lx[n]] = i
                nn[n, :lx[n]] = Y[n, i]
        cur = align_ref(X, nn, mask, estimate_scale, allow_reflection, dtype=dtype)
        Xt = apply_ref(X, *cur)
        hist.append(cur)
        nns.append(idx)
        sq = ((Xt - nn) ** 2).sum(2)
        rmse = ((sq * mask).sum(1) / mask.sum(1).clamp(min=1e-9)).sqrt()
        rel = torch.ones(N, dtype=dtype) if prev is None else (prev - rmse) / prev
        if bool((rel <= relative_rmse_thr).all()):
            converged = True
            break
        prev = rmse
    return ICPRef(converged, rmse, Xt, cur, hist, nns)


def rotations(axis, angle):
    """(N,3,3) float64 rotation matrices (Rodrigues) about `axis` (N,3) by `angle` (N,) radians."""
    a = axis.double() / axis.double().norm(dim=1, keepdim=True)
    K = torch.zeros(a.shape[0], 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -a[:, 2], a[:, 1], a[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -a[:, 0], -a[:, 1], a[:, 0]
    sn, cs = angle.double().sin()[:, None, None], angle.double().cos()[:, None, None]
    return torch.eye(3, dtype=torch.float64)[None] + sn * K + (1 - cs) * torch.bmm(K, K)


def registration_pair(N, P1, P2, x_lengths=None, y_lengths=None, scale=None, seed=0, noise=1e-3):
    """Seeded float32 (X (N,P1,3), Y (N,P2,3), true RTs): Gaussian sources; every target is a source point of its
    cloud (a random subset of the valid ones, drawn with replacement where more targets than sources are asked for)
    moved by a rotation <= 0.25 rad, a shift <= 0.3 and the cloud's scale, plus `noise` * N(0,1). Every cloud's
    transform is small (transforms that grow with the cloud index made float32 and float64 runs diverge)."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, P1, 3, generator=g)
    R = rotations(torch.randn(N, 3, generator=g), 0.25 * torch.rand(N, generator=g)).float()
    T = 0.17 * (2 * torch.rand(N, 3, generator=g) - 1)
    s = torch.ones(N) if scale is None else torch.tensor(scale, dtype=torch.float32)
    moved = apply_ref(X, R, T, s)
    Y = torch.zeros(N, P2, 3)
    for n in range(N):
        lx = P1 if x_lengths is None else int(x_lengths[n])
        ly = P2 if y_lengths is None else int(y_lengths[n])
        pick = torch.randperm(lx, generator=g)[:ly] if ly <= lx else torch.randint(0, lx, (ly,), generator=g)
        Y[n, :ly] = moved[n, pick] + noise * torch.randn(ly, 3, generator=g)
    return X, Y, RTs(R, T, s)


# name -> (N, P1, P2, x_lengths, y_lengths, scale, icp options): the shapes of the GPU suite (test_gpu_icp.py), whose
# input condition test_icp_cpu.py checks: the minimum size; heterogeneous lengths; two query tiles against two
# target chunks; scale; reflection allowed; many small clouds.
CASES = {
    "min": (1, 4, 4, None, None, None, {}),
    "het": (3, 300, 200, (300, 150, 40), (200, 64, 65), None, {}),
    "chunks": (2, 600, 1100, None, (1100, 1030), None, {}),
    "scale": (2, 257, 400, None, None, (1.1, 0.9), {"estimate_scale": True}),
    "reflect": (2, 257, 130, None, None, None, {"allow_reflection": True}),
    "many-64": (70, 64, 48, None, None, None, {}),
    "many-33": (300, 33, 20, None, None, None, {}),
    "init": (3, 300, 200, (300, 150, 40), (200, 64, 65), None, {"init": True}),
    "capped": (3, 300, 200, (300, 150, 40), (200, 64, 65), None, {"max_iterations": 2}),
}
_CACHE: dict = {}


def case(name):
    """(X, Y, x_lengths, y_lengths, icp keyword arguments) of a case, on the CPU, computed once and never modified.
    "init" starts from the true transform perturbed by 0.05 rad and a 0.05 shift."""
    if ("case", name) not in _CACHE:
        N, P1, P2, xl, yl, scale, opts = CASES[name]
        X, Y, true = registration_pair(N, P1, P2, xl, yl, scale, seed=sorted(CASES).index(name))
        kw = dict(opts)
        if kw.pop("init", False):
            g = torch.Generator().manual_seed(99)
            dR = rotations(torch.randn(N, 3, generator=g), torch.full((N,), 0.05)).float()
            kw["init"] = RTs(torch.bmm(true.R, dR), true.T + 0.05 * (2 * torch.rand(N, 3, generator=g) - 1), true.s)
        _CACHE["case", name] = (X, Y, None if xl is None else torch.tensor(xl), None if yl is None else torch.tensor(yl),
                                kw)
    return _CACHE["case", name]


def restated(name, dtype):
    """icp_ref of a case in `dtype`, computed once."""
    if (name, dtype) not in _CACHE:
        X, Y, xl, yl, kw = case(name)
        _CACHE[name, dtype] = icp_ref(X, Y, xl, yl, dtype=dtype, **kw)
    return _CACHE[name, dtype]


def icp_composed(X, Y, y_lengths=None, init=None, max_iterations=100, relative_rmse_thr=1e-6):
    """The same loop composed from torch ops on the tensors' device, full source clouds: cdist -> argmin -> gather ->
    torch.linalg.svd, with upstream's convergence test every iteration (one host read). Materialises (N, P1, P2).
    Returns (converged, rmse, Xt, (R, T, s), iterations)."""
    N, P1, _ = X.shape
    dev, dt = X.device, X.dtype
    R = torch.eye(3, device=dev, dtype=dt)[None].repeat(N, 1, 1)
    T, s = torch.zeros(N, 3, device=dev, dtype=dt), torch.ones(N, device=dev, dtype=dt)
    if init is not None:
        R, T, s = init
    Xt = s[:, None, None] * torch.bmm(X, R) + T[:, None, :]
    pad = None
    if y_lengths is not None:
        pad = torch.arange(Y.shape[1], device=dev)[None, None, :] >= y_lengths[:, None, None]
    Xmu = X.mean(1, keepdim=True)
    Xc = X - Xmu
    prev, rmse, converged, it = None, None, False, 0
    for it in range(1, max_iterations + 1):
        d = torch.cdist(Xt, Y)
        if pad is not None:
            d = d.masked_fill(pad, float("inf"))
        nn = Y.gather(1, d.argmin(dim=2)[..., None].expand(-1, -1, 3))
        Ymu = nn.mean(1, keepdim=True)
        U, _, Vh = torch.linalg.svd(torch.bmm(Xc.transpose(1, 2), nn - Ymu) / P1)
        E = torch.eye(3, device=dev, dtype=dt)[None].repeat(N, 1, 1)
        E[:, 2, 2] = torch.det(torch.bmm(U, Vh))
        R = torch.bmm(torch.bmm(U, E), Vh)
        T = (Ymu - torch.bmm(Xmu, R))[:, 0]
        Xt = torch.bmm(X, R) + T[:, None, :]
        rmse = ((Xt - nn) ** 2).sum(2).mean(1).sqrt()
        rel = torch.ones_like(rmse) if prev is None else (prev - rmse) / prev
        if bool((rel <= relative_rmse_thr).all()):
            converged = True
            break
        prev = rmse
    return converged, rmse, Xt, (R, T, s), it
