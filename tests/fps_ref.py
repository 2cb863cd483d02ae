"""Plain-torch restatement of sample_farthest_points on the CPU: the yardstick of test_fps_cpu.py / test_gpu_fps.py.

Per cloud n, with L = lengths[n] and k_n = min(K[n], L): the first index is start[n]; m = +inf for every point p < L;
after each selection s, m = minimum(m, d(., s)) with d = (dx*dx + dy*dy) + dz*dz, one torch op per operation in
float32 (the kernels' operation order, so the values are bitwise the kernels'), and the next index is the FIRST
position of max(m): the lowest index among equal values. A selected point stays in the running with m = 0. Slots
k >= k_n are -1 / 0 (the low-level convention of kernels.farthest_points).
"""
import functools

import torch


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def lattice():
    """The 4x4x4 integer lattice in index order: every distance is an exact integer and most maxima are shared."""
    r = torch.arange(4, dtype=torch.float32)
    return torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(1, -1, 3)


@functools.lru_cache(maxsize=None)
def cloud(N, P, seed=None):
    """A random (N, P, 3) float32 batch on the CPU (never modified)."""
    return _randn(N, P, 3, seed=P if seed is None else seed)


@functools.lru_cache(maxsize=None)
def case(name):
    """(points, lengths, K, start_idx) of a named case on the CPU (never modified). "NxPkK" is a random batch."""
    if name == "lattice":
        return lattice(), None, 20, None
    if name == "same":  # 70 identical points: start, then index 0 for ever
        return _randn(1, 1, 3, seed=5).expand(1, 70, 3).contiguous(), None, 6, torch.tensor([3])
    if name == "ragged":  # an empty cloud, one point, seven points, a full cloud
        return cloud(4, 300), torch.tensor([0, 1, 7, 300]), 12, None
    if name == "klist":  # K per cloud, above and below the lengths, and 0
        return cloud(4, 300), torch.tensor([0, 1, 7, 300]), (5, 9, 3, 0), None
    if name == "kmore":  # K[n] > lengths[n] everywhere but the last cloud
        return cloud(3, 90), torch.tensor([4, 90, 60]), (8, 100, 60), None
    if name == "start":
        return cloud(3, 300), torch.tensor([300, 150, 2]), 10, torch.tensor([299, 77, 1])
    dims, K = name.split("k")
    N, P = (int(v) for v in dims.split("x"))
    return cloud(N, P), None, int(K), None


def register_capacity(geometry):
    """The largest P that ``geometry(1, P, 1)`` (kernels.farthest_geometry) does not report as streamed."""
    hi = 1
    while not geometry(1, hi, 1)[2]:
        hi *= 2
    lo = hi // 2  # not streamed
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if geometry(1, mid, 1)[2] else (mid, hi)
    return lo


def _per_cloud(v, N, default):
    if v is None:
        return [default] * N
    if torch.is_tensor(v):
        return [int(i) for i in v.tolist()]
    if isinstance(v, (list, tuple)):
        return [int(i) for i in v]
    return [int(v)] * N


def sq_dist(pts, s):
    """(L,) float32 squared distances of the points to pts[s], in the kernels' operation order."""
    df = pts - pts[s]
    return (df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1]) + df[:, 2] * df[:, 2]


def fps_ref(points, lengths=None, K=50, start_idx=None, dtype=torch.float32):
    """(idx (N,Kmax) int32, pts (N,Kmax,3) dtype) on the CPU."""
    points = points.detach().cpu().to(dtype)
    N, P = points.shape[0], points.shape[1]
    Ls, Ks, starts = _per_cloud(lengths, N, P), _per_cloud(K, N, 0), _per_cloud(start_idx, N, 0)
    Kmax = max(Ks) if Ks else 0
    idx = torch.full((N, Kmax), -1, dtype=torch.int32)
    pts = torch.zeros((N, Kmax, 3), dtype=dtype)
    for n in range(N):
        L, kn = Ls[n], min(Ks[n], Ls[n])
        if kn == 0:
            continue
        c = points[n, :L]
        m = torch.full((L,), float("inf"), dtype=dtype)
        cur = starts[n]
        for k in range(kn):
            idx[n, k] = cur
            pts[n, k] = c[cur]
            if k + 1 == kn:
                break
            m = torch.minimum(m, sq_dist(c, cur))
            cur = int((m == m.max()).nonzero()[0, 0])  # the first position of the maximum
    return idx, pts
