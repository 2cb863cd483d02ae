"""Plain-torch restatement of knn_points on the CPU: the yardstick of test_knn_cpu.py / test_gpu_knn.py.

Per cloud, ``points_ref.pair_dist`` on [:len1, :len2] (the kernels' operation order, one torch op per operation), then
a STABLE sort of every row: among equal distances the lowest index comes first, which is the kernels' key order
(distance, index), inside the K kept and at the K-th / (K+1)-th boundary. In float32 the outputs are bitwise what the
kernels define. Slots k >= min(K, len2) and rows past len1 are 0 / -1 (the low-level convention of nearest_points).
"""
import functools

import torch

from tests.points_ref import _lengths, pair_dist


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def lattice_ties():
    """Targets: the 4x4x4 integer lattice twice over; queries: lattice + 0.5. Every distance occurs an even number of times
    per query (test_knn_cpu.py counts the queries whose K-th and (K+1)-th distances are equal)."""
    r = torch.arange(4, dtype=torch.float32)
    lat = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    return (lat + 0.5)[None], torch.cat([lat, lat], 0)[None]


@functools.lru_cache(maxsize=None)
def case(name):
    """(p1, p2, lengths1, lengths2) of a named case on the CPU (never modified). "P1xP2" is one random cloud pair,
    "NxP1xP2" a batch of N."""
    if name == "ties":
        return lattice_ties() + (None, None)
    if name == "dup":  # 40 identical targets: the K kept are indices 0..K-1
        return _randn(1, 10, 3, seed=11), _randn(1, 1, 3, seed=12).expand(1, 40, 3).contiguous(), None, None
    if name == "het":  # an empty query cloud, an empty target cloud, and len2 < K
        return (_randn(4, 257, 3, seed=1), _randn(4, 1000, 3, seed=2), torch.tensor([257, 1, 128, 0]),
                torch.tensor([500, 1000, 0, 3]))
    dims = [int(v) for v in name.split("x")]
    N, P1, P2 = ([1] + dims) if len(dims) == 2 else dims
    return _randn(N, P1, 3, seed=P1), _randn(N, P2, 3, seed=P2 + 1), None, None


# the forward cases of test_gpu_knn.py::test_knn_bitwise and the K each runs at
CASES = {"1x1": (1,), "1x3": (8,), "63x65": (1, 2, 3, 8, 16, 32), "257x1000": (5, 32), "ties": (3, 8, 12),
         "dup": (8,), "het": (8,), "8x100x20000": (8,), "600x1x1100": (4,), "1x1000x1000": (16,),
         "256x1x40": (2, 16, 32)}


def sorted_dists(q, t, norm=2):
    """(values, indices) of every query's distances to all targets, ascending by (distance, index)."""
    return torch.sort(pair_dist(q, t, norm), dim=1, stable=True)


def knn_ref(p1, p2, lengths1=None, lengths2=None, K=1, norm=2, dtype=torch.float32):
    """(dists (N,P1,K) dtype, idx (N,P1,K) int32) on the CPU."""
    p1, p2 = p1.detach().cpu().to(dtype), p2.detach().cpu().to(dtype)
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    l1, l2 = _lengths(lengths1, N, P1), _lengths(lengths2, N, P2)
    dists = torch.zeros((N, P1, K), dtype=dtype)
    idx = torch.full((N, P1, K), -1, dtype=torch.int32)
    for n in range(N):
        k = min(K, l2[n])
        if l1[n] == 0 or k == 0:
            continue
        v, i = sorted_dists(p1[n, :l1[n]], p2[n, :l2[n]], norm)
        dists[n, :l1[n], :k] = v[:, :k]
        idx[n, :l1[n], :k] = i[:, :k].to(torch.int32)
    return dists, idx


def dists_from_idx(p1, p2, idx, norm=2):
    """dists (N,P1,K) in the inputs' dtype for GIVEN neighbours (idx < 0: a padded slot, 0 and no gradient);
    differentiable w.r.t. p1 and p2."""
    has = idx >= 0
    N, P1, K = idx.shape
    nn = p2[:, :, None].expand(-1, -1, K, -1).gather(1, idx.clamp(min=0).long()[..., None].expand(-1, -1, -1, 3))
    df = p1[:, :, None, :] - nn
    d = (df[..., 0] ** 2 + df[..., 1] ** 2) + df[..., 2] ** 2 if norm == 2 else \
        (df[..., 0].abs() + df[..., 1].abs()) + df[..., 2].abs()
    return torch.where(has, d, torch.zeros_like(d))


def knn_grad_ref(p1, p2, idx, g, norm=2, dtype=torch.float64):
    """(grad_p1, grad_p2) of sum(g * dists) on the CPU in `dtype`, for the given (float32-chosen) neighbours. Entries
    of g in padded slots are ignored (they may be nan)."""
    a = p1.detach().cpu().to(dtype).requires_grad_(True)
    b = p2.detach().cpu().to(dtype).requires_grad_(True)
    idx = idx.detach().cpu()
    gg = torch.where(idx >= 0, g.detach().cpu().to(dtype), torch.zeros((), dtype=dtype))
    ga, gb = torch.autograd.grad((dists_from_idx(a, b, idx, norm) * gg).sum(), (a, b), allow_unused=True)
    return (torch.zeros_like(a) if ga is None else ga), (torch.zeros_like(b) if gb is None else gb)
