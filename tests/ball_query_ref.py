"""Plain-torch restatement of ball_query on the CPU: the yardstick of test_ball_query_cpu.py / test_gpu_ball_query.py.

Per cloud, ``points_ref.pair_dist`` on [:len1, :len2] (the kernels' operation order, one torch op per operation:
dx*dx, + dy*dy, + dz*dz), the mask ``d < r2`` with r2 = float32(radius) * float32(radius) rounded once to float32,
and a cumulative count over j: the hit whose count is c <= K goes to slot c - 1. In float32 the outputs are bitwise
what the kernel defines. Free slots and rows past len1 are 0 / -1.
"""
import functools

import torch

from tests import knn_ref as KR
from tests.points_ref import _lengths, pair_dist


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def radius2(radius):
    """float32(radius) * float32(radius), rounded once to float32 (a 0-dim float32 tensor)."""
    r = torch.tensor(float(radius), dtype=torch.float32)
    return r * r


def _wave_case():
    """P1 = 128 (both waves of one workgroup), P2 = 1025 (a second LDS chunk of one target). Queries 0..63 sit on the
    cluster of targets 0..7; queries 64..127 reach target 1024 alone; targets 8..1023 are far from both."""
    g = torch.Generator().manual_seed(7)
    p2 = torch.empty(1, 1025, 3)
    p2[0, :8] = 0.01 * torch.randn(8, 3, generator=g)
    p2[0, 8:1024] = 100.0 + torch.randn(1016, 3, generator=g)
    p2[0, 1024] = torch.tensor([10.0, 0.0, 0.0])
    p1 = 0.01 * torch.randn(1, 128, 3, generator=g)
    p1[0, 64:, 0] += 10.0
    return p1, p2, None, None


def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(p1, p2, lengths1, lengths2) of a named case on the CPU (never modified). "P1xP2" is one random cloud pair."""
    if name == "strict":  # d = 0.25 is not < 0.25
        return (torch.zeros(1, 1, 3), torch.tensor([[[0.5, 0.0, 0.0], [0.25, 0.0, 0.0]]]), None, None)
    if name in ("round0.7", "round0.1"):
        # a target at distance float32(radius) exactly (d == r2 in float32: no hit) and one an ulp nearer
        r = _f32(name[5:])
        below = torch.nextafter(r, _f32(0.0))
        z = _f32(0.0)
        return (torch.zeros(1, 1, 3), torch.stack([torch.stack([r, z, z]), torch.stack([z, below, z])])[None], None, None)
    if name == "first":  # 600 targets inside the radius of every query
        return 0.01 * _randn(1, 10, 3, seed=21), 0.01 * _randn(1, 600, 3, seed=22), None, None
    if name == "wave":
        return _wave_case()
    if name == "het":  # lengths with 0, 1 and full on both sides
        return (_randn(4, 257, 3, seed=1), _randn(4, 1000, 3, seed=2), torch.tensor([257, 1, 128, 0]),
                torch.tensor([1000, 1, 0, 500]))
    if name == "graph":
        return _randn(2, 300, 3, seed=31), _randn(2, 700, 3, seed=32), None, None
    dims = [int(v) for v in name.split("x")]
    N, P1, P2 = ([1] + dims) if len(dims) == 2 else dims
    return _randn(N, P1, 3, seed=P1), _randn(N, P2, 3, seed=P2 + 1), None, None


# name -> (radius, the Ks it runs at): the forward cases of test_gpu_ball_query.py::test_ball_query_bitwise
CASES = {
    "1x3": (100.0, (5,)),
    "strict": (0.5, (2,)),
    "round0.7": (0.7, (2,)),
    "round0.1": (0.1, (2,)),
    "first": (1.0, (500, 8)),
    "wave": (0.5, (4,)),
    "63x65": (1.0, (1, 7, 64)),
    "513x2049": (0.5, (1, 7, 64)),
    "het": (0.6, (8,)),
    "100x20000": (0.22, (16,)),   # the split path
    "257x1000": (0.7, (8,)),
}


def hit_counts(p1, p2, lengths1, lengths2, radius):
    """Per cloud, the number of targets inside the radius of every query (a list of (len1,) int64 tensors)."""
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    l1, l2 = _lengths(lengths1, N, P1), _lengths(lengths2, N, P2)
    r2 = radius2(radius)
    return [(pair_dist(p1[n, :l1[n]].float(), p2[n, :l2[n]].float()) < r2).sum(1) for n in range(N)]


def ball_query_ref(p1, p2, lengths1=None, lengths2=None, K=500, radius=0.2):
    """(dists (N,P1,K) float32, idx (N,P1,K) int32) on the CPU."""
    p1, p2 = p1.detach().cpu().float(), p2.detach().cpu().float()
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    l1, l2 = _lengths(lengths1, N, P1), _lengths(lengths2, N, P2)
    r2 = radius2(radius)
    dists = torch.zeros((N, P1, K), dtype=torch.float32)
    idx = torch.full((N, P1, K), -1, dtype=torch.int32)
    for n in range(N):
        if l1[n] == 0 or l2[n] == 0:
            continue
        d = pair_dist(p1[n, :l1[n]], p2[n, :l2[n]])
        hit = d < r2
        count = torch.cumsum(hit, 1)  # 1-based place of a hit among its query's hits, over j
        keep = hit & (count <= K)
        i, j = keep.nonzero(as_tuple=True)
        slot = count[i, j] - 1
        idx[n, i, slot] = j.to(torch.int32)
        dists[n, i, slot] = d[i, j]
    return dists, idx


def dists_from_idx(p1, p2, idx):
    """dists (N,P1,K) in the inputs' dtype for GIVEN neighbours (idx < 0: a free slot, 0 and no gradient)."""
    return KR.dists_from_idx(p1, p2, idx, 2)


def grad_ref(p1, p2, idx, g, dtype=torch.float64):
    """(grad_p1, grad_p2) of sum(g * dists) on the CPU in `dtype`, for the given (float32-chosen) neighbours. Entries
    of g in free slots are ignored (they may be nan)."""
    return KR.knn_grad_ref(p1, p2, idx, g, 2, dtype)
