"""ball_query(grid=) on the MI355X (k_ball_query_grid of csrc/mr_ballquery.hip): idx and the bit patterns of dists
equal the float32 restatement of tests/ball_query_ref.py, which is what the brute-force ball_query is held to
(test_gpu_ball_query.py).

* every forward case of test_gpu_ball_query.py with K <= 64 through the grid, with its named expectations;
* clouds chosen against a grid (test_gpu_knn_grid.adversarial's data, regenerated here) at radii where some queries
  have more than K hits and some fewer, so that first-K-in-index-order and the padding are both exercised; a lattice
  whose neighbours lie at exactly the radius on cell faces; coincident targets;
* the grid is really used (the counter of evaluated distances); K > 64; the public wrapper; gradients bitwise those of
  the call without a grid; determinism; HIP graph capture of build + search + backward; a stale grid.
"""
import functools

import pytest
import torch

from tests import ball_query_ref as BR
from tests.test_gpu_ball_query import _ref  # one cached reference per (case, K, radius) for both modules
from torch_renderer_amd import kernels
from torch_renderer_amd.ops import PointGrid, ball_query

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(t):
    return None if t is None else t.to(DEV)


def _rand(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def _search(p1, p2, l1, l2, K, radius, visited=None):
    p1, p2, l1, l2 = _dev(p1), _dev(p2), _dev(l1), _dev(l2)
    grid = kernels.point_grid_build(p2, l2)
    out = kernels.ball_query_grid(p1, p2, grid, l1, l2, K=K, radius=radius, visited=visited)
    torch.cuda.synchronize()
    return out


def _same(got, ref, tag):
    dists, idx = got
    rd, ri = ref
    assert dists.dtype == torch.float32 and idx.dtype == torch.int32 and dists.shape == rd.shape == idx.shape
    assert torch.equal(idx.cpu(), ri), (tag, (idx.cpu() != ri).sum().item())
    assert torch.equal(dists.cpu().view(torch.int32), rd.view(torch.int32)), tag


# --------------------------------------------------------------------------- the existing cases, bitwise
@pytest.mark.parametrize("name,K", [(n, k) for n, (_, ks) in BR.CASES.items() for k in ks if k <= 64])
def test_ball_query_grid_bitwise(name, K):
    radius = BR.CASES[name][0]
    _same(_search(*BR.case(name), K, radius), _ref(name, K, radius), (name, K))
    ri = _ref(name, K, radius)[1]
    if name == "1x3":
        assert (ri[..., :3] == torch.arange(3, dtype=torch.int32)).all() and (ri[..., 3:] == -1).all()
        _same(_search(*BR.case(name), K, 0.0), _ref(name, K, 0.0), (name, K, "radius 0"))
        assert (_ref(name, K, 0.0)[1] == -1).all()
    if name in ("strict", "round0.7", "round0.1"):
        assert ri.tolist() == [[[1, -1]]]
    if name == "wave":
        assert (ri[0, :64] == torch.arange(4, dtype=torch.int32)).all()
        assert (ri[0, 64:, 0] == 1024).all() and (ri[0, 64:, 1:] == -1).all()
    if name == "het":
        assert (ri[3] == -1).all() and (ri[2] == -1).all() and (ri[1, 1:] == -1).all() and (ri[0, :, 0] >= -1).all()
        assert (ri[0] >= 0).any() and (ri[0] == -1).any()


def test_first_k_not_nearest_k():
    radius, K = BR.CASES["first"][0], 8
    p1, p2, _, _ = BR.case("first")
    dists, idx = _search(p1, p2, None, None, K, radius)
    assert torch.equal(idx.cpu()[0], torch.arange(K, dtype=torch.int32).expand(p1.shape[1], K))
    assert not torch.equal(dists, dists.sort(-1).values)  # not sorted by distance either


# --------------------------------------------------------------------------- clouds chosen against a grid
@functools.lru_cache(maxsize=None)
def adversarial(name):
    """(p1, p2) on the CPU (never modified): the data of test_gpu_knn_grid.adversarial."""
    q, t = _rand(1, 200, 3, seed=101), _rand(1, 3000, 3, seed=102)
    if name == "uniform":
        return q, t
    if name == "outside":  # queries up to 2x outside the targets' box
        return (q - 0.5) * 4.0 + 0.5, t
    if name == "offset":
        return q + 1000.0, t + 1000.0
    if name == "planar":
        p = t.clone()
        p[..., 2] = 0.25
        return q, p
    if name == "outlier":
        p = t.clone()
        p[0, 0] = torch.tensor([500.0, -300.0, 40.0])
        return q, p
    if name == "lattice":  # the 12^3 lattice of spacing 1/8 twice over; every 7th lattice point is a query
        r = torch.arange(12, dtype=torch.float32) / 8.0
        lat = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
        return lat[::7][None].contiguous(), torch.cat([lat, lat], 0)[None]
    if name == "coincident":
        return q, torch.tensor([0.3, 1.3, 2.3]).expand(1, 3000, 3).contiguous()
    if name == "gaussian":
        g = torch.Generator().manual_seed(103)
        return torch.randn(1, 200, 3, generator=g), torch.randn(1, 3000, 3, generator=g)
    if name == "1x257x20000":  # 18^3 cells, more than the 1,024 threads of the scan; P1 is no multiple of the wave
        return _rand(1, 257, 3, seed=104), _rand(1, 20000, 3, seed=105)
    raise KeyError(name)


# (case, K, radius, both): both = some query has more than K hits and some query fewer
ADVERSARIAL = (("uniform", 8, 0.125, True), ("offset", 8, 0.125, True), ("outlier", 8, 0.125, True),
               ("outside", 8, 0.25, True), ("planar", 8, 0.125, True), ("gaussian", 8, 1.0, True),
               ("gaussian", 32, 1.0, True), ("1x257x20000", 8, 0.05, True), ("lattice", 16, 0.125, False),
               ("lattice", 16, 0.25, False), ("coincident", 8, 0.25, False), ("coincident", 8, 3.0, False))


@functools.lru_cache(maxsize=None)
def _adv_ref(name, K, radius):
    p1, p2 = adversarial(name)
    return BR.ball_query_ref(p1, p2, None, None, K, radius), BR.hit_counts(p1, p2, None, None, radius)[0]


@pytest.mark.parametrize("name,K,radius,both", ADVERSARIAL)
def test_ball_query_grid_bitwise_adversarial(name, K, radius, both):
    p1, p2 = adversarial(name)
    ref, hits = _adv_ref(name, K, radius)
    print(f"[ball grid] {name} K = {K} radius {radius}: hits per query {hits.min().item()}..{hits.max().item()}, "
          f"{(hits < K).sum().item()} queries below K, {(hits > K).sum().item()} above")
    if both:
        assert (hits > K).any() and (hits < K).any()
    if name == "lattice" and radius == 0.125:  # the point and its duplicate; the neighbours at exactly the radius: no
        assert (hits == 2).all()
    if name == "lattice" and radius == 0.25:
        assert hits.min() >= 16 and hits.max() <= 54
    if name == "coincident":
        assert (hits == (0 if radius == 0.25 else 3000)).all()
    got = _search(p1, p2, None, None, K, radius)
    _same(got, ref, (name, K, radius))
    if name == "coincident" and radius == 3.0:
        assert torch.equal(got[1].cpu()[0], torch.arange(8, dtype=torch.int32).expand(200, 8))


def test_a_nan_coordinate_never_hits_and_a_cloud_that_is_not_finite_is_scanned_whole():
    p1, p2 = (t.clone() for t in adversarial("uniform"))
    p2[0, 5, 1] = float("nan")
    p2[0, 900, 0] = float("inf")
    p1[0, 3, 2] = float("nan")
    K, radius = 8, 0.125
    ref = BR.ball_query_ref(p1, p2, None, None, K, radius)
    assert (ref[1][0, 3] == -1).all() and not (ref[1] == 5).any() and not (ref[1] == 900).any()
    visited = torch.zeros(1, dtype=torch.int64, device=DEV)
    _same(_search(p1, p2, None, None, K, radius, visited), ref, "nan")
    assert visited.item() == 200 * 3000  # one cell


# --------------------------------------------------------------------------- the grid is used; K > 64
def test_the_search_visits_a_fraction_of_the_targets():
    p1, p2 = adversarial("1x257x20000")
    K, radius = 8, 0.05
    visited = torch.zeros(1, dtype=torch.int64, device=DEV)
    _same(_search(p1, p2, None, None, K, radius, visited), _adv_ref("1x257x20000", K, radius)[0], "visited")
    print(f"[ball grid] 257 x 20000, radius {radius}: {visited.item() / 257:.1f} distances per query, "
          f"{visited.item() / (257 * 20000):.5f} of all pairs")
    assert 0 < visited.item() < 257 * 20000 / 10


def test_k_above_64_is_refused_with_a_grid_and_runs_without():
    p1, p2, _, _ = (_dev(t) for t in BR.case("63x65"))
    grid = PointGrid(p2)
    with pytest.raises(NotImplementedError, match="64"):
        ball_query(p1, p2, K=65, radius=1.0, grid=grid)
    with pytest.raises(NotImplementedError, match="64"):
        ball_query(p1, p2, radius=1.0, grid=grid)  # the default K = 500
    with pytest.raises(NotImplementedError, match="64"):
        kernels.ball_query_grid(p1, p2, grid.buffer, K=65, radius=1.0)
    out = ball_query(p1, p2, K=65, radius=1.0)
    assert torch.equal(out.idx.cpu(), BR.ball_query_ref(p1, p2, K=65, radius=1.0)[1].long())
    at64 = ball_query(p1, p2, K=64, radius=1.0, grid=grid)
    assert torch.equal(at64.idx, out.idx[..., :64]) and (out.idx[..., 64] == -1).all()  # at most 64 hits here


# --------------------------------------------------------------------------- the public wrapper
def test_public_wrapper_equals_the_call_without_a_grid():
    radius, (K,) = BR.CASES["het"]
    p1, p2, l1, l2 = (_dev(t) for t in BR.case("het"))
    rd, ri = _ref("het", K, radius)
    grid = PointGrid(p2, l2)
    a = ball_query(p1, p2, l1, l2, K=K, radius=radius, grid=grid)
    b = ball_query(p1, p2, l1, l2, K=K, radius=radius)
    assert a.idx.dtype == torch.int64 and a.dists.dtype == torch.float32 and a.knn.shape == (4, 257, K, 3)
    assert (a.idx == -1).any() and torch.equal(a.idx.cpu(), ri.long())
    for u, w in zip(a, b):
        assert torch.equal(u, w)
    assert (a.knn[a.idx < 0] == 0).all()
    assert ball_query(p1, p2, l1, l2, K=K, radius=radius, return_nn=False, grid=grid).knn is None
    # float64 queries against the float32 targets the grid was built from: read as float32, returned as float64
    o64 = ball_query(p1.double(), p2, l1, l2, K=K, radius=radius, grid=grid)
    assert o64.dists.dtype == torch.float64 and torch.equal(o64.idx, a.idx) and torch.equal(o64.dists, a.dists.double())
    with pytest.raises(ValueError, match="ball_query: the grid was not built from this p2"):
        ball_query(p1, p2.clone(), l1, l2, K=K, radius=radius, grid=grid)
    with pytest.raises(ValueError, match="lengths2"):
        ball_query(p1, p2, l1, None, K=K, radius=radius, grid=grid)


# --------------------------------------------------------------------------- gradients
def _upstream(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("name", ["het", "257x1000"])
def test_gradients_are_those_of_the_call_without_a_grid(name):
    radius, (K,) = BR.CASES[name]
    p1, p2, l1, l2 = BR.case(name)
    g = _dev(_upstream((p1.shape[0], p1.shape[1], K), seed=31))
    a, b = _dev(p1).requires_grad_(True), _dev(p2).requires_grad_(True)
    l1, l2 = _dev(l1), _dev(l2)
    plain = ball_query(a, b, l1, l2, K=K, radius=radius)
    ga, gb = torch.autograd.grad((plain.dists * g).sum() + plain.knn.sum(), (a, b))
    through = ball_query(a, b, l1, l2, K=K, radius=radius, grid=PointGrid(b, l2))
    assert through.dists.requires_grad and not through.idx.requires_grad
    ha, hb = torch.autograd.grad((through.dists * g).sum() + through.knn.sum(), (a, b))
    assert torch.equal(through.idx, plain.idx) and torch.equal(through.idx.cpu(), _ref(name, K, radius)[1].long())
    assert torch.equal(ga.view(torch.int32), ha.view(torch.int32)) and torch.equal(gb.view(torch.int32), hb.view(torch.int32))
    assert ga.abs().sum() > 0 and gb.abs().sum() > 0


# --------------------------------------------------------------------------- determinism, graph capture
def _step(p1, p2, g, K=8, radius=0.6):
    a, b = p1.detach().requires_grad_(True), p2.detach().requires_grad_(True)
    out = ball_query(a, b, K=K, radius=radius, grid=PointGrid(b))
    ga, gb = torch.autograd.grad((out.dists * g).sum() + out.knn.sum(), (a, b))
    return out.dists.detach(), out.idx, out.knn.detach(), ga, gb


def test_two_runs_are_bitwise_equal():
    p1, p2, _, _ = BR.case("graph")
    p1, p2, g = _dev(p1), _dev(p2), _dev(_upstream((2, 300, 8), seed=51))
    for u, w in zip(_step(p1, p2, g), _step(p1, p2, g)):
        assert torch.equal(u, w)


def test_hip_graph_capture_replays_with_changed_inputs():
    p1, p2, _, _ = BR.case("graph")
    g = _dev(_upstream((2, 300, 8), seed=52))
    a, b = _dev(p1).clone(), _dev(p2).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _step(a, b, g)  # warm-up on the side stream: workspace sizes cached, allocator primed
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _step(a, b, g)
    for seed in (61, 62):  # replay twice, each time with other clouds in the captured tensors
        a.copy_(_dev(_upstream((2, 300, 3), seed=seed)))
        b.copy_(_dev(_upstream((2, 700, 3), seed=seed + 10)))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in captured]
        rd, ri = BR.ball_query_ref(a.cpu(), b.cpu(), K=8, radius=0.6)
        assert torch.equal(got[1].cpu(), ri.long()) and torch.equal(got[0].cpu().view(torch.int32), rd.view(torch.int32))
        for u, w in zip(_step(a, b, g), got):
            assert torch.equal(u, w)


# --------------------------------------------------------------------------- a stale grid
def test_a_stale_grid_gives_indices_in_range():
    """The grid of one cloud searched with another of the same shape: every address the search forms is clamped into
    the buffers it was given, so the neighbours are wrong and in range."""
    K, P2 = 8, 3000
    old = _dev(_rand(2, P2, 3, seed=107) * 3.0 - 1.0)
    new = _dev(_rand(2, P2, 3, seed=108))
    l2 = torch.tensor([P2, 1700], device=DEV)
    grid = kernels.point_grid_build(old)  # other points, other lengths
    dists, idx = kernels.ball_query_grid(_dev(_rand(2, 200, 3, seed=109)), new, grid, None, l2, K=K, radius=0.3)
    torch.cuda.synchronize()
    assert ((idx >= -1) & (idx < P2)).all() and torch.isfinite(dists).all()
