"""PointGrid / knn_points(grid=) on the MI355X (csrc/mr_grid.hip): every index and distance bitwise the float32
restatement of tests/knn_ref.py, which is what the brute-force knn_points is held to (test_gpu_knn.py).

* every forward case of test_gpu_knn.py through the grid, and clouds chosen against a grid: queries outside the box, a
  large offset, a planar cloud, a far outlier, a lattice lying on the cell faces, coincident points, a cloud with more
  cells than a scan workgroup has threads;
* the grid is really used (the counter of evaluated distances), and its structure (mr_point_grid_describe);
* gradients bitwise those of the call without a grid; determinism; HIP graph capture of build + search + backward;
* a stale grid gives indices in range.
"""
import functools

import pytest
import torch

from tests import knn_ref as KR
from tests.test_gpu_knn import _ref  # one cached reference per (case, K, norm) for both modules
from torch_renderer_amd import kernels
from torch_renderer_amd.ops import PointGrid, knn_points

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(t):
    return None if t is None else t.to(DEV)


def _rand(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def adversarial(name):
    """(p1, p2, K) on the CPU (never modified)."""
    q, t = _rand(1, 200, 3, seed=101), _rand(1, 3000, 3, seed=102)
    if name == "uniform":
        return q, t, 8
    if name == "outside":  # queries up to 2x outside the targets' box
        return (q - 0.5) * 4.0 + 0.5, t, 8
    if name == "offset":
        return q + 1000.0, t + 1000.0, 8
    if name == "planar":
        p = t.clone()
        p[..., 2] = 0.25
        return q, p, 8
    if name == "outlier":
        p = t.clone()
        p[0, 0] = torch.tensor([500.0, -300.0, 40.0])
        return q, p, 8
    if name == "lattice":  # the 12^3 lattice of spacing 1/8 twice over; every 7th lattice point is a query
        r = torch.arange(12, dtype=torch.float32) / 8.0
        lat = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
        return lat[::7][None].contiguous(), torch.cat([lat, lat], 0)[None], 16
    if name == "coincident":
        return q, torch.tensor([0.3, 1.3, 2.3]).expand(1, 3000, 3).contiguous(), 8
    if name == "gaussian":
        g = torch.Generator().manual_seed(103)
        return torch.randn(1, 200, 3, generator=g), torch.randn(1, 3000, 3, generator=g), 32
    if name == "1x257x20000":  # 18^3 cells, more than the 1,024 threads of the scan; P1 is no multiple of the wave
        return _rand(1, 257, 3, seed=104), _rand(1, 20000, 3, seed=105), 8
    raise KeyError(name)


ADVERSARIAL = ("uniform", "outside", "offset", "planar", "outlier", "lattice", "coincident", "gaussian", "1x257x20000")


@functools.lru_cache(maxsize=None)
def _adv_ref(name, norm):
    p1, p2, K = adversarial(name)
    return KR.knn_ref(p1, p2, None, None, K, norm)


def _search(p1, p2, l1, l2, K, norm, visited=None):
    p1, p2, l1, l2 = _dev(p1), _dev(p2), _dev(l1), _dev(l2)
    grid = kernels.point_grid_build(p2, l2)
    out = kernels.knn_points_grid(p1, p2, grid, l1, l2, K=K, norm=norm, visited=visited)
    torch.cuda.synchronize()
    return out + (grid,)


def _assert_bitwise(tag, dists, idx, rd, ri):
    assert dists.dtype == torch.float32 and idx.dtype == torch.int32 and dists.shape == rd.shape == idx.shape
    assert torch.equal(idx.cpu(), ri), (tag, (idx.cpu() != ri).any(-1).sum().item())
    assert torch.equal(dists.cpu().view(torch.int32), rd.view(torch.int32)), tag


# --------------------------------------------------------------------------- forward, bitwise
@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("name,K", [(n, k) for n, ks in KR.CASES.items() for k in ks])
def test_grid_knn_bitwise(name, K, norm):
    dists, idx, _ = _search(*KR.case(name), K, norm)
    _assert_bitwise((name, K, norm), dists, idx, *_ref(name, K, norm))


@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("name", ADVERSARIAL)
def test_grid_knn_bitwise_adversarial(name, norm):
    p1, p2, K = adversarial(name)
    dists, idx, _ = _search(p1, p2, None, None, K, norm)
    _assert_bitwise((name, K, norm), dists, idx, *_adv_ref(name, norm))


@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("name", ["63x65", "het"])
def test_k1_is_nearest_points(name, norm):
    p1, p2, l1, l2 = KR.case(name)
    dists, idx, _ = _search(p1, p2, l1, l2, 1, norm)
    dx, ix, _, _ = kernels.nearest_points(_dev(p1), _dev(p2), _dev(l1), _dev(l2), norm=norm)
    assert torch.equal(idx[..., 0], ix) and torch.equal(dists[..., 0].view(torch.int32), dx.view(torch.int32))


def test_public_call_equals_the_call_without_a_grid():
    p1, p2, l1, l2 = (_dev(t) for t in KR.case("het"))
    K = 8
    grid = PointGrid(p2, l2)
    a = knn_points(p1, p2, l1, l2, K=K, return_nn=True, grid=grid)
    b = knn_points(p1, p2, l1, l2, K=K, return_nn=True)
    assert a.idx.dtype == torch.int64 and (a.idx >= 0).all()
    for u, w in zip(a, b):
        assert torch.equal(u, w)
    c = knn_points(p1, p2, l1, l2, K=K, norm=1, return_sorted=False, version=3, grid=grid)
    d = knn_points(p1, p2, l1, l2, K=K, norm=1)
    assert c.knn is None and torch.equal(c.idx, d.idx) and torch.equal(c.dists, d.dists)
    with pytest.raises(ValueError):
        knn_points(p1, p2.clone(), l1, l2, K=K, grid=grid)
    # a Pointclouds brings its lengths
    from torch_renderer_amd.ops import Pointclouds
    pc = Pointclouds([p2[n, :int(l)] for n, l in enumerate(KR.case("het")[3]) if int(l) > 0])
    pg = PointGrid(pc)
    keep = [n for n, l in enumerate(KR.case("het")[3]) if int(l) > 0]
    e = knn_points(p1[keep], pc.points_padded(), l1[keep], pc.num_points_per_cloud(), K=K, grid=pg)
    assert torch.equal(e.idx, b.idx[keep]) and torch.equal(e.dists, b.dists[keep])


# --------------------------------------------------------------------------- the grid is used, and its structure
@pytest.mark.parametrize("norm", [2, 1])
def test_the_search_visits_a_fraction_of_the_targets(norm):
    p1, p2, K = adversarial("uniform")
    visited = torch.zeros(1, dtype=torch.int64, device=DEV)
    dists, idx, _ = _search(p1, p2, None, None, K, norm, visited)
    _assert_bitwise(("uniform", K, norm), dists, idx, *_adv_ref("uniform", norm))
    share = visited.item() / (200 * 3000)
    print(f"[knn grid] uniform 200 x 3000, K = {K}, norm {norm}: {share:.4f} of all pairs evaluated")
    assert 0 < share <= 0.25, share
    # the counter adds up over calls, and a cloud of one cell visits every pair
    p1, p2, K = adversarial("coincident")
    visited.zero_()
    _search(p1, p2, None, None, K, norm, visited)
    assert visited.item() == 200 * 3000


def test_grid_structure():
    for name in ADVERSARIAL:
        _, p2, _ = adversarial(name)
        P = p2.shape[1]
        dims, cell, most = kernels.point_grid_describe(kernels.point_grid_build(_dev(p2)), 1, P)
        print(f"[knn grid] {name}: dims {dims[0].tolist()}, h {cell[0, 3].item():.6g}, largest cell {most[0].item()}")
        assert (dims >= 1).all() and int(dims[0].prod()) <= P and cell[0, 3] > 0 and 1 <= most[0] <= P
        assert torch.equal(cell[0, :3], p2[0].min(0).values)
        if name == "coincident":
            assert dims[0].tolist() == [1, 1, 1] and most[0] == P
        if name == "planar":
            assert dims[0, 2] == 1 and dims[0, 0] > 1 and dims[0, 1] > 1
        if name == "1x257x20000":
            assert int(dims[0].prod()) > 1024
    # het: lengths 500, 1000, 0, 3 of 1000; the empty cloud is one cell
    _, p2, _, l2 = KR.case("het")
    grid = PointGrid(_dev(p2), _dev(l2))
    dims, cell, most = grid.describe()
    assert dims.shape == (4, 3) and cell.shape == (4, 4) and most.shape == (4,)
    assert (dims >= 1).all() and (cell[:, 3] > 0).all() and torch.isfinite(cell).all()
    for n, L in enumerate(l2.tolist()):
        assert int(dims[n].prod()) <= max(L, 1) and 0 <= most[n] <= L and (L == 0 or most[n] >= 1), (n, L)
    assert dims[2].tolist() == [1, 1, 1] and most[2] == 0


def test_a_cloud_that_is_not_finite_is_one_cell():
    p2 = _rand(2, 500, 3, seed=106)
    p2[0, 17, 1] = float("inf")
    dims, cell, most = kernels.point_grid_describe(kernels.point_grid_build(_dev(p2)), 2, 500)
    assert dims[0].tolist() == [1, 1, 1] and most[0] == 500 and int(dims[1].prod()) > 1
    assert torch.isfinite(cell).all() and (cell[:, 3] > 0).all()


# --------------------------------------------------------------------------- gradients
def _upstream(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("norm", [2, 1])
def test_gradients_are_those_of_the_call_without_a_grid(norm):
    p1, p2, _, _ = KR.case("63x65")
    K = 8
    g = _dev(_upstream((1, 63, K), seed=31))
    a, b = _dev(p1).requires_grad_(True), _dev(p2).requires_grad_(True)
    plain = knn_points(a, b, K=K, norm=norm)
    ga, gb = torch.autograd.grad((plain.dists * g).sum(), (a, b))
    with_grid = knn_points(a, b, K=K, norm=norm, grid=PointGrid(b))
    assert with_grid.dists.requires_grad and not with_grid.idx.requires_grad
    ha, hb = torch.autograd.grad((with_grid.dists * g).sum(), (a, b))
    assert torch.equal(with_grid.idx, plain.idx) and torch.equal(with_grid.dists, plain.dists)
    assert torch.equal(with_grid.idx.cpu(), _ref("63x65", K, norm)[1].long())
    assert torch.equal(ga, ha) and torch.equal(gb, hb) and ga.abs().sum() > 0 and gb.abs().sum() > 0
    sa, sb = torch.autograd.grad(knn_points(a, b, K=K, norm=norm, grid=PointGrid(b)).dists.sum(), (a, b))
    ta, tb = torch.autograd.grad(knn_points(a, b, K=K, norm=norm).dists.sum(), (a, b))
    assert torch.equal(sa, ta) and torch.equal(sb, tb)


# --------------------------------------------------------------------------- determinism, graph capture
def _step(p1, p2, g, K=16):
    a, b = p1.detach().requires_grad_(True), p2.detach().requires_grad_(True)
    out = knn_points(a, b, K=K, grid=PointGrid(b))
    ga, gb = torch.autograd.grad(out.dists, (a, b), g)
    return out.dists.detach(), out.idx, ga, gb


def test_two_runs_are_bitwise_equal():
    p1, p2, _, _ = KR.case("1x1000x1000")
    p1, p2, g = _dev(p1), _dev(p2), _dev(_upstream((1, 1000, 16), seed=51))
    for u, w in zip(_step(p1, p2, g), _step(p1, p2, g)):
        assert torch.equal(u, w)


def test_hip_graph_capture_replays_with_changed_inputs():
    K = 8
    g = _dev(_upstream((2, 300, K), seed=53))
    a, b = _dev(_upstream((2, 300, 3), seed=60)), _dev(_upstream((2, 700, 3), seed=70))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _step(a, b, g, K)  # warm-up on the side stream: workspace sizes cached, allocator primed
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _step(a, b, g, K)
    for seed in (61, 62):  # replay twice, each time with other clouds in the captured tensors
        a.copy_(_dev(_upstream((2, 300, 3), seed=seed)))
        b.copy_(_dev(_upstream((2, 700, 3), seed=seed + 10)))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in captured]
        eager = _step(a, b, g, K)
        rd, ri = KR.knn_ref(a.cpu(), b.cpu(), K=K)
        assert torch.equal(got[1].cpu(), ri.long()) and torch.equal(got[0].cpu().view(torch.int32), rd.view(torch.int32))
        for u, w in zip(eager, got):
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
    dists, idx = kernels.knn_points_grid(_dev(_rand(2, 200, 3, seed=109)), new, grid, None, l2, K=K)
    torch.cuda.synchronize()
    assert ((idx >= -1) & (idx < P2)).all() and torch.isfinite(dists).all()
