"""ball_query / masked_gather on the MI355X (csrc/mr_ballquery.hip) against the CPU restatement of
tests/ball_query_ref.py.

* forward: idx and the bit patterns of dists equal the float32 restatement (the first K hits in index order), over
  the launch regimes test_ball_query_cpu.py proves the named shapes reach: strictness, first-K against nearest-K, a
  wave that fills before its neighbour, chunk and tile boundaries, a heterogeneous batch, and the split path against
  both the restatement and the unsplit launch of the same clouds;
* the public wrapper's padding, dtypes and masked_gather;
* gradients: every entry within 1e-4 * max|ref64| of the float64 restatement evaluated with the float32 neighbours
  (the bar of test_gpu_knn.py); the float32 restatement's own error is printed beside it;
* determinism, HIP graph capture, and sample_farthest_points -> ball_query -> masked_gather end to end.
"""
import functools

import pytest
import torch

from tests import ball_query_ref as BR
from torch_renderer_amd import kernels
from torch_renderer_amd.ops import ball_query, knn_points, masked_gather, sample_farthest_points

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(t):
    return None if t is None else t.to(DEV)


@functools.lru_cache(maxsize=None)
def _ref(name, K, radius):
    p1, p2, l1, l2 = BR.case(name)
    return BR.ball_query_ref(p1, p2, l1, l2, K, radius)


def _run(name, K, radius):
    p1, p2, l1, l2 = BR.case(name)
    out = kernels.ball_query(_dev(p1), _dev(p2), _dev(l1), _dev(l2), K=K, radius=radius)
    torch.cuda.synchronize()
    return out


def _same(got, ref, tag):
    dists, idx = got
    rd, ri = ref
    assert dists.dtype == torch.float32 and idx.dtype == torch.int32 and dists.shape == rd.shape == idx.shape
    assert torch.equal(idx.cpu(), ri), (tag, (idx.cpu() != ri).sum().item())
    assert torch.equal(dists.cpu().view(torch.int32), rd.view(torch.int32)), tag


# --------------------------------------------------------------------------- forward, bitwise
@pytest.mark.parametrize("name,K", [(n, k) for n, (_, ks) in BR.CASES.items() for k in ks])
def test_ball_query_bitwise(name, K):
    radius = BR.CASES[name][0]
    _same(_run(name, K, radius), _ref(name, K, radius), (name, K))
    ri = _ref(name, K, radius)[1]
    if name == "1x3":
        assert (ri[..., :3] == torch.arange(3, dtype=torch.int32)).all() and (ri[..., 3:] == -1).all()
        _same(_run(name, K, 0.0), _ref(name, K, 0.0), (name, K, "radius 0"))
        assert (_ref(name, K, 0.0)[1] == -1).all()
    if name in ("strict", "round0.7", "round0.1"):
        assert ri.tolist() == [[[1, -1]]]
    if name == "wave":
        assert (ri[0, :64] == torch.arange(4, dtype=torch.int32)).all()
        assert (ri[0, 64:, 0] == 1024).all() and (ri[0, 64:, 1:] == -1).all()
    if name == "het":
        assert (ri[3] == -1).all() and (ri[2] == -1).all() and (ri[1, 1:] == -1).all() and (ri[0, :, 0] >= -1).all()
        assert (ri[0] >= 0).any() and (ri[0] == -1).any()


@pytest.mark.parametrize("K", [500, 8])
def test_first_k_not_nearest_k(K):
    radius = BR.CASES["first"][0]
    p1, p2, _, _ = BR.case("first")
    dists, idx = _run("first", K, radius)
    assert torch.equal(idx.cpu()[0], torch.arange(K, dtype=torch.int32).expand(p1.shape[1], K))
    if K == 8:
        near = knn_points(_dev(p1), _dev(p2), K=8).idx
        assert not torch.equal(near, idx.long())
        assert not torch.equal(dists, dists.sort(-1).values)  # not sorted by distance either


def test_split_path_is_bitwise_the_unsplit_launch():
    radius, (K,) = BR.CASES["100x20000"]
    p1, p2, _, _ = BR.case("100x20000")
    assert kernels.ball_query_geometry(1, 100, 20000, K)[1] > 1 and kernels.ball_query_geometry(300, 100, 20000, K)[1] == 1
    split = _run("100x20000", K, radius)
    _same(split, _ref("100x20000", K, radius), "split")
    many = kernels.ball_query(_dev(p1).expand(300, -1, -1), _dev(p2).expand(300, -1, -1), K=K, radius=radius)
    for got, one in zip(many, split):
        assert torch.equal(got.view(torch.int32), one.view(torch.int32).expand(300, -1, -1))


# --------------------------------------------------------------------------- the public wrapper
def test_public_wrapper_padding_dtypes_and_masked_gather():
    radius, (K,) = BR.CASES["het"]
    p1, p2, l1, l2 = BR.case("het")
    rd, ri = _ref("het", K, radius)
    out = ball_query(_dev(p1), _dev(p2), _dev(l1), _dev(l2), K=K, radius=radius)
    assert out.idx.dtype == torch.int64 and out.dists.dtype == torch.float32 and out.knn.shape == (4, 257, K, 3)
    assert torch.equal(out.idx.cpu(), ri.long()) and (out.idx == -1).any()
    assert torch.equal(out.dists.cpu().view(torch.int32), rd.view(torch.int32))
    want = torch.zeros(4, 257, K, 3)
    for n in range(4):
        has = ri[n] >= 0
        want[n][has] = p2[n][ri[n][has].long()]
    assert torch.equal(out.knn.cpu(), want) and (out.knn[out.idx < 0] == 0).all()
    assert ball_query(_dev(p1), _dev(p2), _dev(l1), _dev(l2), K=K, radius=radius, return_nn=False).knn is None
    # float64 inputs: read as float32, returned as float64
    o64 = ball_query(_dev(p1).double(), _dev(p2).double(), _dev(l1), _dev(l2), K=K, radius=radius)
    assert o64.dists.dtype == torch.float64 and o64.knn.dtype == torch.float64
    assert torch.equal(o64.idx, out.idx) and torch.equal(o64.dists, out.dists.double())
    # any feature tensor, not only points
    feat = torch.arange(4 * 1000 * 2, dtype=torch.float32, device=DEV).reshape(4, 1000, 2)
    got = masked_gather(feat, out.idx)
    assert got.shape == (4, 257, K, 2) and (got[out.idx < 0] == 0).all()
    has = out.idx >= 0
    n_i = has.nonzero()[:, 0]
    assert torch.equal(got[has], feat[n_i, out.idx[has]])
    # the defaults: K = 500, radius 0.2, return_nn
    d = ball_query(_dev(p1), _dev(p2))
    assert d.idx.shape == (4, 257, 500) and d.knn.shape == (4, 257, 500, 3)
    assert torch.equal(d.idx.cpu(), BR.ball_query_ref(p1, p2, K=500, radius=0.2)[1].long())


# --------------------------------------------------------------------------- gradients
def _upstream(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _grads(p1, p2, l1, l2, K, radius, g):
    a, b = _dev(p1).requires_grad_(True), _dev(p2).requires_grad_(True)
    dists, idx = kernels.BallQuery.apply(a, b, _dev(l1), _dev(l2), K, radius)
    assert not idx.requires_grad and dists.requires_grad
    ga, gb = torch.autograd.grad(dists, (a, b), _dev(g))
    torch.cuda.synchronize()
    return idx, ga, gb


def _check_grads(tag, got, ref64, ref32):
    for nm, gt, r, r32 in zip(("grad_p1", "grad_p2"), got, ref64, ref32):
        bar = 1e-4 * r.abs().max().item()
        e = (gt.cpu().double() - r).abs().max().item()
        e32 = (r32.double() - r).abs().max().item()
        print(f"[ball] {tag} {nm}: max|err| {e:.3e}, bar {bar:.3e}, float32 restatement's own error {e32:.3e}")
        assert torch.isfinite(gt).all() and e <= bar, (tag, nm, e, bar)


@pytest.mark.parametrize("name", ["het", "257x1000"])
def test_ball_query_gradients(name):
    radius, (K,) = BR.CASES[name]
    p1, p2, l1, l2 = BR.case(name)
    g = _upstream((p1.shape[0], p1.shape[1], K), seed=31)
    idx, ga, gb = _grads(p1, p2, l1, l2, K, radius, g)
    assert torch.equal(idx.cpu(), _ref(name, K, radius)[1])
    ref64 = BR.grad_ref(p1, p2, idx, g, torch.float64)
    ref32 = BR.grad_ref(p1, p2, idx, g, torch.float32)
    _check_grads(f"{name} K={K}", (ga, gb), ref64, ref32)
    # a target nothing reached has the gradient +0 (not -0)
    reached = torch.zeros(p2.shape[:2], dtype=torch.bool)
    for n in range(p2.shape[0]):
        reached[n, idx[n].cpu()[idx[n].cpu() >= 0].long()] = True
    assert (~reached).any()
    assert (gb.cpu()[~reached].view(torch.int32) == 0).all()
    # two runs are bitwise equal
    idx2, ga2, gb2 = _grads(p1, p2, l1, l2, K, radius, g)
    assert torch.equal(idx2, idx) and torch.equal(ga2.view(torch.int32), ga.view(torch.int32))
    assert torch.equal(gb2.view(torch.int32), gb.view(torch.int32))
    if name == "het":  # nan in the free slots of g: not read
        gn = torch.where(idx.cpu() < 0, torch.full_like(g, float("nan")), g)
        assert torch.isnan(gn).any()
        _, na, nb = _grads(p1, p2, l1, l2, K, radius, gn)
        assert torch.equal(na, ga) and torch.equal(nb, gb)
        assert (ga[3] == 0).all() and (ga[1, 1:] == 0).all() and (gb[2] == 0).all() and (gb[3, 500:] == 0).all()


def test_return_nn_gradient_adds_to_the_dists_path():
    radius, (K,) = BR.CASES["het"]
    p1, p2, l1, l2 = BR.case("het")
    gd, gk = _upstream((4, 257, K), seed=41), _upstream((4, 257, K, 3), seed=42)
    a, b = _dev(p1).requires_grad_(True), _dev(p2).requires_grad_(True)
    out = ball_query(a, b, _dev(l1), _dev(l2), K=K, radius=radius)
    ga, gb = torch.autograd.grad((out.dists * _dev(gd)).sum() + (out.knn * _dev(gk)).sum(), (a, b))
    idx = _ref("het", K, radius)[1]
    refs = []
    for dt in (torch.float64, torch.float32):
        ra, rb = p1.to(dt).requires_grad_(True), p2.to(dt).requires_grad_(True)
        d = BR.dists_from_idx(ra, rb, idx)
        nn = masked_gather(rb, idx.long())
        refs.append(torch.autograd.grad((d * gd.to(dt)).sum() + (nn * gk.to(dt)).sum(), (ra, rb)))
    _check_grads("het return_nn", (ga, gb), refs[0], refs[1])


# --------------------------------------------------------------------------- graph capture, end to end
def _step(p1, p2, g, K=8, radius=0.6):
    a, b = p1.detach().requires_grad_(True), p2.detach().requires_grad_(True)
    out = ball_query(a, b, K=K, radius=radius)
    ga, gb = torch.autograd.grad((out.dists * g).sum() + out.knn.sum(), (a, b))
    return out.dists.detach(), out.idx, out.knn.detach(), ga, gb


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
        eager = _step(a, b, g)
        rd, ri = BR.ball_query_ref(a.cpu(), b.cpu(), K=8, radius=0.6)
        assert torch.equal(got[1].cpu(), ri.long()) and torch.equal(got[0].cpu().view(torch.int32), rd.view(torch.int32))
        for u, w in zip(eager, got):
            assert torch.equal(u, w)


def test_farthest_points_then_ball_query_then_gather():
    cloud = _upstream((2, 1000, 3), seed=71)
    radius, K = 0.5, 16
    cent, cidx = sample_farthest_points(_dev(cloud), K=32)
    out = ball_query(cent, _dev(cloud), K=K, radius=radius)
    feat = _dev(_upstream((2, 1000, 5), seed=72))
    grouped = masked_gather(feat, out.idx)
    torch.cuda.synchronize()
    assert torch.equal(cent.cpu(), cloud.gather(1, cidx.cpu()[..., None].expand(-1, -1, 3)))
    rd, ri = BR.ball_query_ref(cent.cpu(), cloud, K=K, radius=radius)
    assert torch.equal(out.idx.cpu(), ri.long()) and torch.equal(out.dists.cpu().view(torch.int32), rd.view(torch.int32))
    # every centroid is a point of the cloud: it finds itself (d = 0 < r2) unless K earlier points are in reach
    me = (out.idx == cidx[..., None]).any(-1) | (out.idx[..., -1] >= 0) & (out.idx[..., -1] < cidx)
    assert me.all()
    want = torch.zeros(2, 32, K, 5)
    has = ri >= 0
    for n in range(2):
        want[n][has[n]] = feat[n].cpu()[ri[n][has[n]].long()]
    assert grouped.shape == (2, 32, K, 5) and torch.equal(grouped.cpu(), want)
    assert torch.equal(out.knn.cpu(), masked_gather(cloud, ri.long()))
