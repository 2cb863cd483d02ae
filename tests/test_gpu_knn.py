"""knn_points / knn_gather on the MI355X (csrc/mr_knn.hip) against the CPU restatement of tests/knn_ref.py.

* forward: dists and idx bitwise the float32 restatement (a stable sort: the lowest index first among equal
  distances), both norms, over the launch regimes test_knn_cpu.py proves the named shapes exercise; at K = 1 bitwise
  kernels.nearest_points; the public padding, return_nn and return_sorted;
* gradients: every entry within 1e-4 * max|ref64| of the float64 restatement evaluated with the float32 neighbours
  (the bar of test_gpu_points.py for chamfer gradients); the float32 restatement's own error is printed beside it;
* determinism and HIP graph capture.
"""
import functools

import pytest
import torch

from tests import knn_ref as KR
from torch_renderer_amd import kernels
from torch_renderer_amd.ops import knn_gather, knn_points

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(t):
    return None if t is None else t.to(DEV)


@functools.lru_cache(maxsize=None)
def _ref(name, K, norm):
    p1, p2, l1, l2 = KR.case(name)
    return KR.knn_ref(p1, p2, l1, l2, K, norm)


def _run(name, K, norm):
    p1, p2, l1, l2 = KR.case(name)
    out = kernels.knn_points(_dev(p1), _dev(p2), _dev(l1), _dev(l2), K=K, norm=norm)
    torch.cuda.synchronize()
    return out


# --------------------------------------------------------------------------- forward, bitwise
@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("name,K", [(n, k) for n, ks in KR.CASES.items() for k in ks])
def test_knn_bitwise(name, K, norm):
    dists, idx = _run(name, K, norm)
    rd, ri = _ref(name, K, norm)
    assert dists.dtype == torch.float32 and idx.dtype == torch.int32 and dists.shape == rd.shape == idx.shape
    assert torch.equal(idx.cpu(), ri), (name, K, norm, (idx.cpu() != ri).sum().item())
    assert torch.equal(dists.cpu().view(torch.int32), rd.view(torch.int32)), (name, K, norm)
    if name == "dup":
        assert torch.equal(ri[0], torch.arange(K, dtype=torch.int32).expand(ri.shape[1], K))
    if name == "1x3":
        assert (ri[..., 3:] == -1).all() and (ri[..., :3] >= 0).all() and (rd[..., 3:] == 0).all()
    if name == "het":
        assert (ri[3] == -1).all() and (ri[2] == -1).all() and (ri[1, 1:] == -1).all() and (ri[1, 0] >= 0).all()
        assert (ri[0, :, :] >= 0).all()


@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("name", ["63x65", "het", "8x100x20000"])
def test_k1_is_nearest_points(name, norm):
    p1, p2, l1, l2 = KR.case(name)
    dists, idx = _run(name, 1, norm)
    dx, ix, _, _ = kernels.nearest_points(_dev(p1), _dev(p2), _dev(l1), _dev(l2), norm=norm)
    assert torch.equal(idx[..., 0], ix) and torch.equal(dists[..., 0].view(torch.int32), dx.view(torch.int32))


def test_public_padding_and_return_nn():
    p1, p2, l1, l2 = KR.case("het")
    K = 8
    dists, idx = _run("het", K, 2)
    out = knn_points(_dev(p1), _dev(p2), _dev(l1), _dev(l2), K=K, return_nn=True, version=3)
    assert out.idx.dtype == torch.int64 and out.dists.dtype == torch.float32 and out.knn.shape == (4, 257, K, 3)
    pad = idx < 0
    assert pad.any() and (out.idx[pad] == 0).all() and (out.dists[pad] == 0).all()
    assert torch.equal(out.idx[~pad], idx[~pad].long()) and torch.equal(out.dists, dists)
    # knn: p2 gathered at idx, zero rows in the slots past lengths2
    want = torch.zeros(4, 257, K, 3)
    for n in range(4):
        k = min(K, int(l2[n]))
        want[n, :, :k] = p2[n][out.idx[n, :, :k].cpu()]
    assert torch.equal(out.knn.cpu(), want)
    assert (out.knn[3, :, 3:] == 0).all() and (out.knn[2] == 0).all()
    assert torch.equal(knn_gather(_dev(p2), out.idx, _dev(l2)), out.knn)
    assert knn_points(_dev(p1), _dev(p2), K=2).knn is None
    # any feature tensor, not only points
    feat = torch.arange(4 * 1000 * 2, dtype=torch.float32, device=DEV).reshape(4, 1000, 2)
    got = knn_gather(feat, out.idx, _dev(l2))
    assert got.shape == (4, 257, K, 2) and torch.equal(got[0, 5, 2], feat[0, out.idx[0, 5, 2]])


def test_return_sorted_false_is_the_same_set():
    p1, p2, l1, l2 = KR.case("het")
    a = knn_points(_dev(p1), _dev(p2), _dev(l1), _dev(l2), K=8)
    b = knn_points(_dev(p1), _dev(p2), _dev(l1), _dev(l2), K=8, return_sorted=False)
    assert torch.equal(a.idx.sort(-1).values, b.idx.sort(-1).values)
    assert torch.equal(a.dists.sort(-1).values, b.dists.sort(-1).values)


# --------------------------------------------------------------------------- gradients
def _upstream(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _grads(p1, p2, l1, l2, K, norm, g):
    a, b = _dev(p1).requires_grad_(True), _dev(p2).requires_grad_(True)
    dists, idx = kernels.KnnPoints.apply(a, b, _dev(l1), _dev(l2), K, norm)
    assert not idx.requires_grad
    ga, gb = torch.autograd.grad(dists, (a, b), _dev(g))
    torch.cuda.synchronize()
    return idx, ga, gb


def _check_grads(tag, got, ref64, ref32):
    for nm, gt, r, r32 in zip(("grad_p1", "grad_p2"), got, ref64, ref32):
        bar = 1e-4 * r.abs().max().item()
        e = (gt.cpu().double() - r).abs().max().item()
        e32 = (r32.double() - r).abs().max().item()
        print(f"[knn] {tag} {nm}: max|err| {e:.3e}, bar {bar:.3e}, float32 restatement's own error {e32:.3e}")
        assert torch.isfinite(gt).all() and e <= bar, (tag, nm, e, bar)


@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("name,K", [("63x65", 8), ("het", 8), ("ties", 12), ("1000x4", 4)])
def test_knn_gradients(name, K, norm):
    p1, p2, l1, l2 = KR.case(name)
    g = _upstream((p1.shape[0], p1.shape[1], K), seed=31)
    idx, ga, gb = _grads(p1, p2, l1, l2, K, norm, g)
    if name == "1000x4":  # every target is a neighbour of every query: 1,000 addends per row of grad_p2
        assert torch.equal(idx.cpu().sort(-1).values, torch.arange(4, dtype=torch.int32).expand(1, 1000, 4))
    else:
        assert torch.equal(idx.cpu(), _ref(name, K, norm)[1])
    ref64 = KR.knn_grad_ref(p1, p2, idx, g, norm, torch.float64)
    ref32 = KR.knn_grad_ref(p1, p2, idx, g, norm, torch.float32)
    _check_grads(f"{name} K={K} norm={norm}", (ga, gb), ref64, ref32)
    if name == "het":  # nan in the padded slots of g: not read
        gn = torch.where(idx.cpu() < 0, torch.full_like(g, float("nan")), g)
        assert torch.isnan(gn).any()
        _, na, nb = _grads(p1, p2, l1, l2, K, norm, gn)
        assert torch.isfinite(na).all() and torch.isfinite(nb).all()
        assert torch.equal(na, ga) and torch.equal(nb, gb)
        assert (ga[3] == 0).all() and (ga[1, 1:] == 0).all() and (gb[2] == 0).all() and (gb[0, 500:] == 0).all()


@pytest.mark.parametrize("norm", [2, 1])
def test_return_nn_gradient_adds_to_the_dists_path(norm):
    p1, p2, l1, l2 = KR.case("het")
    K = 8
    gd, gk = _upstream((4, 257, K), seed=41), _upstream((4, 257, K, 3), seed=42)
    a, b = _dev(p1).requires_grad_(True), _dev(p2).requires_grad_(True)
    out = knn_points(a, b, _dev(l1), _dev(l2), K=K, norm=norm, return_nn=True)
    ga, gb = torch.autograd.grad((out.dists * _dev(gd)).sum() + (out.knn * _dev(gk)).sum(), (a, b))
    idx = _ref("het", K, norm)[1]
    refs = []
    for dt in (torch.float64, torch.float32):
        ra, rb = p1.to(dt).requires_grad_(True), p2.to(dt).requires_grad_(True)
        d = KR.dists_from_idx(ra, rb, idx, norm)
        nn = knn_gather(rb, idx.clamp(min=0).long(), l2)
        refs.append(torch.autograd.grad((d * gd.to(dt)).sum() + (nn * gk.to(dt)).sum(), (ra, rb)))
    _check_grads(f"het return_nn norm={norm}", (ga, gb), refs[0], refs[1])


# --------------------------------------------------------------------------- determinism, graph capture
def _step(p1, p2, g, K=16):
    a, b = p1.detach().requires_grad_(True), p2.detach().requires_grad_(True)
    dists, idx = kernels.KnnPoints.apply(a, b, None, None, K, 2)
    ga, gb = torch.autograd.grad(dists, (a, b), g)
    return dists.detach(), idx, ga, gb


def test_two_runs_are_bitwise_equal():
    p1, p2, _, _ = KR.case("1x1000x1000")
    p1, p2, g = _dev(p1), _dev(p2), _dev(_upstream((1, 1000, 16), seed=51))
    for u, w in zip(_step(p1, p2, g), _step(p1, p2, g)):
        assert torch.equal(u, w)


def test_hip_graph_capture_replays_the_eager_step():
    p1, p2, _, _ = KR.case("1x1000x1000")
    p1, p2, g = _dev(p1), _dev(p2), _dev(_upstream((1, 1000, 16), seed=52))
    eager = _step(p1, p2, g)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _step(p1, p2, g)  # warm-up on the side stream: workspace sizes cached, allocator primed
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _step(p1, p2, g)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for u, w in zip(eager, captured):
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
        assert torch.equal(got[1].cpu(), ri) and torch.equal(got[0].cpu().view(torch.int32), rd.view(torch.int32))
        for u, w in zip(eager, got):
            assert torch.equal(u, w)
