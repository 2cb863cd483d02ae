"""sample_farthest_points on the MI355X (csrc/mr_fps.hip) against the CPU restatement of tests/fps_ref.py.

* forward: idx bitwise the float32 restatement's (the first position of the maximum: the lowest index among equal
  distances) and pts bitwise points[idx], over every (threads, points per thread) pair the library builds, the
  boundaries kernels.farthest_geometry reports, the streamed path, ragged batches, K per cloud and explicit starts;
* the public padding, dtypes, Pointclouds input and random_start_point;
* the gradient of selected_points: exactly the CPU scatter-add of the upstream gradient at idx. The upstream values
  are small integers, so a row selected several times has one sum whatever the order of its addends;
* determinism and HIP graph capture.
"""
import functools

import pytest
import torch

from tests import fps_ref as FR
from torch_renderer_amd import kernels
from torch_renderer_amd.ops import sample_farthest_points
from torch_renderer_amd.structures import Pointclouds

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(t):
    if isinstance(t, tuple):
        return torch.tensor(t, dtype=torch.int64, device=DEV)
    return t.to(DEV) if torch.is_tensor(t) else t


@functools.lru_cache(maxsize=None)
def _ref(name):
    return FR.fps_ref(*FR.case(name))


def _run(points, lengths=None, K=50, start=None):
    out = kernels.farthest_points(_dev(points), _dev(lengths), _dev(K), _dev(start))
    torch.cuda.synchronize()
    return out


def _check(tag, got, ref, points):
    idx, pts = got
    ri, rp = ref
    assert idx.dtype == torch.int32 and pts.dtype == torch.float32 and idx.shape == ri.shape and pts.shape == rp.shape
    assert torch.equal(idx.cpu(), ri), (tag, (idx.cpu() != ri).sum().item())
    assert torch.equal(pts.cpu().view(torch.int32), rp.view(torch.int32)), tag
    # pts is points[idx], 0 in the unused slots
    want = torch.where((ri >= 0)[..., None], points.gather(1, ri.clamp(min=0).long()[..., None].expand(-1, -1, 3)),
                       torch.zeros(()))
    assert torch.equal(pts.cpu().view(torch.int32), want.view(torch.int32)), tag


# --------------------------------------------------------------------------- forward, bitwise
# one wave; several waves; every (threads, points per thread) pair: 64 x 1, 2, 4; 256 x 2, 4, 8; 1,024 x 4, 8, 16, 32
CASES = ["1x50k10", "1x100k20", "1x200k20", "1x300k40", "2x600k20", "1x1500k40", "1x2100k12", "1x5000k12", "1x9000k12",
         "1x17000k12", "lattice", "same", "ragged", "klist", "kmore", "start"]


@pytest.mark.parametrize("name", CASES)
def test_fps_bitwise(name):
    points, lengths, K, start = FR.case(name)
    ri, _ = _ref(name)
    _check(name, _run(points, lengths, K, start), _ref(name), points)
    if name == "same":
        assert ri[0].tolist() == [3, 0, 0, 0, 0, 0]
    if name == "ragged":
        assert (ri[0] == -1).all() and ri[1].tolist() == [0] + [-1] * 11 and (ri[2, :7] >= 0).all()
        assert (ri[2, 7:] == -1).all() and (ri[3] >= 0).all()
    if name == "kmore":
        assert ri.shape == (3, 100) and (ri[0, 4:] == -1).all() and (ri[1, :90] >= 0).all() and (ri[1, 90:] == -1).all()
    if name == "start":
        assert ri[:, 0].tolist() == [299, 77, 1]


def test_cases_cover_every_instantiation():
    seen = {kernels.farthest_geometry(*FR.case(n)[0].shape[:2], 1)[:2] for n in CASES}
    assert len(seen) == 10, sorted(seen)


@pytest.mark.parametrize("P0", [50, 300, 1500])
def test_boundaries_of_the_geometry(P0):
    """P exactly at, one below and one above the (threads x points per thread) capacity the geometry reports."""
    threads, per, streamed = kernels.farthest_geometry(1, P0, 16)
    edge = threads * per
    assert not streamed and kernels.farthest_geometry(1, edge, 16) == (threads, per, False)
    assert kernels.farthest_geometry(1, edge + 1, 16) != (threads, per, False)
    for P in (edge - 1, edge, edge + 1):
        points = FR.cloud(1, P)
        _check(P, _run(points, K=16), FR.fps_ref(points, K=16), points)


def test_streamed_path():
    """One point above the register capacity: the cloud is read from global memory every round. A second cloud of the
    batch is short: its m values lie behind the first cloud's in the workspace."""
    P = FR.register_capacity(kernels.farthest_geometry) + 1
    assert kernels.farthest_geometry(2, P, 4)[2] and not kernels.farthest_geometry(2, P - 1, 4)[2]
    points = FR.cloud(2, P)
    lengths, start = torch.tensor([P, 70]), torch.tensor([P - 1, 5])
    _check("streamed", _run(points, lengths, 4, start), FR.fps_ref(points, lengths, 4, start), points)


def test_k_as_int_list_and_tensor():
    points, lengths, K, _ = FR.case("kmore")
    ri, rp = _ref("kmore")
    for k in (list(K), torch.tensor(K), torch.tensor(K, device=DEV)):
        pts, idx = sample_farthest_points(_dev(points), _dev(lengths), k)
        assert idx.shape == (3, 100) and torch.equal(idx.cpu(), ri.long()) and torch.equal(pts.cpu(), rp)
    pts, idx = sample_farthest_points(_dev(points), _dev(lengths), 100)  # an int above every length
    r100 = FR.fps_ref(points, lengths, 100)
    assert torch.equal(idx.cpu(), r100[0].long()) and torch.equal(pts.cpu(), r100[1])
    assert (idx[0, 4:] == -1).all() and (idx[2, 60:] == -1).all() and (idx[1, :90] >= 0).all()


# --------------------------------------------------------------------------- the public layer
def test_public_padding_dtypes_and_pointclouds():
    points, lengths, K, _ = FR.case("ragged")
    ri, rp = _ref("ragged")
    pts, idx = sample_farthest_points(_dev(points), _dev(lengths), K)
    assert idx.dtype == torch.int64 and pts.dtype == torch.float32 and idx.shape == (4, 12) and pts.shape == (4, 12, 3)
    assert torch.equal(idx.cpu(), ri.long()) and torch.equal(pts.cpu(), rp)
    pad = idx < 0
    assert pad.any() and (idx[pad] == -1).all() and (pts[pad] == 0).all() and pad[0].all() and not pad[3].any()
    # the default K = 50 and no lengths
    p50, i50 = sample_farthest_points(_dev(points))
    r50 = FR.fps_ref(points, K=50)
    assert i50.shape == (4, 50) and torch.equal(i50.cpu(), r50[0].long()) and torch.equal(p50.cpu(), r50[1])
    # the dtype is kept: float16 values are exact in float32, a float64 input is read as float32
    half = points.half()
    ph, ih = sample_farthest_points(_dev(half), _dev(lengths), K)
    rh = FR.fps_ref(half.float(), lengths, K)
    assert ph.dtype == torch.float16 and torch.equal(ih.cpu(), rh[0].long()) and torch.equal(ph.cpu(), rh[1].half())
    pd, idd = sample_farthest_points(_dev(points.double()), _dev(lengths), K)
    assert pd.dtype == torch.float64 and torch.equal(idd.cpu(), ri.long()) and torch.equal(pd.cpu(), rp.double())
    # a Pointclouds brings its lengths
    clouds = Pointclouds([_dev(points[n, :int(l)]) for n, l in enumerate(lengths)])
    pc, ic = sample_farthest_points(clouds, K=K)
    assert torch.equal(ic, idx) and torch.equal(pc, pts)
    full = Pointclouds(_dev(points))
    pf, jf = sample_farthest_points(full, K=K)
    rf = FR.fps_ref(points, K=K)
    assert torch.equal(jf.cpu(), rf[0].long()) and torch.equal(pf.cpu(), rf[1])
    # K = 0: empty tensors
    p0, i0 = sample_farthest_points(_dev(points), K=0)
    assert p0.shape == (4, 0, 3) and i0.shape == (4, 0) and i0.dtype == torch.int64


def test_random_start_point():
    points, lengths, _, _ = FR.case("ragged")
    lengths = torch.tensor([3, 1, 7, 300])
    K = 9
    torch.manual_seed(1234)
    pa, ia = sample_farthest_points(_dev(points), _dev(lengths), K, random_start_point=True)
    torch.manual_seed(1234)
    pb, ib = sample_farthest_points(_dev(points), _dev(lengths), K, random_start_point=True)
    assert torch.equal(ia, ib) and torch.equal(pa, pb)
    starts = ia[:, 0].cpu()
    assert ((starts >= 0) & (starts < lengths)).all(), starts.tolist()
    ri, rp = FR.fps_ref(points, lengths, K, starts)
    assert torch.equal(ia.cpu(), ri.long()) and torch.equal(pa.cpu(), rp)
    # without lengths the draws cover [0, P); over 64 clouds they are not all the same
    many = FR.cloud(64, 40)
    _, im = sample_farthest_points(_dev(many), K=3, random_start_point=True)
    s = im[:, 0].cpu()
    assert ((s >= 0) & (s < 40)).all() and len(set(s.tolist())) > 1
    rm = FR.fps_ref(many, K=3, start_idx=s)
    assert torch.equal(im.cpu(), rm[0].long())


# --------------------------------------------------------------------------- gradient
@pytest.mark.parametrize("name", ["ragged", "same", "kmore"])
def test_gradient_is_the_scatter_add(name):
    points, lengths, K, start = FR.case(name)
    ri, _ = _ref(name) if name != "same" else FR.fps_ref(points, K=6)
    if name == "same":  # the public call starts at 0: index 0 six times, whose gradients must sum
        start = None
        assert ri[0].tolist() == [0] * 6
    a = _dev(points).requires_grad_(True)
    pts, idx = sample_farthest_points(a, _dev(lengths), list(K) if isinstance(K, tuple) else K)
    assert pts.requires_grad and not idx.requires_grad and torch.equal(idx.cpu(), ri.long())
    g = torch.randint(-8, 9, pts.shape, generator=torch.Generator().manual_seed(61)).float()
    pts.backward(_dev(g))
    torch.cuda.synchronize()
    want = torch.zeros_like(points)
    for n in range(ri.shape[0]):
        for k in range(ri.shape[1]):
            if ri[n, k] >= 0:
                want[n, ri[n, k]] += g[n, k]
    assert a.grad.dtype == torch.float32 and torch.equal(a.grad.cpu(), want)
    if name == "same":
        assert torch.equal(a.grad[0, 0].cpu(), g[0].sum(0)) and (a.grad[0, 1:] == 0).all()


# --------------------------------------------------------------------------- determinism, graph capture
def _step(points, g, K=64):
    a = points.detach().requires_grad_(True)
    pts, idx = sample_farthest_points(a, K=K)
    ga, = torch.autograd.grad(pts, a, g)
    return pts.detach(), idx, ga


def test_two_runs_are_bitwise_equal():
    points = _dev(FR.cloud(3, 1500))
    g = _dev(torch.randn(3, 64, 3, generator=torch.Generator().manual_seed(71)))
    for u, w in zip(_step(points, g), _step(points, g)):
        assert torch.equal(u, w)


def test_hip_graph_capture_replays_the_eager_step():
    points = _dev(FR.cloud(3, 1500))
    g = _dev(torch.randn(3, 64, 3, generator=torch.Generator().manual_seed(72)))
    eager = _step(points, g)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _step(points, g)  # warm-up on the side stream: workspace sizes cached, allocator primed
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _step(points, g)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for u, w in zip(eager, captured):
        assert torch.equal(u, w)
    ri, rp = FR.fps_ref(points.cpu(), K=64)
    assert torch.equal(captured[1].cpu(), ri.long()) and torch.equal(captured[0].cpu(), rp)
