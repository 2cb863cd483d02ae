"""chamfer_distance, sample_points_from_meshes and their kernels (csrc/mr_points.hip) on the GPU against the
plain-torch restatements of tests/points_ref.py run on the CPU.

* nearest_points: dist and idx BITWISE the float32 restatement (same operation order, first minimum), for both
  norms, cloud sizes from 1 to 5000, heterogeneous and zero lengths, exact ties with duplicated targets, and the
  sizes at which the staged chunk is 64, 192 and its maximum of 1024 targets (the chunk never holds more than 1024
  targets, so the (300, 5000) case already merges 79 chunks with atomicMin; `chunks-1024` splits 1100 targets into
  a full chunk and a partial one);
* chamfer loss: within 1e-5 relative of the float64 restatement (its own argmin), every reduction, weights, single
  direction, heterogeneous lengths; the float32 restatement's own error is printed beside;
* chamfer gradients: every entry within 1e-4 * max|ref64| of the float64 gradient taken with the float32 neighbours;
* SamplePoints: points within 1e-6 * max(1, |ref|) (six float32 roundings of magnitude <= max|v|), vertex gradient
  within 1e-4 * max|ref64|; sample_points_from_meshes: seeds, bounding boxes, area shares;
* determinism, HIP graph capture, and the geometry-fitting loop the two functions were written for.
"""
import functools
import itertools

import pytest
import torch

from tests import points_ref as R
from tests.mesh_priors_ref import brute_topology, priors_from_topology, topology_to
from torch_renderer_amd import Meshes, kernels
from torch_renderer_amd.loss import chamfer_distance, mesh_shape_priors
from torch_renderer_amd.ops import sample_points_from_meshes
from torch_renderer_amd.utils import ico_sphere

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _lattice_ties():
    """Targets: the 4x4x4 integer lattice twice over; queries: lattice + 0.5."""
    r = torch.arange(4, dtype=torch.float32)
    lat = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    return (lat + 0.5)[None], torch.cat([lat, lat], 0)[None]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, y, x_lengths, y_lengths) of a case on the CPU (never modified)."""
    if name == "ties":
        return _lattice_ties() + (None, None)
    if name == "het":  # heterogeneous lengths, one empty x cloud and one empty y cloud
        P1, P2 = 257, 1000
        return (_randn(4, P1, 3, seed=1), _randn(4, P2, 3, seed=2), torch.tensor([P1, 1, P1 // 2, 0]),
                torch.tensor([P2 // 2, P2, 0, P2]))
    if name == "het3":  # the same without the empty clouds
        x, y, xl, yl = _case("het")
        return x[:3], y[:3], xl[:3], torch.tensor([500, 1000, 1])
    if name == "one-target":  # every query shares one nearest target: the deepest scatter
        return _randn(1, 1000, 3, seed=3), _randn(1, 1, 3, seed=4), None, None
    if name == "chunks-192":  # 8 clouds x 1 query tile: the 20,000 targets are staged 192 at a time
        return _randn(8, 100, 3, seed=5), _randn(8, 20000, 3, seed=6), None, None
    if name == "chunks-1024":  # 600 clouds: no splitting is wanted, the chunk is the maximum (1024 + 76 targets)
        return _randn(600, 1, 3, seed=7), _randn(600, 1100, 3, seed=8), None, None
    P1, P2 = (int(v) for v in name.split("x"))
    return _randn(1, P1, 3, seed=P1), _randn(1, P2, 3, seed=P2 + 1), None, None


@functools.lru_cache(maxsize=None)
def _nn(name, norm, dtype):
    x, y, xl, yl = _case(name)
    return R.nearest_ref(x, y, xl, yl, norm, dtype)


def _dev(t):
    return None if t is None else t.to(DEV)


# --------------------------------------------------------------------------- nearest neighbours, bitwise
@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("name", ["1x1", "63x65", "257x1000", "1000x1000", "300x5000", "het", "ties", "one-target",
                                  "chunks-192", "chunks-1024"])
def test_nearest_points_bitwise(name, norm):
    x, y, xl, yl = _case(name)
    got = kernels.nearest_points(_dev(x), _dev(y), _dev(xl), _dev(yl), norm=norm)
    torch.cuda.synchronize()
    ref = _nn(name, norm, torch.float32)
    for nm, a, b in zip(("dist_x", "idx_x", "dist_y", "idx_y"), got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape, nm
        assert torch.equal(a.cpu(), b), (name, norm, nm, (a.cpu() != b).sum().item())
    if name == "het":
        assert ref[1][3].max() == -1 and ref[1][2].max() == -1 and ref[3][2].max() == -1 and ref[3][3].max() == -1


def test_ties_case_has_every_multiplicity():
    """Checked on the CPU: each query has 1, 2, 4 or 8 equidistant targets in the first copy (and as many again in
    the second), and the restatement picks the lowest of them."""
    x, y, _, _ = _case("ties")
    for norm in (1, 2):
        d = R.pair_dist(x[0], y[0], norm)
        cnt = (d[:, :64] == d.min(1, keepdim=True).values).sum(1)
        assert sorted(set(cnt.tolist())) == [1, 2, 4, 8]
        assert torch.equal((d == d.min(1, keepdim=True).values).sum(1), 2 * cnt)
        idx = _nn("ties", norm, torch.float32)[1][0].long()
        assert torch.equal(idx, (d == d.min(1, keepdim=True).values).float().argmax(1)) and idx.max() < 64


# --------------------------------------------------------------------------- chamfer loss and gradients
def _weights(N):
    return torch.linspace(0.5, 2.0, N)


def _upstream(N, batch_reduction):
    return torch.linspace(0.7, 1.3, N) if batch_reduction is None else torch.tensor(0.9)


def _check_chamfer(name, norm=2, weighted=False, **kw):
    x, y, xl, yl = _case(name)
    N = x.shape[0]
    w = _weights(N) if weighted else None
    go = _upstream(N, kw.get("batch_reduction", "mean"))
    xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    loss, normals = chamfer_distance(xg, yg, _dev(xl), _dev(yl), weights=_dev(w), norm=norm, **kw)
    (loss * go.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert normals is None and loss.dtype == torch.float32 and loss.device == DEV
    assert loss.shape == ((N,) if kw.get("batch_reduction", "mean") is None else ())

    rk = dict(x_lengths=xl, y_lengths=yl, weights=w, norm=norm, **kw)
    i32 = _nn(name, norm, torch.float32)
    i64 = _nn(name, norm, torch.float64)
    l64, _, _ = R.chamfer_ref(x, y, idx=(i64[1], i64[3]), dtype=torch.float64, **dict(rk))
    l32, _, _ = R.chamfer_ref(x, y, idx=(i32[1], i32[3]), dtype=torch.float32, **dict(rk))
    scale = l64.abs().max().item()
    err = (loss.detach().cpu().double() - l64).abs().max().item()
    own = (l32.double() - l64).abs().max().item()
    tag = f"{name} norm={norm} w={weighted} {kw}"
    print(f"[chamfer] {tag}: loss rel err {err / scale:.2e} (f32 restatement {own / scale:.2e})")
    assert err <= 1e-5 * scale, (tag, err, scale)

    _, gx64, gy64 = R.chamfer_ref(x, y, idx=(i32[1], i32[3]), dtype=torch.float64, grad_out=go, **dict(rk))
    for nm, g, r in (("grad_x", xg.grad, gx64), ("grad_y", yg.grad, gy64)):
        bar = 1e-4 * r.abs().max().item()
        e = (g.cpu().double() - r).abs().max().item()
        print(f"[chamfer] {tag} {nm}: max|err| {e:.3e}, bar {bar:.3e}")
        assert torch.isfinite(g).all() and e <= bar, (tag, nm, e, bar)


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("point_reduction,batch_reduction", list(itertools.product(("mean", "sum"),
                                                                                   ("mean", "sum", None))))
def test_chamfer_reductions(point_reduction, batch_reduction, weighted, single):
    _check_chamfer("het", weighted=weighted, point_reduction=point_reduction, batch_reduction=batch_reduction,
                   single_directional=single)


@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("name", ["1000x1000", "het3", "ties", "one-target", "300x5000"])
def test_chamfer_cases(name, norm):
    _check_chamfer(name, norm=norm)


def test_chamfer_norm1_reductions_and_no_grad():
    _check_chamfer("het", norm=1, weighted=True, point_reduction="sum", batch_reduction=None)
    _check_chamfer("het", norm=1, weighted=True, point_reduction="mean", batch_reduction="sum",
                   single_directional=True)
    x, y, xl, yl = _case("het")
    a, _ = chamfer_distance(x.to(DEV), y.to(DEV), _dev(xl), _dev(yl))
    b, _ = chamfer_distance(x.to(DEV).requires_grad_(True), y.to(DEV), _dev(xl), _dev(yl))
    assert not a.requires_grad and b.requires_grad and torch.equal(a, b.detach())
    zero, _ = chamfer_distance(x.to(DEV), y.to(DEV), weights=torch.zeros(4, device=DEV))
    assert zero.item() == 0.0  # upstream: a zero weight sum gives a zero loss


# --------------------------------------------------------------------------- SamplePoints
def _ico0():
    m = ico_sphere(0)
    return m.verts_list()[0].float() * 1.7 + 0.3, m.faces_list()[0]


def _hand_samples(F, N=2):
    """face_idx (N,S) and uv (2,N,S), S = 2 F + 40: every face hit twice and face 3 another 40 times, uv at 0, next
    to 1 and inside."""
    near1 = torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)).item()
    fi = torch.cat([torch.arange(F), torch.full((40,), 3), torch.arange(F)])[None].repeat(N, 1)
    S = fi.shape[1]
    fi[1] = fi[1].flip(0)
    uv = torch.rand(2, N, S, generator=torch.Generator().manual_seed(11))
    corners = list(itertools.product((0.0, near1, 0.5), repeat=2))
    for k, (u, v) in enumerate(corners):
        uv[0, :, k], uv[1, :, k] = u, v
        uv[0, 0, 30 + k], uv[1, 0, 30 + k] = u, v  # and on the much-hit face
    return fi, uv


def _sample_ref64(v, f, fi, uv, gp):
    vr = v.double().requires_grad_(True)
    p = R.sample_ref(vr, f, fi, uv.double())
    g, = torch.autograd.grad(p, vr, gp.double())
    return p.detach(), g


def test_sample_points_forward_and_gradient():
    v, f = _ico0()
    fi, uv = _hand_samples(f.shape[0])
    assert set(fi.flatten().tolist()) == set(range(20))
    gp = _randn(*fi.shape, 3, seed=12)
    p64, g64 = _sample_ref64(v, f, fi, uv, gp)
    leaf = v.to(DEV).requires_grad_(True)
    p = kernels.SamplePoints.apply(leaf, f.to(DEV), fi.to(DEV), uv.to(DEV))
    p.backward(gp.to(DEV))
    torch.cuda.synchronize()
    assert p.shape == fi.shape + (3,) and p.dtype == torch.float32
    err = ((p.detach().cpu().double() - p64).abs() / p64.abs().clamp(min=1.0)).max().item()
    print(f"[sample] points max err / max(1,|ref|) {err:.2e}")
    assert err <= 1e-6
    bar = 1e-4 * g64.abs().max().item()
    e = (leaf.grad.cpu().double() - g64).abs().max().item()
    print(f"[sample] vertex grad max|err| {e:.3e}, bar {bar:.3e}")
    assert e <= bar
    areas = kernels.face_areas(v.to(DEV), f.to(DEV))
    a64 = R.face_areas_ref(v.double(), f)
    assert ((areas.cpu().double() - a64).abs() <= 1e-6 * a64).all()


def test_sample_points_mesh_without_faces_in_a_batch():
    v, f = _ico0()
    fi, uv = _hand_samples(f.shape[0])
    fi[1] = -1  # the second mesh of the batch has no faces
    leaf = v.to(DEV).requires_grad_(True)
    p = kernels.SamplePoints.apply(leaf, f.to(DEV), fi.to(DEV), uv.to(DEV))
    p.sum().backward()
    one = v.to(DEV).requires_grad_(True)
    q = kernels.SamplePoints.apply(one, f.to(DEV), fi[:1].to(DEV), uv[:, :1].contiguous().to(DEV))
    q.sum().backward()
    assert torch.equal(p[1], torch.zeros_like(p[1])) and torch.equal(p[0], q[0]) and torch.equal(leaf.grad, one.grad)
    # through the public function: the empty mesh's rows are zeros and its vertices take a zero gradient
    a, b = v.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    m = Meshes([a, b], [f.to(DEV), torch.zeros((0, 3), dtype=torch.int64, device=DEV)])
    pts = sample_points_from_meshes(m, 50)
    pts.sum().backward()
    assert pts.shape == (2, 50, 3) and torch.equal(pts[1], torch.zeros_like(pts[1])) and pts[0].abs().max() > 0
    assert a.grad.abs().max() > 0 and (b.grad is None or b.grad.abs().max() == 0)


def test_sample_points_extended_batch_sums_the_copies():
    v, f = _ico0()
    F, V = f.shape[0], v.shape[0]
    fi, uv = _hand_samples(F, N=3)
    gp = _randn(*fi.shape, 3, seed=13)
    leaf = v.to(DEV).requires_grad_(True)
    kernels.SamplePoints.apply(leaf, f.to(DEV), fi.to(DEV), uv.to(DEV)).backward(gp.to(DEV))
    copies = v.repeat(3, 1).to(DEV).requires_grad_(True)  # three materialised copies
    f3 = torch.cat([f + k * V for k in range(3)], 0).to(DEV)
    fi3 = (fi + F * torch.arange(3)[:, None]).to(DEV)
    kernels.SamplePoints.apply(copies, f3, fi3, uv.to(DEV)).backward(gp.to(DEV))
    want = copies.grad.view(3, V, 3).double().sum(0)
    assert (leaf.grad.double() - want).abs().max().item() <= 1e-6 * want.abs().max().item()
    # the public function on Meshes.extend(3): independent draws per copy, one gradient on the shared vertices;
    # the barycentric weights of a sample sum to 1, so d(sum of points)/d(vertices) sums to 3 * S per coordinate
    src = v.to(DEV).requires_grad_(True)
    torch.manual_seed(5)
    pts = sample_points_from_meshes(Meshes([src], [f.to(DEV)]).extend(3), 200)
    pts.sum().backward()
    assert pts.shape == (3, 200, 3) and not torch.equal(pts[0], pts[1]) and not torch.equal(pts[1], pts[2])
    assert src.grad.shape == (V, 3) and (src.grad.sum(0) - 600.0).abs().max().item() <= 600.0 * 1e-5


# --------------------------------------------------------------------------- sample_points_from_meshes
def test_sample_points_from_meshes_seed_and_bounds():
    v, f = _ico0()
    v2 = v * torch.tensor([0.5, 2.0, 1.0]) - 1.0
    m = Meshes([v.to(DEV), v2.to(DEV)], [f.to(DEV), f[:11].to(DEV)])  # different face counts: the padded draw
    torch.manual_seed(3)
    a = sample_points_from_meshes(m, 1000)
    torch.manual_seed(3)
    b = sample_points_from_meshes(m, 1000)
    torch.manual_seed(4)
    c = sample_points_from_meshes(m, 1000)
    assert a.shape == (2, 1000, 3) and torch.equal(a, b) and not torch.equal(a, c)
    for k, vv in enumerate((v, v2[f[:11].unique()])):
        tol = 6 * 2.0 ** -24 * vv.abs().max().item()  # six float32 roundings of magnitude <= max|v|
        lo, hi = vv.min(0).values.to(DEV) - tol, vv.max(0).values.to(DEV) + tol
        assert ((a[k] >= lo) & (a[k] <= hi)).all()
    assert sample_points_from_meshes(Meshes([v.to(DEV)], [f.to(DEV)])).shape == (1, 10000, 3)


def test_sample_points_from_meshes_area_share():
    """Two triangles of areas 3 : 1 (the small one at z = 1): the large face's share of S = 20,000 samples is
    0.75 +- 0.015, 5 sigma of the binomial (sigma = 0.0031)."""
    v = torch.tensor([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 1.0],
                      [0.0, 2.0, 1.0]])
    f = torch.tensor([[0, 1, 2], [3, 4, 5]])
    assert kernels.face_areas(v.to(DEV), f.to(DEV)).tolist() == [3.0, 1.0]
    torch.manual_seed(0)
    p = sample_points_from_meshes(Meshes([v.to(DEV)], [f.to(DEV)]), 20000)
    z = p[0, :, 2]
    assert ((z == 0) | ((z - 1).abs() <= 1e-6)).all()
    share = (z == 0).float().mean().item()
    print(f"[sample] share on the large face {share:.4f}")
    assert abs(share - 0.75) <= 0.015


# --------------------------------------------------------------------------- determinism, graph, the loop
def _cow_like_step(seed):
    src, trg = ico_sphere(2), ico_sphere(1)
    leaf = src.verts_list()[0].float().to(DEV).requires_grad_(True)
    tv = (trg.verts_list()[0].float() * 0.7 + 0.2).to(DEV).requires_grad_(True)
    torch.manual_seed(seed)
    ps = sample_points_from_meshes(Meshes([leaf], [src.faces_list()[0].to(DEV)]), 1000)
    pt = sample_points_from_meshes(Meshes([tv], [trg.faces_list()[0].to(DEV)]), 1000)
    loss, _ = chamfer_distance(pt, ps)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), leaf.grad, tv.grad


def test_two_runs_are_bitwise_equal():
    a, b, c = _cow_like_step(7), _cow_like_step(7), _cow_like_step(8)
    for u, w in zip(a, b):
        assert torch.equal(u, w)
    assert not torch.equal(a[1], c[1])
    assert a[1].abs().max() > 0 and a[2].abs().max() > 0


def test_hip_graph_capture_replays_the_eager_step():
    x = _randn(2, 700, 3, seed=20).to(DEV).requires_grad_(True)
    y = _randn(2, 900, 3, seed=21).to(DEV).requires_grad_(True)
    w = torch.tensor([1.0, 0.5], device=DEV)

    def step():
        x.grad = y.grad = None
        loss, _ = chamfer_distance(x, y, weights=w, batch_reduction=None)
        (loss * w).sum().backward()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    x.grad = y.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, pool=torch.cuda.graph_pool_handle()):
        out = step()
    out = out.detach()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    got = [out.clone(), x.grad.clone(), y.grad.clone()]
    eager = [step().detach(), x.grad, y.grad]
    torch.cuda.synchronize()
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    del graph, out


def test_geometry_fitting_loop_converges():
    """mesh_deformer.py:299-352 geometry_train: ico_sphere(2) + a zero deform_verts leaf fitted to the sphere scaled
    by 0.7 and shifted by 0.2; per step two sample_points_from_meshes(..., 1000), chamfer_distance and the shape
    priors with the reference's weights (1, 1, 0.01, 0.1); SGD lr 1.0, momentum 0.9, 30 steps. The chamfer term at
    the last step is below half its first value (the float64 CPU restatement of the same loop with its own draws,
    loop_ref64 below, goes from 0.2487 to 0.0175, 0.07 of its first value, so the factor stands), every loss
    finite."""
    sph = ico_sphere(2)
    v0, f = sph.verts_list()[0].float().to(DEV), sph.faces_list()[0].to(DEV)
    src = Meshes([v0], [f])
    trg = Meshes([v0 * 0.7 + 0.2], [f])
    deform = torch.zeros_like(v0, requires_grad=True)
    opt = torch.optim.SGD([deform], lr=1.0, momentum=0.9)
    torch.manual_seed(0)
    hist = []
    for _ in range(30):
        opt.zero_grad()
        new_src = src.offset_verts(deform)
        sample_trg = sample_points_from_meshes(trg, 1000)
        sample_src = sample_points_from_meshes(new_src, 1000)
        loss_chamfer, _ = chamfer_distance(sample_trg, sample_src)
        edge, lap, normal = mesh_shape_priors(new_src)
        total = loss_chamfer * 1.0 + edge * 1.0 + normal * 0.01 + lap * 0.1
        total.backward()
        opt.step()
        hist.append([t.detach() for t in (loss_chamfer, edge, normal, lap, total)])
    vals = torch.stack([torch.stack(h) for h in hist]).cpu()
    print(f"[loop] chamfer first {vals[0, 0].item():.5f} last {vals[-1, 0].item():.5f}")
    assert torch.isfinite(vals).all() and torch.isfinite(deform).all()
    assert vals[-1, 0].item() < 0.5 * vals[0, 0].item()


def loop_ref64(steps=30, S=1000):
    """The float64 CPU restatement of test_geometry_fitting_loop_converges (its own draws): chamfer per step."""
    sph = ico_sphere(2)
    v0, f = sph.verts_list()[0].double(), sph.faces_list()[0]
    topo = topology_to(brute_topology([f], [v0.shape[0]]), "cpu", torch.float64)
    tv = v0 * 0.7 + 0.2
    deform = torch.zeros_like(v0, requires_grad=True)
    opt = torch.optim.SGD([deform], lr=1.0, momentum=0.9)
    torch.manual_seed(0)
    out = []

    def draw(v):
        fi = torch.multinomial(R.face_areas_ref(v.detach(), f)[None], S, replacement=True)
        return R.sample_ref(v, f, fi, torch.rand(2, 1, S, dtype=torch.float64))

    for _ in range(steps):
        opt.zero_grad()
        v = v0 + deform
        pt, ps = draw(tv), draw(v)
        _, ix, _, iy = R.nearest_ref(pt, ps, dtype=torch.float64)
        cham = R.chamfer_from_idx(pt, ps, ix, iy)
        edge, lap, normal = priors_from_topology(v, topo, 0.0)
        (cham + edge + 0.01 * normal + 0.1 * lap).backward()
        opt.step()
        out.append(cham.item())
    return out
