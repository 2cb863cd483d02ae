"""loss.posed_chamfer_distance / kernels.posed_chamfer (k_posed_nn, k_posed_final of csrc/mr_points.hip) on the GPU.

* neighbours: idx_x / idx_y BITWISE those of kernels.nearest_points on the materialised clouds
  (kernels.similarity_transform of x under every pose, y repeated), the distances those indices give bitwise its
  distances, and the loss the float64 sum of them rounded once. A workgroup takes 512 queries and stages 1,024
  targets at a time, so the shapes are a single point, a partial tile (63, 65), one past a tile and one past a chunk
  (513, 1025), and the pose-search shape (1000, 500); S = 1, 3 and 257;
* exact ties on an integer lattice, under the identity and a quarter turn with an integer translation, against the
  CPU restatement (tests/pose_chamfer_ref.py): every tie goes to the lowest index;
* the loss against chamfer_distance(batch_reduction=None) on the materialised clouds within 2 float32 ulps (both sum
  float32 distances in float64 and round once; the orders of the float64 sums differ), and against the float64
  restatement with the GPU's neighbours within 1e-4 * max(1, |ref|);
* the gradients to R, T, s (and through euler_angles_to_matrix) against float64 autograd of the restatement with the
  GPU's neighbours fixed, every entry within 1e-4 * max(1, max|ref|);
* bitwise reproducibility, HIP graph capture, and the pose search the function was written for.
"""
import functools

import pytest
import torch

from tests import pose_chamfer_ref as PR
from torch_renderer_amd import _lib, kernels
from torch_renderer_amd.loss import chamfer_distance, posed_chamfer_distance
from torch_renderer_amd.transforms import euler_angles_to_matrix

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(1, 1), (63, 65), (513, 1025), (1000, 500)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _clouds(P1, P2):
    g = _gen(1000 * P1 + P2)
    return torch.randn(P1, 3, generator=g), torch.randn(P2, 3, generator=g)


@functools.lru_cache(maxsize=None)
def _poses(S, seed=0):
    """(R, T, s) on the CPU (never modified): random rotations, shifts of 0.3 sigma, scales in [0.5, 1.5)."""
    g = _gen(77 + S + seed)
    R = euler_angles_to_matrix(torch.randn(S, 3, generator=g), "XYZ")
    return R, 0.3 * torch.randn(S, 3, generator=g), torch.rand(S, generator=g) + 0.5


def _rts(R, T, s):
    S = R.shape[0]
    sc = torch.ones(S, 1, device=R.device) if s is None else s.reshape(S, 1)
    return torch.cat((R.reshape(S, 9), T.reshape(S, 3), sc), 1).contiguous()


def _materialised(x, y, R, T, s):
    S = R.shape[0]
    xt = kernels.similarity_transform(x[None].expand(S, -1, -1), _rts(R, T, s))
    return xt, y[None].expand(S, -1, -1).contiguous()


def _dist_of(q, t, idx, norm):
    """Per-point distances of q (S,Pq,3) to t[idx] in the kernels' order, one torch op per operation."""
    nn = t.gather(1, idx.long()[..., None].expand(-1, -1, 3))
    d = q - nn
    if norm == 2:
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return (d[..., 0].abs() + d[..., 1].abs()) + d[..., 2].abs()


def _ulp(ref):
    a = ref.abs()
    return torch.nextafter(a, torch.full_like(a, float("inf"))) - a


# --------------------------------------------------------------------------- neighbours, bitwise
@pytest.mark.parametrize("with_s", [False, True])
@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("S", [1, 3, 257])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_neighbours_bitwise_those_of_the_materialised_clouds(shape, S, norm, with_s):
    x, y = (c.to(DEV) for c in _clouds(*shape))
    R, T, s = (p.to(DEV) for p in _poses(S))
    s = s if with_s else None
    out, ix, iy = kernels.posed_chamfer(x, y, R, T, s, norm=norm, flags=0, return_idx=True)
    xt, ye = _materialised(x, y, R, T, s)
    dx, jx, dy, jy = kernels.nearest_points(xt, ye, norm=norm)
    assert ix.dtype == torch.int32 and ix.shape == (S, shape[0]) and iy.shape == (S, shape[1])
    assert torch.equal(ix, jx) and torch.equal(iy, jy)
    assert torch.equal(_dist_of(xt, ye, ix, norm), dx) and torch.equal(_dist_of(ye, xt, iy, norm), dy)
    ref = (dx.double().sum(1) + dy.double().sum(1)).float()
    assert out.shape == (S,) and out.dtype == torch.float32
    assert bool(((out - ref).abs() <= _ulp(ref)).all()), (out - ref).abs().max().item()


# --------------------------------------------------------------------------- ties
def test_exact_ties_go_to_the_lowest_index():
    """x: the 4x4x4 integer lattice; y: the lattice + 0.5, twice over. Every x has up to 8 (x 2) equidistant targets
    and every y up to 8 equidistant sources. Pose 1 turns the lattice onto itself (x R = (-x1, x0, x2), T = (3,0,0)):
    all arithmetic is exact, so the distances tie exactly."""
    r = torch.arange(4, dtype=torch.float32)
    x = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    y = torch.cat((x + 0.5, x + 0.5), 0)
    R = torch.stack((torch.eye(3), torch.tensor([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])))
    T = torch.tensor([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
    for norm in (2, 1):
        dx, jx, dy, jy = PR.posed_nearest_ref(x, y, R, T, None, norm=norm)
        assert int(jx.max()) < 64  # the restatement itself never picks the duplicate
        out, ix, iy = kernels.posed_chamfer(x.to(DEV), y.to(DEV), R.to(DEV), T.to(DEV), norm=norm, flags=0,
                                            return_idx=True)
        assert torch.equal(ix.cpu(), jx) and torch.equal(iy.cpu(), jy)
        # multiples of 0.25 summed: exact in float64 and in float32, whatever the order
        assert torch.equal(out.cpu(), dx.sum(1) + dy.sum(1))


# --------------------------------------------------------------------------- the loss
@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("point_reduction", ["mean", "sum"])
def test_loss_against_chamfer_distance_and_the_float64_restatement(point_reduction, single, norm):
    x, y = (c.to(DEV) for c in _clouds(513, 1025))
    R, T, s = (p.to(DEV) for p in _poses(5))
    kw = dict(norm=norm, point_reduction=point_reduction, single_directional=single)
    got = posed_chamfer_distance(x[None], y[None], R, T[:, None], s, **kw)
    assert got.shape == (5,) and got.dtype == torch.float32 and not got.requires_grad
    xt, ye = _materialised(x, y, R, T, s)
    ref, _ = chamfer_distance(xt, ye, batch_reduction=None, **kw)
    err = (got - ref).abs()
    print("vs chamfer_distance, in ulps:", (err / _ulp(ref)).tolist())
    assert bool((err <= 2 * _ulp(ref)).all())
    # the same through the (R, T, s) triple and a non-contiguous R
    assert torch.equal(posed_chamfer_distance(x, y, (R, T, s), **kw), got)
    Rt = R.transpose(1, 2).contiguous().transpose(1, 2)
    assert not Rt.is_contiguous() and torch.equal(posed_chamfer_distance(x, y, Rt, T, s, **kw), got)
    flags = (_lib.MR_CHAMFER_POINT_MEAN if point_reduction == "mean" else 0) | (_lib.MR_CHAMFER_SINGLE if single else 0)
    out, ix, iy = kernels.posed_chamfer(x, y, R, T, s, norm=norm, flags=flags, return_idx=True)
    assert torch.equal(out, got) and (iy is None) == single
    r64, _, _, _ = PR.posed_chamfer_ref(x, y, R, T, s, idx=(ix, iy), **kw)
    e64 = (got.cpu().double() - r64).abs()
    print("vs float64 restatement:", e64.max().item())
    assert bool((e64 <= 1e-4 * r64.abs().clamp(min=1.0)).all())


# --------------------------------------------------------------------------- gradients
def _leaves(S, with_s=True):
    R, T, s = (p.to(DEV).clone().requires_grad_(True) for p in _poses(S))
    return R, T, (s if with_s else None)


def _close(got, ref, what):
    err = (got.detach().cpu().double() - ref).abs().max().item()
    bar = 1e-4 * max(1.0, ref.abs().max().item())
    print(f"{what}: max err {err:.3e}, bar {bar:.3e}")
    assert err <= bar, what


@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("shape", [(63, 65), (513, 1025)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("point_reduction,single", [("mean", False), ("sum", False), ("mean", True)])
def test_gradients_against_float64_autograd_with_the_gpu_neighbours(point_reduction, single, shape, norm):
    S = 4
    x, y = (c.to(DEV) for c in _clouds(*shape))
    R, T, s = _leaves(S)
    w = torch.tensor([1.0, -0.5, 2.0, 0.25], device=DEV)  # a non-uniform upstream gradient
    kw = dict(norm=norm, point_reduction=point_reduction, single_directional=single)
    loss = posed_chamfer_distance(x, y, R, T, s, **kw)
    (loss * w).sum().backward()
    flags = (_lib.MR_CHAMFER_POINT_MEAN if point_reduction == "mean" else 0) | (_lib.MR_CHAMFER_SINGLE if single else 0)
    _, ix, iy = kernels.posed_chamfer(x, y, R, T, s, norm=norm, flags=flags, return_idx=True)
    _, gR, gT, gs = PR.posed_chamfer_ref(x, y, R, T, s, idx=(ix, iy), grad_out=w, **kw)
    assert R.grad.shape == R.shape and T.grad.shape == T.shape and s.grad.shape == s.shape
    _close(R.grad, gR, "dR")
    _close(T.grad, gT, "dT")
    _close(s.grad, gs, "ds")
    if single:  # the y -> x terms are absent: the bidirectional gradient is another one
        _, jx, jy = kernels.posed_chamfer(x, y, R, T, s, norm=norm, flags=flags & ~_lib.MR_CHAMFER_SINGLE,
                                          return_idx=True)
        _, _, bT, _ = PR.posed_chamfer_ref(x, y, R, T, s, idx=(jx, jy), grad_out=w, norm=norm,
                                           point_reduction=point_reduction)
        assert (bT - gT).abs().max() > 1e-3 and torch.equal(jx, ix)


def test_gradient_without_a_scale_and_to_a_subset_of_the_pose():
    x, y = (c.to(DEV) for c in _clouds(63, 65))
    R, T, _ = _leaves(3, with_s=False)
    T3 = T.detach()[:, None].clone().requires_grad_(True)  # (S,1,3)
    posed_chamfer_distance(x, y, R.detach(), T3).sum().backward()
    assert T3.grad.shape == (3, 1, 3)
    _, ix, iy = kernels.posed_chamfer(x, y, R, T, return_idx=True)
    _, gR, gT, _ = PR.posed_chamfer_ref(x, y, R, T, None, idx=(ix, iy))
    _close(T3.grad[:, 0], gT, "dT alone")
    posed_chamfer_distance(x, y, R, T.detach()).sum().backward()
    _close(R.grad, gR, "dR alone")
    assert T.grad is None
    with torch.no_grad():
        assert not posed_chamfer_distance(x.requires_grad_(True), y, R, T).requires_grad
    with pytest.raises(NotImplementedError, match="requires grad"):
        posed_chamfer_distance(x, y, R, T)


def test_gradient_reaches_euler_angles():
    x, y = (c.to(DEV) for c in _clouds(63, 65))
    g = _gen(9)
    e0, T0 = torch.randn(3, 3, generator=g), 0.3 * torch.randn(3, 3, generator=g)
    e = e0.to(DEV).requires_grad_(True)
    T = T0.to(DEV).requires_grad_(True)
    R = euler_angles_to_matrix(e, "XYZ")
    posed_chamfer_distance(x, y, R, T).sum().backward()
    _, ix, iy = kernels.posed_chamfer(x, y, R.detach(), T.detach(), return_idx=True)
    e64 = e0.double().requires_grad_(True)
    T64 = T0.double().requires_grad_(True)
    ref = PR.posed_chamfer_from_idx(x.cpu(), y.cpu(), euler_angles_to_matrix(e64, "XYZ"), T64, None, ix.cpu(), iy.cpu())
    ge, gT = torch.autograd.grad(ref.sum(), (e64, T64))
    assert ge.abs().max() > 1e-3
    _close(e.grad, ge, "d euler")
    _close(T.grad, gT, "dT")


# --------------------------------------------------------------------------- reproducibility and capture
def _step_fn(norm=2):
    x, y = (c.to(DEV) for c in _clouds(1000, 500))
    R, T, s = _leaves(64)
    w = torch.linspace(0.5, 1.5, 64, device=DEV)

    def step():
        R.grad = T.grad = s.grad = None
        loss = posed_chamfer_distance(x, y, R, T, s, norm=norm)
        (loss * w).sum().backward()
        return loss

    return step, (R, T, s)


@pytest.mark.parametrize("norm", [2, 1])
def test_two_runs_agree_bitwise(norm):
    step, leaves = _step_fn(norm)
    a = [step().detach().clone()] + [l.grad.clone() for l in leaves]
    b = [step().detach().clone()] + [l.grad.clone() for l in leaves]
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert a[1].abs().max() > 0 and a[3].abs().max() > 0


def test_hip_graph_capture_replays_the_eager_step():
    step, (R, T, s) = _step_fn()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    R.grad = T.grad = s.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, pool=torch.cuda.graph_pool_handle()):
        out = step()
    out = out.detach()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    got = [out.clone(), R.grad.clone(), T.grad.clone(), s.grad.clone()]
    eager = [step().detach(), R.grad, T.grad, s.grad]
    torch.cuda.synchronize()
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    del graph, out


# --------------------------------------------------------------------------- the pose search
def test_pose_search_finds_the_true_pose_and_adam_refines_a_nearby_one():
    """pytorch3d_icp_evaluation.py:158-239's inner loop: a 500-point cloud (an anisotropic Gaussian, sigmas 1.5, 0.7,
    0.2, so that a rotation matters), the target its copy under a known pose with the tenth of the points of lowest x
    cropped away; 256 random hypotheses and the true one at index 100. The two-sided loss of the true pose is the
    crop's x -> y error alone: the CPU restatement gives 0.0671 for it and 0.1242 for the best random hypothesis, a
    margin far above float32 rounding, so the argmin is index 100. (A crop at the centroid does not have this
    property: there the restatement itself prefers poses that push the whole cloud into the kept half.) Then Adam on
    (euler, T) from 0.1 rad / 0.05 away: the float64 CPU restatement of the same 25 steps (lr 0.01) takes the loss
    from 0.1003 to 0.0639; the test asks for any decrease."""
    g = _gen(31)
    x = torch.randn(500, 3, generator=g) * torch.tensor([1.5, 0.7, 0.2])
    e_true = torch.tensor([0.4, -0.7, 1.1])
    T_true = torch.tensor([0.3, -0.2, 0.5])
    full = x @ euler_angles_to_matrix(e_true, "XYZ") + T_true
    y = full[full[:, 0] > full[:, 0].quantile(0.1)]
    assert y.shape[0] == 450
    e = torch.randn(257, 3, generator=g) * 1.5
    T = torch.randn(257, 3, generator=g) * 0.5
    e[100], T[100] = e_true, T_true
    xd, yd = x.to(DEV), y.to(DEV)
    loss = posed_chamfer_distance(xd, yd, euler_angles_to_matrix(e.to(DEV), "XYZ"), T.to(DEV))
    assert int(loss.argmin()) == 100
    ev = (e_true + 0.1).to(DEV).reshape(1, 3).requires_grad_(True)
    Tv = (T_true + 0.05).to(DEV).reshape(1, 3).requires_grad_(True)
    opt = torch.optim.Adam([ev, Tv], lr=0.01)
    hist = []
    for _ in range(25):
        opt.zero_grad()
        l = posed_chamfer_distance(xd, yd, euler_angles_to_matrix(ev, "XYZ"), Tv)
        l.sum().backward()
        opt.step()
        hist.append(l.detach())
    hist = torch.cat(hist).cpu()
    print("adam:", hist[0].item(), "->", hist[-1].item())
    assert torch.isfinite(hist).all() and hist[-1] < hist[0]
