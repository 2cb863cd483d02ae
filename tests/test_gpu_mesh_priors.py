"""The fused mesh shape priors (torch_renderer_amd.loss.mesh_shape_priors and the three upstream-named functions:
mr_mesh_priors_*, csrc/mr_priors.hip) on the GPU against the plain-torch restatement of tests/mesh_priors_ref.py
run on the CPU in float32 and float64.

* losses: within 1e-5 relative of the float64 value (the float32 restatement alone is within 7e-7);
* gradients, small meshes: every entry of each of the three gradients within 1e-4 * max|ref64| of the float64
  gradient (the float32 restatement alone is at most 0.02 of that bar), also with target_length = 0.3;
* gradients, cow and teapot (several workgroups, the multi-stage reduction): helpers.report against the float32
  restatement with the float64 one as the conditioning, and at most 5% of the entries ill-conditioned;
* an extended batch equals the single mesh, two calls are bitwise equal, the priors add to a soft-silhouette
  loss's gradient exactly, a captured HIP graph replays the eager result, a zero-area face keeps the loss finite.
"""
import functools

import pytest
import torch

from tests.helpers import mesh_arrays, report
from tests.mesh_priors_ref import brute_topology, fan_mesh, priors_ref, tetrahedron
from torch_renderer_amd import Meshes
from torch_renderer_amd import loss as L
from torch_renderer_amd.utils import ico_sphere

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _jitter(v, seed=0):
    return v + 0.05 * torch.randn(v.shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """[(verts, faces)] of a case, on the CPU (never modified)."""
    if name.startswith("ico"):
        m = ico_sphere(int(name[3]))
        return [(_jitter(m.verts_list()[0]), m.faces_list()[0])]
    if name == "fan":
        v, f = fan_mesh()
        return [(_jitter(v), f)]
    if name == "batch3":
        return _mesh("ico0") + _mesh("ico1") + _mesh("fan")
    v, f, _ = mesh_arrays(name)  # cow, teapot
    return [(v, f)]


@functools.lru_cache(maxsize=None)
def _ref(name, target_length, copies=1):
    """The restatement's (losses, gradients) in float32 and float64, computed once per case."""
    ms = _mesh(name) * copies
    vl, fl = [v for v, _ in ms], [f for _, f in ms]
    topo = brute_topology(fl, [v.shape[0] for v in vl])
    return (priors_ref(vl, fl, target_length, torch.float32, topo),
            priors_ref(vl, fl, target_length, torch.float64, topo))


def _gpu(ms, target_length=0.0, extend=None):
    """Fused losses and the three separate gradients w.r.t. the packed vertices."""
    leaves = [v.to(DEV).requires_grad_(True) for v, _ in ms]
    m = Meshes(leaves, [f.to(DEV) for _, f in ms])
    if extend:
        m = m.extend(extend)
    losses = L.mesh_shape_priors(m, target_length)
    grads = []
    for loss in losses:
        gs = torch.autograd.grad(loss, leaves, retain_graph=True)
        grads.append(torch.cat(gs, 0))
    torch.cuda.synchronize()
    return [x.detach() for x in losses], grads


NAMES = ("edge", "laplacian", "normal")


def _check_losses(name, got, r64):
    for nm, a, b in zip(NAMES, got, r64):
        assert a.shape == () and a.dtype == torch.float32 and a.device == DEV
        rel = abs(a.item() - b.item()) / abs(b.item())
        print(f"[priors] {name} {nm} loss: got {a.item():.8e}, f64 {b.item():.8e}, rel {rel:.2e}")
        assert rel <= 1e-5, (name, nm, a.item(), b.item())


@pytest.mark.parametrize("target_length", [0.0, 0.3])
@pytest.mark.parametrize("name", ["ico0", "ico1", "ico2", "fan", "batch3"])
def test_losses_and_gradients_strict(name, target_length):
    (_, g32), (l64, g64) = _ref(name, target_length)
    losses, grads = _gpu(_mesh(name), target_length)
    _check_losses(name, losses, l64)
    for nm, g, r32, r64 in zip(NAMES, grads, g32, g64):
        bar = 1e-4 * r64.abs().max().item()
        err = (g.cpu().double() - r64).abs().max().item()
        own = (r32.double() - r64).abs().max().item()
        print(f"[priors] {name} t={target_length} grad {nm}: max|err| {err:.3e} = {err / bar:.4f} of the bar "
              f"(f32 restatement {own / bar:.4f})")
        assert torch.isfinite(g).all() and err <= bar, (name, nm, err, bar)


@pytest.mark.parametrize("target_length", [0.0, 0.3])
def test_extended_batch_equals_the_single_mesh(target_length):
    (_, _), (l64, g64) = _ref("ico1", target_length, copies=4)  # the restatement over four materialised copies
    one_l, one_g = _gpu(_mesh("ico1"), target_length)
    ext_l, ext_g = _gpu(_mesh("ico1"), target_length, extend=4)
    _check_losses("ico1 x4", ext_l, l64)
    V = one_g[0].shape[0]
    for nm, a, b, r64 in zip(NAMES, ext_g, one_g, g64):
        assert a.shape == (V, 3) and torch.equal(a, b), nm  # the shared vertices take the gradient once
        shared = r64.reshape(4, V, 3).sum(0)  # the copies' gradients reach the one source tensor
        assert (a.cpu().double() - shared).abs().max().item() <= 1e-4 * shared.abs().max().item(), nm
    for a, b in zip(ext_l, one_l):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["cow", "teapot"])
def test_gradients_real_meshes(name):
    (l32, g32), (l64, g64) = _ref(name, 0.0)
    losses, grads = _gpu(_mesh(name))
    _check_losses(name, losses, l64)
    for nm, g, r32, r64 in zip(NAMES, grads, g32, g64):
        scale = r64.abs().max().item()
        tol = 1e-4 * scale
        ill = ((r32.double() - r64).abs() > 0.1 * tol).double().mean().item()
        print(f"[priors] {name} grad {nm}: ill-conditioned share {100 * ill:.2f}%")
        assert ill <= 0.05, (name, nm, ill)
        report(f"{name} priors grad {nm}", g, r32, tol=tol, rel_above_one=False, ref64=r64)


def test_single_term_functions_use_their_own_term():
    ms = _mesh("batch3")
    (_, _), (l64, g64) = _ref("batch3", 0.3)
    fns = (lambda m: L.mesh_edge_loss(m, 0.3), L.mesh_laplacian_smoothing, L.mesh_normal_consistency)
    fused_l, fused_g = _gpu(ms, 0.3)
    for k, fn in enumerate(fns):
        leaves = [v.to(DEV).requires_grad_(True) for v, _ in ms]
        out = fn(Meshes(leaves, [f.to(DEV) for _, f in ms]))
        out.backward()
        assert torch.equal(out.detach(), fused_l[k]), NAMES[k]
        assert torch.equal(torch.cat([x.grad for x in leaves], 0), fused_g[k]), NAMES[k]
    with torch.no_grad():  # no gradient rows are written; the values are the same
        vals = L.mesh_shape_priors(Meshes([v.to(DEV) for v, _ in ms], [f.to(DEV) for _, f in ms]), 0.3)
    assert all(torch.equal(a, b) and not a.requires_grad for a, b in zip(vals, fused_l))


def test_tetrahedron_and_no_adjacent_pairs():
    a = 0.37
    v, f = tetrahedron(a)
    m = Meshes([v.float().to(DEV)], [f.to(DEV)])
    edge, lap, normal = L.mesh_shape_priors(m)
    assert abs(edge.item() - a * a) <= 1e-5 * a * a
    assert abs(lap.item() - a * 6.0 ** 0.5 / 3.0) <= 1e-5 * a
    assert abs(normal.item() - 4.0 / 3.0) <= 1e-5
    assert abs(L.mesh_edge_loss(m, target_length=a).item()) <= 1e-12
    # two triangles that share no edge: normal consistency 0 with a zero gradient
    g = torch.Generator().manual_seed(1)
    leaf = torch.randn(6, 3, generator=g).to(DEV).requires_grad_(True)
    loss = L.mesh_normal_consistency(Meshes([leaf], [torch.tensor([[0, 1, 2], [3, 4, 5]], device=DEV)]))
    loss.backward()
    assert loss.item() == 0.0 and torch.equal(leaf.grad, torch.zeros_like(leaf))


def test_two_calls_are_bitwise_equal():
    a_l, a_g = _gpu(_mesh("cow"), 0.1)
    b_l, b_g = _gpu(_mesh("cow"), 0.1)
    for x, y in zip(a_l + a_g, b_l + b_g):
        assert torch.equal(x, y)


def test_priors_add_to_a_silhouette_loss():
    """deform = zeros; mesh = src.offset_verts(deform); total = sum(priors) + soft-silhouette MSE of one 32x32 view:
    deform.grad equals the sum of the two gradients taken in separate backward passes (two float32 addends)."""
    import math

    from torch_renderer_amd.cameras import PerspectiveCameras
    from torch_renderer_amd.mesh_renderer import (BlendParams, MeshRasterizer, MeshRenderer, RasterizationSettings,
                                                  SoftSilhouetteShader)
    from torch_renderer_amd.transforms import look_at_view_transform

    v, f = _mesh("ico2")[0]
    src = Meshes([v.to(DEV)], [f.to(DEV)])
    sigma = 1e-4
    R, T = look_at_view_transform(dist=2.7, elev=torch.tensor([20.0]), azim=torch.tensor([30.0]))
    rs = RasterizationSettings(image_size=(32, 32), blur_radius=math.log(1.0 / 1e-4 - 1.0) * sigma, faces_per_pixel=8,
                               perspective_correct=False)
    renderer = MeshRenderer(rasterizer=MeshRasterizer(cameras=PerspectiveCameras(device=DEV, R=R.to(DEV), T=T.to(DEV)),
                                                      raster_settings=rs),
                            shader=SoftSilhouetteShader(blend_params=BlendParams(sigma=sigma)))
    target = torch.zeros(1, 32, 32, device=DEV)
    target[:, 8:24, 8:24] = 1.0

    def grad(priors, sil):
        deform = torch.zeros(v.shape, device=DEV, requires_grad=True)
        mesh = src.offset_verts(deform)
        total = 0.0
        if priors:
            total = total + sum(L.mesh_shape_priors(mesh))
        if sil:
            total = total + ((renderer(mesh)[..., 3] - target) ** 2).mean()
        total.backward()
        return deform.grad

    both, gp, gs = grad(True, True), grad(True, False), grad(False, True)
    torch.cuda.synchronize()
    assert gp.abs().max() > 0 and gs.abs().max() > 0
    assert torch.allclose(both, gp + gs, rtol=1e-6, atol=1e-9)


def test_hip_graph_capture_replays_the_eager_step():
    v, f = _mesh("ico2")[0]
    leaf = v.to(DEV).requires_grad_(True)
    faces = f.to(DEV)
    w = torch.tensor([1.0, 0.5, 0.25], device=DEV)

    def step():
        leaf.grad = None
        e, lp, n = L.mesh_shape_priors(Meshes([leaf], [faces]), 0.2)
        total = e * w[0] + lp * w[1] + n * w[2]
        total.backward()
        return e, lp, n

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    leaf.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, pool=torch.cuda.graph_pool_handle()):
        outs = step()
    outs = tuple(o.detach() for o in outs)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in outs] + [leaf.grad.clone()]
    eager = [o.detach() for o in step()] + [leaf.grad]
    torch.cuda.synchronize()
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    del graph, outs


def test_degenerate_face_keeps_the_loss_finite():
    """One zero-area face (three collinear vertices): the losses are finite and match the restatement's values;
    gradients are not compared there (torch's own are of order 1e8)."""
    v, f = fan_mesh()
    v = v.clone()
    v[2] = 0.5 * (v[0] + v[1])  # face (0, 1, 2) collapses onto its edge (0, 1)
    (_, _), (l64, _) = priors_ref([v], [f], 0.0, torch.float32), priors_ref([v], [f], 0.0, torch.float64)
    leaf = v.to(DEV).requires_grad_(True)
    losses = L.mesh_shape_priors(Meshes([leaf], [f.to(DEV)]))
    sum(losses).backward()
    assert all(torch.isfinite(x) for x in losses)
    for nm, a, b in zip(NAMES, losses, l64):
        assert abs(a.item() - b.item()) <= 1e-5 * max(abs(b.item()), 1e-30), (nm, a.item(), b.item())
