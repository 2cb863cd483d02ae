"""The fused pose-optimiser loss (torch_renderer_amd.losses.pose_loss, mr_pose_loss_*; SURVEY.md §8f
rank 4) against torch's own nn.L1Loss / HuberLoss(delta=0.05) / MSELoss on CPU, restating
camera_pose_optimizer.py:257-276 calc_loss: the total and its three terms within float32 rounding
of a different summation order (relative 1e-5), and the gradients w.r.t. depth, silhouette and
the RGBA image (through the [..., :3] view the reference passes) within 1e-6 of their scale.
Inputs include exact ties (silhouette == mask: L1's sign(0) = 0) and depth errors at exactly
+-delta (the Huber branch point)."""
import pytest
import torch

from tests.helpers import report
from torch_renderer_amd.losses import pose_loss

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _torch_loss(depth, sil, color, mask, depth_ref, rgb_ref):
    sil_loss = torch.nn.L1Loss()(sil, mask.float())
    color_loss = torch.nn.MSELoss()(color, rgb_ref)
    hloss = torch.nn.HuberLoss(delta=0.05)(torch.masked_select(depth, mask), torch.masked_select(depth_ref, mask))
    return sil_loss + hloss + color_loss * 0.01, (sil_loss, hloss, color_loss)


@pytest.mark.parametrize("shape", [(1, 64, 80), (3, 33, 47)])
@pytest.mark.parametrize("rgba_view", [True, False])
def test_pose_loss_matches_torch(shape, rgba_view):
    g = torch.Generator().manual_seed(7)
    depth = torch.rand(shape, generator=g) * 2
    depth_ref = depth + (torch.rand(shape, generator=g) - 0.5) * 0.2
    flat_d, flat_r = depth.view(-1), depth_ref.view(-1)
    flat_r[:5] = flat_d[:5] + 0.05   # exactly at the Huber branch point (in f32 arithmetic)
    flat_r[5:10] = flat_d[5:10]      # zero error
    mask = torch.rand(shape, generator=g) > 0.4
    sil = torch.rand(shape, generator=g)
    sil.view(-1)[:20] = mask.view(-1)[:20].float()  # exact ties: sign(0) = 0
    rgba = torch.rand(shape + (4,), generator=g)
    rgb_ref = torch.rand(shape + (3,), generator=g)
    # torch reference on CPU
    dr_, sr_, ir_ = (t.clone().requires_grad_(True) for t in (depth, sil, rgba))
    tot_r, terms_r = _torch_loss(dr_, sr_, ir_[..., :3], mask, depth_ref, rgb_ref)
    tot_r.backward()
    # fused on the GPU
    dg, sg, ig = (t.to(DEV).requires_grad_(True) for t in (depth, sil, rgba))
    color = ig[..., :3] if rgba_view else ig[..., :3].contiguous()
    tot, terms = pose_loss(dg, sg, color, mask.to(DEV), depth_ref.to(DEV), rgb_ref.to(DEV), return_terms=True)
    tot.backward()
    for name, a, b in (("total", tot, tot_r), ("sil", terms[0], terms_r[0]), ("huber", terms[1], terms_r[1]),
                       ("mse", terms[2], terms_r[2])):
        a, b = float(a.detach()), float(b.detach())
        print(f"[parity] pose_loss {name}: {a:.9g} vs torch {b:.9g}")
        assert abs(a - b) <= 1e-5 * max(abs(b), 1e-6), name
    report("pose_loss grad depth", dg.grad, dr_.grad, tol=1e-6)
    report("pose_loss grad sil", sg.grad, sr_.grad, tol=1e-6)
    report("pose_loss grad rgba", ig.grad, ir_.grad, tol=1e-6)


def test_pose_loss_deterministic_and_empty_mask():
    g = torch.Generator().manual_seed(3)
    shape = (2, 50, 60)
    args = [torch.rand(shape, generator=g).to(DEV), torch.rand(shape, generator=g).to(DEV),
            torch.rand(shape + (3,), generator=g).to(DEV), (torch.rand(shape, generator=g) > 0.5).to(DEV),
            torch.rand(shape, generator=g).to(DEV), torch.rand(shape + (3,), generator=g).to(DEV)]
    a = pose_loss(*args)
    b = pose_loss(*args)
    assert torch.equal(a, b)
    args[3] = torch.zeros(shape, dtype=torch.bool, device=DEV)
    assert torch.isnan(pose_loss(*args))  # torch: mean over an empty selection


@pytest.mark.parametrize("shape", [(2, 64, 80), (3, 33, 47)])
def test_pose_loss_upstream_scale_and_second_backward(shape):
    """The forward writes the gradients for dL/dtotal = 1 (mr_pose_loss_forward_grad, one pass; the
    (2, 64, 80) case is the vectorised kernel, (3, 33, 47) the two-pass fallback); a backward with
    another upstream rescales them (mr_pose_loss_scale), and a second backward over a retained graph
    recomputes them from the saved inputs: both against torch."""
    g = torch.Generator().manual_seed(11)
    depth = torch.rand(shape, generator=g) * 2
    depth_ref = depth + (torch.rand(shape, generator=g) - 0.5) * 0.2
    mask = torch.rand(shape, generator=g) > 0.4
    sil = torch.rand(shape + (4,), generator=g)
    rgba = torch.rand(shape + (4,), generator=g)
    rgb_ref = torch.rand(shape + (3,), generator=g)
    dr_, sr_, ir_ = (t.clone().requires_grad_(True) for t in (depth, sil, rgba))
    tot_r, _ = _torch_loss(dr_, sr_[..., 3], ir_[..., :3], mask, depth_ref, rgb_ref)
    (2.5 * tot_r).backward()
    dg, sg, ig = (t.to(DEV).requires_grad_(True) for t in (depth, sil, rgba))
    tot = pose_loss(dg, sg[..., 3], ig[..., :3], mask.to(DEV), depth_ref.to(DEV), rgb_ref.to(DEV))
    (2.5 * tot).backward(retain_graph=True)
    report("pose_loss x2.5 grad depth", dg.grad, dr_.grad, tol=1e-6)
    report("pose_loss x2.5 grad sil image", sg.grad, sr_.grad, tol=1e-6)
    report("pose_loss x2.5 grad rgba", ig.grad, ir_.grad, tol=1e-6)
    g1 = [t.grad.clone() for t in (dg, sg, ig)]
    tot.backward()  # second backward, upstream 1: the slow path from the saved inputs
    for a, b, name in zip((dg.grad, sg.grad, ig.grad), g1, ("depth", "sil", "rgba")):
        report(f"pose_loss second backward {name}", a - b, b / 2.5, tol=1e-6)


# Above k_pose_loss_final's first pass: the final reduction sums the nb = ceil(npix / 1024) per-workgroup
# partials 4096 per pass, four per thread (lanes u = 0..3 at i0 + u * 1024, guarded by i0 + u * 1024 < nb).
#   (17, 512, 512): npix = 4,456,448, nb = 4352 > 4096: a second pass whose u >= 1 lanes are all guarded off;
#   (5, 511, 512):  npix = 1,308,160 = 1277.5 * 1024, nb = 1278: the u = 1 lanes partly guarded, a ragged
#                   last workgroup (npix % 1024 = 512).
BIG_SHAPES = [(17, 512, 512), (5, 511, 512)]


def _big_inputs(shape, seed=5):
    g = torch.Generator().manual_seed(seed)
    depth = torch.rand(shape, generator=g) * 2
    depth_ref = depth + (torch.rand(shape, generator=g) - 0.5) * 0.2
    flat_d, flat_r = depth.view(-1), depth_ref.view(-1)
    flat_r[:5] = flat_d[:5] + 0.05     # at the Huber branch point, either side
    flat_r[5:10] = flat_d[5:10] - 0.05
    flat_r[10:15] = flat_d[10:15]      # zero error
    mask = torch.rand(shape, generator=g) > 0.4
    mask.view(-1)[:15] = True
    sil4 = torch.rand(shape + (4,), generator=g)
    sil4.view(-1, 4)[:20, 3] = mask.view(-1)[:20].float()  # exact ties: sign(0) = 0
    rgba = torch.rand(shape + (4,), generator=g)
    rgb_ref = torch.rand(shape + (3,), generator=g)
    return depth, depth_ref, mask, sil4, rgba, rgb_ref


@pytest.mark.parametrize("shape", BIG_SHAPES)
@pytest.mark.parametrize("rgba_view", [True, False])
def test_pose_loss_above_one_reduction_pass(shape, rgba_view):
    """The loss over more workgroup partials than one thread-pass of k_pose_loss_final takes, against
    the same three torch losses in float64 on the CPU: total and terms within 1e-5 relative. The
    gradients are ~1 / npix ~ 2e-7, below this file's absolute 1e-6, so the backward runs through
    npix * total (k_pose_loss_scale's grid-stride loops) and the O(1) gradients are held to 1e-6 *
    max(1, |ref|); a second backward with upstream 1 (k_pose_loss_bwd from the saved inputs) is
    compared the same way after scaling by npix."""
    depth, depth_ref, mask, sil4, rgba, rgb_ref = _big_inputs(shape)
    npix = depth.numel()
    nb = -(-npix // 1024)
    assert (nb > 4096) if shape[0] == 17 else (1024 < nb < 4096 and npix % 1024 != 0)
    if rgba_view:
        sil_src, col_src = sil4, rgba
        view_s, view_c = (lambda t: t[..., 3]), (lambda t: t[..., :3])
    else:
        sil_src, col_src = sil4[..., 3].contiguous(), rgba[..., :3].contiguous()
        view_s = view_c = lambda t: t  # noqa: E731
    # float64 reference
    dr_, sr_, ir_ = (t.double().requires_grad_(True) for t in (depth, sil_src, col_src))
    tot_r, terms_r = _torch_loss(dr_, view_s(sr_), view_c(ir_), mask, depth_ref.double(), rgb_ref.double())
    (npix * tot_r).backward()
    refs = [t.grad for t in (dr_, sr_, ir_)]
    assert max(float(r.abs().max()) for r in refs) > 0.5  # O(1) once scaled by npix
    # fused on the GPU
    dg, sg, ig = (t.to(DEV).requires_grad_(True) for t in (depth, sil_src, col_src))
    tot, terms = pose_loss(dg, view_s(sg), view_c(ig), mask.to(DEV), depth_ref.to(DEV), rgb_ref.to(DEV),
                           return_terms=True)
    for name, a, b in (("total", tot, tot_r), ("sil", terms[0], terms_r[0]), ("huber", terms[1], terms_r[1]),
                       ("mse", terms[2], terms_r[2])):
        a, b = float(a.detach()), float(b.detach())
        print(f"[parity] pose_loss {shape} {name}: {a:.9g} vs torch f64 {b:.9g} (rel {abs(a - b) / abs(b):.2e})")
        assert abs(a - b) <= 1e-5 * max(abs(b), 1e-6), name
    (npix * tot).backward(retain_graph=True)
    names = ("depth", "sil", "rgba" if rgba_view else "rgb")
    for nm, leaf, r in zip(names, (dg, sg, ig), refs):
        report(f"pose_loss {shape} x npix grad {nm}", leaf.grad, r, tol=1e-6)
        leaf.grad = None
    tot.backward()  # second backward, upstream 1: recomputed from the saved inputs
    for nm, leaf, r in zip(names, (dg, sg, ig), refs):
        report(f"pose_loss {shape} second backward x npix grad {nm}", leaf.grad * float(npix), r, tol=1e-6)


def test_pose_loss_above_one_reduction_pass_deterministic_and_empty_mask():
    depth, depth_ref, mask, sil4, rgba, rgb_ref = (t.to(DEV) for t in _big_inputs(BIG_SHAPES[0], seed=6))
    args = [depth, sil4[..., 3], rgba[..., :3], mask, depth_ref, rgb_ref]
    a, ta = pose_loss(*args, return_terms=True)
    b, tb = pose_loss(*args, return_terms=True)
    assert torch.isfinite(a) and torch.equal(a, b)
    assert all(torch.equal(x, y) for x, y in zip(ta, tb))
    args[3] = torch.zeros_like(mask)
    assert torch.isnan(pose_loss(*args))  # torch: mean over an empty selection
