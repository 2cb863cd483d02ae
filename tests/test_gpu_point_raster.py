"""The point renderer on the GPU against tests/point_raster_ref.py: the raster boundary (mr_rasterize_points), the
projection and the fragments bitwise; images and gradients against the float64 shadow with the decisions fixed;
background, untouched points, reproducibility, graph capture and the reference-named wrappers. The inputs'
conditioning is asserted on the CPU (tests/test_point_raster_cpu.py)."""
import functools

import pytest
import torch

from tests import point_raster_ref as PR
from tests.helpers import canonical_views, report
from torch_renderer_amd import Pointclouds
from torch_renderer_amd import kernels as Kn
from torch_renderer_amd import points_renderer as PRn
from torch_renderer_amd.cameras import PerspectiveCameras, view_batch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = [(1, 1), (7, 5), (24, 40), (40, 24)]   # no tile multiples, both ways non-square
KMAX = 50


@functools.lru_cache(maxsize=None)
def _boundary():
    return PR.boundary_clouds(Kn.point_raster_chunk())


@functools.lru_cache(maxsize=None)
def _boundary_ref(H, W, rname):
    """The reference at K = 50, computed once: a smaller K keeps its first K slots."""
    pts, first, count = _boundary()
    return PR.rasterize_ref(pts, first, count, H, W, PR.boundary_radii(H, W, pts.shape[0])[rname], KMAX)


def _dev(x):
    return x.to(DEV) if torch.is_tensor(x) else x


def _assert_fragments(got, ref, what):
    for a, b, nm in zip(got, ref, ("idx", "zbuf", "dists")):
        a = a.cpu()
        assert a.shape == b.shape and a.dtype == b.dtype, (what, nm)
        assert torch.equal(a, b), f"{what} {nm}: {(a != b).sum().item()} of {a.numel()} entries differ"


@pytest.mark.parametrize("K", [1, 3, 10, 50])
@pytest.mark.parametrize("H,W", SIZES)
def test_raster_boundary_bitwise(H, W, K):
    pts, first, count = _boundary()
    assert Kn.point_raster_chunk() == 256 and count.tolist() == [0, 1, 255, 256, 257, 513]
    assert (pts[:, 2] < 0).any() and (pts[:, 2] == 0).sum() >= 3 and (pts[:, :2].abs() > 1.7).any()
    for rname, radius in PR.boundary_radii(H, W, pts.shape[0]).items():
        ref = tuple(t[..., :K] for t in _boundary_ref(H, W, rname))
        got = Kn.rasterize_points(pts.to(DEV), first.to(DEV), count.to(DEV), H, W, _dev(radius), K)
        _assert_fragments(got, ref, f"{H}x{W} K={K} r={rname}")
        filled = (ref[0] >= 0).any(-1).float().mean().item()
        if rname == "small" and H * W > 1:
            assert 0.0 < filled < 0.9     # most points hit no centre
        if rname == "big":
            assert (ref[0][1:, ..., 0] >= 0).all()     # every pixel of every non-empty cloud's view


def test_raster_boundary_shared_cloud():
    """One cloud's rows named by 3 views: scanned in place, idx the row or idx_base[n] + the point."""
    pts, first, count = _boundary()
    P = 513
    cloud = pts[first[5]:first[5] + P]
    f3, c3 = torch.zeros(3, dtype=torch.int64), torch.full((3,), P)
    H, W, K = 24, 40, 3
    radius = PR.boundary_radii(H, W, P)["mix"]
    for base in (None, torch.arange(3) * P):
        ref = PR.rasterize_ref(cloud, f3, c3, H, W, radius, K, idx_base=base)
        got = Kn.rasterize_points(cloud.to(DEV), f3.to(DEV), c3.to(DEV), H, W, radius.to(DEV), K,
                                  None if base is None else base.to(DEV))
        _assert_fragments(got, ref, f"shared base={base is not None}")
    assert torch.equal(got[0][1][got[0][1] >= 0] - P, got[0][0][got[0][0] >= 0])


def test_raster_boundary_limits():
    pts, first, count = _boundary()
    with pytest.raises(NotImplementedError):
        Kn.rasterize_points(pts.to(DEV), first.to(DEV), count.to(DEV), 8, 8, 0.1, 51)
    with pytest.raises(NotImplementedError):
        Kn.rasterize_points(pts.to(DEV), first.to(DEV), count.to(DEV), 8, 8, torch.rand(pts.shape[0], device=DEV)
                            .requires_grad_(True), 2)


def test_ties_go_to_the_lowest_index():
    g = torch.Generator().manual_seed(7)
    half = torch.cat([(torch.randint(-6, 7, (300, 2), generator=g).float() / 4.0),
                      torch.randint(0, 4, (300, 1), generator=g).float() * 0.5], 1)   # 4 depth levels, z = 0 included
    pts = torch.cat([half, half[torch.randperm(300, generator=g)]], 0)                # every point twice
    first, count = torch.tensor([0]), torch.tensor([600])
    H, W, K = 24, 40, 10
    ref = PR.rasterize_ref(pts, first, count, H, W, 0.2, K)
    z = ref[1]
    assert ((z[..., 1:] == z[..., :-1]) & (ref[0][..., 1:] >= 0)).float().mean() > 0.3   # ties everywhere
    got = Kn.rasterize_points(pts.to(DEV), first.to(DEV), count.to(DEV), H, W, 0.2, K)
    _assert_fragments(got, ref, "ties")


def test_raster_boundary_backward():
    """grad = (g_dists 2 dx, g_dists 2 dy, g_zbuf) summed over the kept slots: against autograd of the fixed-decision
    values in float64, and bitwise reproducible."""
    case = PR.boundary_backward_case(Kn.point_raster_chunk())
    pts, first, count = case["pts"], case["first"], case["count"]
    grads = []
    for _ in range(2):
        p = pts.to(DEV).requires_grad_(True)
        idx, zbuf, dists = Kn.rasterize_points(p, first.to(DEV), count.to(DEV), PR.BWD_H, PR.BWD_W, case["radius"],
                                               PR.BWD_K)
        ((zbuf * case["gz"].to(DEV)).sum() + (dists * case["gd"].to(DEV)).sum()).backward()
        grads.append(p.grad.cpu())
    assert torch.equal(grads[0], grads[1])
    ref_idx = PR.rasterize_ref(pts, first, count, PR.BWD_H, PR.BWD_W, case["radius"], PR.BWD_K)[0]
    assert torch.equal(idx.cpu(), ref_idx)
    refs = [PR.boundary_backward_ref(case, ref_idx, dt) for dt in (torch.float32, torch.float64)]
    report("raster boundary grad points", grads[0], refs[0], ref64=refs[1])
    untouched = torch.ones(pts.shape[0], dtype=torch.bool)
    untouched[idx.cpu()[idx.cpu() >= 0]] = False
    assert untouched.any() and (grads[0][untouched] == 0).all()


# --------------------------------------------------------------------------- rasterizer / renderer
def _cameras(Kcv, H, W):
    return PerspectiveCameras(focal_length=((float(Kcv[0, 0]), float(Kcv[1, 1])),),
                              principal_point=((float(Kcv[0, 2]), float(Kcv[1, 2])),), in_ndc=False,
                              image_size=torch.tensor([[H, W]]), device=DEV)


@functools.lru_cache(maxsize=None)
def _case(mode, shared, C):
    case = PR.render_case(mode, shared, C)
    idx = PR.case_idx(case)
    return case, idx, PR.render_ref(case, idx, torch.float32), PR.render_ref(case, idx, torch.float64)


def _gpu_render(case, compositor=None, perm=None, radius=PR.RENDER_RADIUS):
    """PointsRenderer on a case: (renderer, clouds, leaves, features, kwargs). perm: an order of the views."""
    H, W = PR.RENDER_H, PR.RENDER_W
    _, _, _, (_, _, Kcv) = canonical_views(torch.cat(case["clouds"], 0), PR.RENDER_N, H, W, dist=1.6)
    cams = _cameras(Kcv, H, W)
    order = list(range(PR.RENDER_N)) if perm is None else perm
    pts = [c.to(DEV).requires_grad_(True) for c in case["clouds"]]
    feats = [f.to(DEV).requires_grad_(True) for f in case["feats"]]
    R = case["R"][order].to(DEV).requires_grad_(True)
    T = case["T"][order].to(DEV).requires_grad_(True)
    if case["shared"]:
        pc, fl = Pointclouds([pts[0]]).extend(PR.RENDER_N), [feats[0]]
    else:
        pc, fl = Pointclouds([pts[i] for i in order]), [feats[i] for i in order]
    rs = PRn.PointsRasterizationSettings(image_size=(H, W), radius=radius, points_per_pixel=PR.RENDER_K)
    comp = compositor or (PRn.AlphaCompositor if case["mode"] == "alpha" else PRn.NormWeightedCompositor)(
        background_color=case["bg"])
    ren = PRn.PointsRenderer(PRn.PointsRasterizer(cams, rs), comp)
    return ren, pc, dict(points=pts, feats=feats, R=R, T=T), fl, dict(R=R, T=T)


def _run(case, perm=None, radius=PR.RENDER_RADIUS):
    ren, pc, leaves, fl, kw = _gpu_render(case, perm=perm, radius=radius)
    img = ren(pc, features=fl, **kw)
    order = list(range(PR.RENDER_N)) if perm is None else perm
    (img * case["wt"][order].to(DEV)).sum().backward()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731
    return (img.detach(), torch.cat([z(p) for p in leaves["points"]], 0), torch.cat([z(f) for f in leaves["feats"]], 0),
            z(leaves["R"]), z(leaves["T"]))


@pytest.mark.parametrize("shared", [True, False])
def test_transform_and_fragments_bitwise(shared):
    case = PR.render_case("alpha", shared, 3)
    ren, pc, leaves, _, kw = _gpu_render(case)
    ras = ren.rasterizer
    intr = view_batch(ras.cameras, (PR.RENDER_H, PR.RENDER_W), kw["R"], kw["T"])[2]
    assert torch.equal(intr.cpu().float(), case["intr"])
    ndc_ref, first, cnt, _ = PR.case_ndc(case)
    ndc = ras.transform(pc, **kw)
    assert ndc.shape == ndc_ref.shape and torch.equal(ndc.detach().cpu(), ndc_ref)
    frag = ras(pc, **kw)
    assert isinstance(frag, PRn.PointFragments)
    _assert_fragments(frag, PR.rasterize_ref(ndc_ref, first, cnt, PR.RENDER_H, PR.RENDER_W, PR.RENDER_RADIUS,
                                             PR.RENDER_K), f"fragments shared={shared}")
    if shared:  # a batch of one cloud under N cameras broadcasts likewise
        one = ras(Pointclouds([leaves["points"][0]]), **kw)
        _assert_fragments(one, [t.cpu() for t in frag], "one cloud under N cameras")


@pytest.mark.parametrize("mode,shared,C", PR.RENDER_CASES)
def test_values_and_gradients(mode, shared, C):
    case, idx, r32, r64 = _case(mode, shared, C)
    ren, pc, _, _, kw = _gpu_render(case)
    assert torch.equal(ren.rasterizer(pc, **kw).idx.cpu(), idx), "the decisions the shadow is given"
    got = _run(case)
    names = ("image", "grad points", "grad features", "grad R", "grad T")
    for nm, g, a, b in zip(names, got, r32, r64):
        report(f"points {mode} shared={shared} C={C} {nm}", g, a, rel_above_one=nm != "image", ref64=b)
    img = got[0].cpu()
    bgpix = idx[..., 0] < 0
    bg = torch.tensor(case["bg"] + ((1.0,) if C == 4 else ()))
    assert bgpix.any() and torch.equal(img[bgpix], bg.expand(int(bgpix.sum()), C))   # exactly the background
    n_points = sum(c.shape[0] for c in case["clouds"])
    seen = torch.zeros(n_points * (PR.RENDER_N if shared else 1), dtype=torch.bool)
    seen[idx[idx >= 0]] = True
    if shared:
        seen = seen.reshape(PR.RENDER_N, n_points).any(0)
    assert (~seen).any()
    assert (got[1].cpu()[~seen] == 0).all() and (got[2].cpu()[~seen] == 0).all()      # exactly zero


@pytest.mark.parametrize("mode,shared,C", [("alpha", True, 3), ("norm", False, 3)])
def test_per_point_radius(mode, shared, C):
    """A radius per point in the settings (a shared cloud's serves every view): decisions bitwise, images and
    gradients against the float64 shadow."""
    case = PR.render_case(mode, shared, C)
    radius, _ = PR.case_radius(case, True)
    idx = PR.case_idx(case, True)
    r32, r64 = (PR.render_ref(case, idx, dt, True) for dt in (torch.float32, torch.float64))
    ren, pc, _, _, kw = _gpu_render(case, radius=radius.to(DEV))
    assert torch.equal(ren.rasterizer(pc, **kw).idx.cpu(), idx)
    got = _run(case, radius=radius.to(DEV))
    for nm, g, a, b in zip(("image", "grad points", "grad features", "grad R", "grad T"), got, r32, r64):
        report(f"per-point radius {mode} shared={shared} {nm}", g, a, rel_above_one=nm != "image", ref64=b)


@pytest.mark.parametrize("mode,shared,C", [("alpha", True, 3), ("norm", False, 3)])
def test_reproducible_and_view_order_independent(mode, shared, C):
    case = PR.render_case(mode, shared, C)
    a, b = _run(case), _run(case)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    perm = [2, 0, 1]
    c = _run(case, perm=perm)
    assert torch.equal(c[0], a[0][perm]) and torch.equal(c[3], a[3][perm]) and torch.equal(c[4], a[4][perm])
    assert torch.equal(c[1], a[1]) and torch.equal(c[2], a[2])   # leaves keep the case's order


def test_graph_capture_replays_the_eager_step():
    case = PR.render_case("alpha", True, 3)
    ren, pc, leaves, fl, kw = _gpu_render(case)
    wt = case["wt"].to(DEV)
    params = [leaves["points"][0], leaves["feats"][0], leaves["R"], leaves["T"]]

    def step():
        img = ren(pc, features=fl, **kw)
        return (img,) + torch.autograd.grad((img * wt).sum(), params)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, pool=torch.cuda.graph_pool_handle()):
        outs = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    got = [o.detach().clone() for o in outs]
    eager = step()
    torch.cuda.synchronize()
    for x, y in zip(got, eager):
        assert torch.equal(x, y.detach())
    del graph, outs


def test_compositor_functions_upstream_layout():
    """alpha_composite / norm_weighted_sum and the compositor modules in upstream's layout: idx / alphas
    (N,K,H,W), features (C,P) -> (N,C,H,W); any C."""
    for C in (1, 5):
        idx, al, f = PR.composite_layout_case(C)
        N, K, H, W = idx.shape
        P = f.shape[1]
        for fn, mode, cls in ((PRn.alpha_composite, "alpha", PRn.AlphaCompositor),
                              (PRn.norm_weighted_sum, "norm", PRn.NormWeightedCompositor)):
            outs = [PR.composite_layout_ref((idx, al, f), mode, dt) for dt in (torch.float32, torch.float64)]
            a, ff = al.to(DEV).requires_grad_(True), f.to(DEV).requires_grad_(True)
            o = fn(idx.to(DEV), a, ff)
            assert o.shape == (N, C, H, W)
            o.square().sum().backward()
            for nm, x, r, r6 in zip(("out", "grad alphas", "grad features"), (o, a.grad, ff.grad), *outs):
                report(f"{mode} C={C} {nm}", x, r, ref64=r6)
            bgc = tuple(0.1 * (i + 1) for i in range(C))
            ob = cls(background_color=bgc)(idx.to(DEV), al.to(DEV), f.to(DEV))
            rb = PR.composite_ref(idx.permute(0, 2, 3, 1), al.permute(0, 2, 3, 1), f.t(), mode, bgc).permute(0, 3, 1, 2)
            report(f"{mode} C={C} background", ob, rb)
    with pytest.raises(ValueError):
        PRn.AlphaCompositor(background_color=(0.1, 0.2))(idx.to(DEV), al.to(DEV), torch.rand(4, P, device=DEV))


@pytest.mark.parametrize("mode", ["alpha", "norm"])
def test_reference_named_wrappers(mode):
    from torch_renderer_amd import torch_renderer as TR
    from torch_renderer_amd.transforms import opencv_to_pytorch3d

    case = PR.render_case(mode, True, 3)
    H, W = PR.RENDER_H, PR.RENDER_W
    _, _, _, (R_cv, t_cv, Kcv) = canonical_views(torch.cat(case["clouds"], 0), PR.RENDER_N, H, W, dist=1.6)
    cls, comp = (TR.AlphaPointRender, PRn.AlphaCompositor) if mode == "alpha" else \
        (TR.NormPointRender, PRn.NormWeightedCompositor)
    r = cls(Kcv.to(DEV), (H, W), radius=0.1, points_per_pixel=4, background_color=case["bg"], device=DEV)
    pc = Pointclouds([case["clouds"][0].to(DEV)]).extend(PR.RENDER_N)
    feats = [case["feats"][0].to(DEV)]
    Rc, tc = R_cv.float().to(DEV), t_cv.float().to(DEV)
    got = r.render(pc, Rc, tc, feats)
    rs = PRn.PointsRasterizationSettings(image_size=(H, W), radius=0.1, points_per_pixel=4)
    ren = PRn.PointsRenderer(PRn.PointsRasterizer(r._cameras, rs), comp(background_color=case["bg"]))
    Rs, ts = opencv_to_pytorch3d(Rc, tc)
    ref = ren(pc, features=feats, R=Rs, T=ts)[..., :3]
    assert got.shape == (PR.RENDER_N, H, W, 3) and torch.equal(got, ref)
    assert (got != torch.tensor(case["bg"], device=DEV)).any()
