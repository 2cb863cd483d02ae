"""Known answers that pin the point renderer's reference (tests/point_raster_ref.py), the Python surface's defaults
and refusals, and the conditioning of every input tests/test_gpu_point_raster.py uses. No GPU."""
import functools

import numpy as np
import pytest
import torch

from tests import point_raster_ref as PR
from tests.helpers import assert_cap
from torch_renderer_amd import Pointclouds
from torch_renderer_amd import points_renderer as PRn
from torch_renderer_amd import torch_renderer as TR


def _one(points, H, W, radius, K=2):
    pts = torch.tensor(points, dtype=torch.float32).reshape(-1, 3)
    return PR.rasterize_ref(pts, [0], [pts.shape[0]], H, W, radius, K)


# --------------------------------------------------------------------------- rasterization known answers
def test_point_on_a_pixel_centre():
    xf, yf = PR.pixel_centres(4, 4)
    assert np.array_equal(xf, np.float32([0.75, 0.25, -0.25, -0.75])) and np.array_equal(yf, xf)
    idx, zbuf, dists = _one([[0.25, -0.75, 1.5]], 4, 4, 0.1)
    assert idx[0, 3, 1, 0] == 0 and dists[0, 3, 1, 0] == 0.0 and zbuf[0, 3, 1, 0] == 1.5
    assert (idx >= 0).sum() == 1


def test_coverage_is_strict():
    # the centre at (0.25, 0.25) is exactly r = 0.5 from the point: d2 == r2 == 0.25, not covered
    idx, _, dists = _one([[0.75, 0.25, 1.0]], 4, 4, 0.5)
    assert idx[0, 1, 1, 0] == -1 and idx[0, 1, 0, 0] == 0
    r = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
    idx, _, dists = _one([[0.75, 0.25, 1.0]], 4, 4, r)
    assert idx[0, 1, 1, 0] == 0 and dists[0, 1, 1, 0] == 0.25


def test_both_axes_are_flipped():
    idx, _, _ = _one([[0.75, 0.75, 1.0]], 4, 4, 0.1)
    assert idx[0, 0, 0, 0] == 0 and (idx >= 0).sum() == 1     # +x, +y in NDC: small xi, small yi


def test_non_square_ranges():
    xf, yf = PR.pixel_centres(2, 4)                            # W > H: x spans +-2
    assert np.array_equal(xf, np.float32([1.5, 0.5, -0.5, -1.5])) and np.array_equal(yf, np.float32([0.5, -0.5]))
    idx, _, _ = _one([[1.5, 0.5, 1.0]], 2, 4, 0.1)
    assert idx[0, 0, 0, 0] == 0
    xf, yf = PR.pixel_centres(4, 2)                            # H > W: y spans +-2
    assert np.array_equal(yf, np.float32([1.5, 0.5, -0.5, -1.5])) and np.array_equal(xf, np.float32([0.5, -0.5]))
    idx, _, _ = _one([[-0.5, -1.5, 1.0]], 4, 2, 0.1)
    assert idx[0, 3, 1, 0] == 0


def test_depth_order_ties_fill_and_negative_z():
    pts = [[0.25, 0.25, 2.0], [0.25, 0.25, 1.0], [0.25, 0.25, 1.0], [0.25, 0.25, -1.0], [0.25, 0.25, 0.5]]
    idx, zbuf, dists = _one(pts, 4, 4, 0.1, K=5)
    assert idx[0, 1, 1].tolist() == [4, 1, 2, 0, -1]          # z ascending, the tie to the lower index, z < 0 skipped
    assert zbuf[0, 1, 1].tolist() == [0.5, 1.0, 1.0, 2.0, -1.0] and dists[0, 1, 1, 4] == -1.0
    idx, _, _ = _one(pts, 4, 4, 0.1, K=2)
    assert idx[0, 1, 1].tolist() == [4, 1]
    # z = 0 and z = -0.0 are drawn and tie; +inf is drawn last; NaN never
    pts = [[0.25, 0.25, float("inf")], [0.25, 0.25, -0.0], [0.25, 0.25, 0.0], [float("nan"), 0.25, 0.1],
           [0.25, 0.25, float("nan")]]
    idx, _, _ = _one(pts, 4, 4, 0.1, K=5)
    assert idx[0, 1, 1].tolist() == [1, 2, 0, -1, -1]


def test_idx_base_and_per_point_radius():
    pts = torch.tensor([[0.25, 0.25, 1.0], [0.25, 0.25, 2.0]])
    idx, _, _ = PR.rasterize_ref(pts, [0, 0], [2, 2], 4, 4, torch.tensor([0.1, 0.0]), 2, idx_base=[0, 2])
    assert idx[0, 1, 1].tolist() == [0, -1] and idx[1, 1, 1].tolist() == [2, -1]


@pytest.mark.parametrize("seed", range(4))
def test_loop_and_vectorised_versions_agree(seed):
    g = torch.Generator().manual_seed(seed)
    counts = [7, 0, 12]
    pts = torch.cat([(torch.rand(sum(counts), 2, generator=g) * 2 - 1) * 1.3,
                     torch.randint(-1, 3, (sum(counts), 1), generator=g).float() * 0.5], 1)
    first = [0, 7, 7]
    radius = [0.3, 0.9, torch.rand(sum(counts), generator=g)][seed % 3]
    for H, W in ((5, 3), (4, 6)):
        a = PR.rasterize_ref(pts, first, counts, H, W, radius, 3)
        b = PR.rasterize_loop(pts, first, counts, H, W, radius, 3)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        # the fixed-decision values restate zbuf / dists bitwise in float32
        z, d = PR.raster_values(pts, a[0], first, H, W)
        assert torch.equal(z, a[1]) and torch.equal(d, a[2])


# --------------------------------------------------------------------------- compositing known answers
def test_compositor_known_answers():
    idx = torch.tensor([0, 1]).reshape(1, 1, 1, 2)
    a = torch.full((1, 1, 1, 2), 0.5)
    f = torch.tensor([[1.0], [0.0]])
    assert PR.composite_ref(idx, a, f, "alpha").item() == 0.5
    assert PR.composite_ref(idx, a, f, "norm").item() == 0.5
    # alpha: the second layer shows through (1 - 0.5)
    assert PR.composite_ref(idx, a, torch.tensor([[0.0], [1.0]]), "alpha").item() == 0.25
    # norm-weighted: a sum of alphas below 1e-4 divides by 1e-4
    tiny = torch.full((1, 1, 1, 2), 1e-5)
    assert PR.composite_ref(idx, tiny, torch.ones(2, 1), "norm").item() == pytest.approx(2e-5 / 1e-4, rel=1e-6)
    # empty slots are skipped
    assert PR.composite_ref(torch.tensor([0, -1]).reshape(1, 1, 1, 2), a, f, "alpha").item() == 0.5


def test_background_rules():
    idx = torch.tensor([[-1, -1], [0, -1], [-1, 0]]).reshape(1, 1, 3, 2)
    a = torch.full((1, 1, 3, 2), 0.5)
    f4 = torch.ones(1, 4)
    out = PR.composite_ref(idx, a, f4, "alpha", background=(0.1, 0.2, 0.3))
    assert out[0, 0, 0].tolist() == pytest.approx([0.1, 0.2, 0.3, 1.0])   # 3 entries, C = 4: alpha 1 appended
    assert out[0, 0, 1].tolist() == [0.5] * 4
    assert out[0, 0, 2].tolist() == pytest.approx([0.1, 0.2, 0.3, 1.0])   # the FIRST slot decides
    assert PR.composite_ref(idx, a, f4, "alpha")[0, 0, 0].tolist() == [0.0] * 4   # no background: zeros
    with pytest.raises(ValueError):
        PR.composite_ref(idx, a, f4, "alpha", background=(0.1, 0.2))
    with pytest.raises(ValueError):
        PRn._background((0.1, 0.2), 4, "cpu")
    assert PRn._background((0.1, 0.2, 0.3), 4, "cpu").tolist() == pytest.approx([0.1, 0.2, 0.3, 1.0])
    assert PRn._background(None, 4, "cpu") is None


@pytest.mark.parametrize("mode", ["alpha", "norm"])
def test_gradcheck_of_the_float64_shadow(mode):
    g = torch.Generator().manual_seed(3)
    pts = torch.cat([(torch.rand(9, 2, generator=g) * 2 - 1), torch.rand(9, 1, generator=g) + 0.5], 1)
    H, W, K, r = 4, 5, 3, 0.7
    idx = PR.rasterize_ref(pts, [0], [9], H, W, r, K)[0]
    assert (idx >= 0).sum() > 20
    p64 = pts.double().requires_grad_(True)
    f64 = torch.rand(9, 2, generator=g).double().requires_grad_(True)

    def fn(p, f):
        z, d = PR.raster_values(p, idx, [0], H, W)
        return PR.composite_ref(idx, PR.alphas_ref(d, idx, r), f, mode, (0.5, 0.25)), z

    assert torch.autograd.gradcheck(fn, (p64, f64), eps=1e-6, atol=1e-6)


def test_projection_gradcheck_and_mesh_parity():
    from oracle import oracle as O

    g = torch.Generator().manual_seed(4)
    X = torch.rand(6, 3, generator=g)
    case = PR.render_case("alpha", True, 3)
    R, T, intr = case["R"], case["T"], case["intr"]
    # a point projects bitwise as a mesh vertex at the same position does
    fv = O.project_faces_torch(X, torch.tensor([[0, 1, 2], [3, 4, 5]]), R, T, intr).reshape(R.shape[0], 6, 3)
    assert torch.equal(PR.project_ref(X, R, T, intr), fv)
    args = (X.double().requires_grad_(True), R.double().requires_grad_(True), T.double().requires_grad_(True))
    assert torch.autograd.gradcheck(lambda x, r, t: PR.project_ref(x, r, t, intr.double()), args, eps=1e-6, atol=1e-6)


# --------------------------------------------------------------------------- the Python surface
def test_constructor_defaults():
    s = PRn.PointsRasterizationSettings()
    assert (s.image_size, s.radius, s.points_per_pixel, s.bin_size, s.max_points_per_bin) == (256, 0.01, 8, None, None)
    assert PRn.PointsRasterizationSettings(image_size=(3, 5)).hw() == (3, 5)
    assert PRn.PointFragments._fields == ("idx", "zbuf", "dists")
    assert PRn.AlphaCompositor().background_color is None and PRn.NormWeightedCompositor().background_color is None
    assert PRn.PointsRasterizer().raster_settings == s
    import inspect

    for cls in (TR.AlphaPointRender, TR.NormPointRender):
        p = inspect.signature(cls.__init__).parameters
        assert (p["radius"].default, p["points_per_pixel"].default, p["background_color"].default) == \
            (0.003, 10, (0, 0, 0))
    K = torch.tensor([[30.0, 0, 16], [0, 30.0, 12], [0, 0, 1]])
    r = TR.AlphaPointRender(K, (24, 32), device="cpu")
    rs = r._renderer.rasterizer.raster_settings
    assert (rs.radius, rs.points_per_pixel, rs.hw()) == (0.003, 10, (24, 32))
    assert isinstance(r._renderer.compositor, PRn.AlphaCompositor)
    assert isinstance(TR.NormPointRender(K, (24, 32), device="cpu")._renderer.compositor, PRn.NormWeightedCompositor)
    import torch_renderer_amd as A
    from torch_renderer_amd import renderer as Rm

    for name in ("PointsRasterizationSettings", "PointsRasterizer", "PointsRenderer", "PointFragments",
                 "AlphaCompositor", "NormWeightedCompositor", "alpha_composite", "norm_weighted_sum"):
        assert getattr(A, name) is getattr(PRn, name) is getattr(Rm, name)


def test_pointclouds_extend():
    p = torch.rand(5, 3)
    pc = Pointclouds([p])
    e = pc.extend(3)
    assert len(e) == 3 and e.is_shared() and not pc.is_shared()
    assert all(q is p for q in e.points_list())
    assert not Pointclouds([p, torch.rand(2, 3)]).extend(2).is_shared()
    with pytest.raises(ValueError):
        pc.extend(0)


def _cpu_renderer(**kw):
    from torch_renderer_amd import PerspectiveCameras

    cams = PerspectiveCameras(focal_length=((2.0, 2.0),), R=torch.eye(3)[None], T=torch.tensor([[0.0, 0.0, 2.0]]))
    rast = PRn.PointsRasterizer(cams, PRn.PointsRasterizationSettings(image_size=8, **kw))
    return rast, PRn.PointsRenderer(rast, PRn.AlphaCompositor())


def test_refusals_without_a_device():
    from torch_renderer_amd import kernels as Kn

    p = torch.rand(5, 3)
    rast, ren = _cpu_renderer()
    with pytest.raises(ValueError, match="features="):
        ren(Pointclouds([p]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # CPU tensors, as elsewhere
        ren(Pointclouds([p]), features=[torch.rand(5, 3)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Kn.rasterize_points(p, torch.tensor([0]), torch.tensor([5]), 8, 8, 0.1, 2)
    with pytest.raises(NotImplementedError):                       # D != 3
        Kn.rasterize_points(torch.rand(5, 2), torch.tensor([0]), torch.tensor([5]), 8, 8, 0.1, 2)
    with pytest.raises(NotImplementedError, match="radius"):       # a per-point radius that requires grad
        Kn._radius_args(torch.rand(5).requires_grad_(True), 5, "rasterize_points")
    with pytest.raises(NotImplementedError, match="radius"):
        _cpu_renderer(radius=torch.rand(5).requires_grad_(True))[1](Pointclouds([p]), features=[torch.rand(5, 3)])
    for k in ("lights", "materials"):
        with pytest.raises(NotImplementedError, match=k):
            rast(Pointclouds([p]), **{k: object()})
    with pytest.raises(NotImplementedError):
        TR.PulsarPointRender(torch.eye(3), (8, 8))
    with pytest.raises(NotImplementedError):                       # unchanged: Pointclouds holds no features
        Pointclouds([p], features=[torch.rand(5, 3)])
    # batch combinations: 2 clouds under 3 cameras
    with pytest.raises(ValueError, match="differ"):
        rast(Pointclouds([p, p.clone()]), R=torch.eye(3)[None].expand(3, 3, 3), T=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="differ"):
        rast(Pointclouds([p]).extend(2), R=torch.eye(3)[None].expand(3, 3, 3), T=torch.zeros(3, 3))
    with pytest.raises(ValueError):
        ren(Pointclouds([p]), features=[torch.rand(4, 3)])         # a feature row per point


# --------------------------------------------------------------------------- conditioning of the GPU file's inputs
@functools.lru_cache(maxsize=None)
def case_runs(mode, shared, C):
    case = PR.render_case(mode, shared, C)
    idx = PR.case_idx(case)
    return case, idx, PR.render_ref(case, idx, torch.float32), PR.render_ref(case, idx, torch.float64)


@pytest.mark.parametrize("mode,shared,C", PR.RENDER_CASES)
def test_render_cases_are_well_conditioned(mode, shared, C):
    case, idx, r32, r64 = case_runs(mode, shared, C)
    filled = idx >= 0
    assert filled.any(dim=-1).float().mean() > 0.1 and (~filled[..., 0]).any()   # drawn and background pixels
    assert filled.all(dim=-1).any() and (filled[..., 0] & ~filled[..., -1]).any()  # full and partly filled lists
    n_points = sum(c.shape[0] for c in case["clouds"])
    seen = torch.zeros(n_points * (PR.RENDER_N if shared else 1), dtype=torch.bool)
    seen[idx[filled]] = True
    if shared:
        seen = seen.reshape(PR.RENDER_N, n_points).any(0)
    assert (~seen).any() and seen.any()                          # points no pixel kept: their gradients must be zero
    for name, a, b in zip(("image", "grad points", "grad features", "grad R", "grad T"), r32, r64):
        assert torch.isfinite(b).all()
        assert_cap(f"{mode} shared={shared} C={C} {name}", a, (a.double() - b).abs().float(),
                   share=name in ("image", "grad points"))
    assert r64[1].abs().max() > 1e-3 and r64[3].abs().max() > 1e-3 and r64[4].abs().max() > 1e-3
    assert (r64[1][~seen] == 0).all() and (r64[2][~seen] == 0).all()


@pytest.mark.parametrize("mode,shared,C", [("alpha", True, 3), ("norm", False, 3)])
def test_per_point_radius_cases_are_well_conditioned(mode, shared, C):
    case = PR.render_case(mode, shared, C)
    radius, packed = PR.case_radius(case, True)
    assert radius.shape[0] == sum(c.shape[0] for c in case["clouds"]) and len(set(radius.tolist())) == 3
    assert packed.shape[0] == radius.shape[0] * (PR.RENDER_N if shared else 1)
    idx = PR.case_idx(case, True)
    assert not torch.equal(idx, PR.case_idx(case))
    r32, r64 = (PR.render_ref(case, idx, dt, True) for dt in (torch.float32, torch.float64))
    for name, a, b in zip(("image", "grad points", "grad features", "grad R", "grad T"), r32, r64):
        assert_cap(f"per-point radius {mode} shared={shared} {name}", a, (a.double() - b).abs().float(),
                   share=name in ("image", "grad points"))


def test_boundary_backward_and_compositor_inputs_are_well_conditioned():
    from torch_renderer_amd import kernels as Kn

    case = PR.boundary_backward_case(Kn.point_raster_chunk())
    assert case["count"].tolist() == [0, 1, 255, 256, 257, 513]
    idx = PR.rasterize_ref(case["pts"], case["first"], case["count"], PR.BWD_H, PR.BWD_W, case["radius"], PR.BWD_K)[0]
    a, b = (PR.boundary_backward_ref(case, idx, dt) for dt in (torch.float32, torch.float64))
    assert_cap("raster boundary grad points", a, (a.double() - b).abs().float())
    for C in (1, 5):
        lay = PR.composite_layout_case(C)
        assert (lay[0][:, 0] < 0).any() and (lay[0] >= 0).any()
        for mode in ("alpha", "norm"):
            r32, r64 = (PR.composite_layout_ref(lay, mode, dt) for dt in (torch.float32, torch.float64))
            for name, x, y in zip(("out", "grad alphas", "grad features"), r32, r64):
                assert_cap(f"{mode} C={C} {name}", x, (x.double() - y).abs().float())
