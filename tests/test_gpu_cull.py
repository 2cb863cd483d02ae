"""RasterizationSettings.cull_backfaces on every path that reads it, against the oracle's cull (itself
pinned without the flag by tests/test_oracle.py::test_cull_backfaces_equals_rasterizing_the_front_faces_only):
the modular rasterizer from world vertices (RasterizeMeshesWorld) and from face_verts (mr_rasterize_meshes),
their backward (with the clipped backward's recomputation of the near-plane sub-triangles), the fused
one-launch render (ShadeConfig.cull; per-view and count -> scan binning) and the fused soft silhouette
(SoftSilhouetteWorld). Fragments bitwise; images and gradients within tests.helpers.report's bar.

Meshes: the jittered level-2 ico-sphere (tests.helpers.jittered_ico) and the same with the winding flipped
— one front and one back layer per pixel, so culling removes about half of the K-deep fragments and, on the
flipped mesh, changes every nearest face — and the cow cut open by the near plane (tests/test_gpu_clip.py),
whose interior is back faces. Every test first asserts, from the oracle alone, that culling changes its
input by the stated margin (a kernel ignoring the flag then fails), and every rendering test that the f32
oracle's own spread stays within tests.helpers.assert_cap."""
import functools
import math

import pytest
import torch

from oracle import oracle as O
from tests.helpers import assert_cap, canonical_views, jittered_ico, mesh_arrays, oracle_runs, report
from torch_renderer_amd import Meshes, TexturesVertex
from torch_renderer_amd.cameras import FoVPerspectiveCameras, PerspectiveCameras
from torch_renderer_amd.mesh_renderer import (BlendParams, MeshRasterizer, MeshRenderer, PointLights,
                                              RasterizationSettings, SoftPhongShader, SoftSilhouetteShader)
from torch_renderer_amd.transforms import look_at_view_transform

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FOV_T = 1.0 / math.tan(math.radians(30.0))
BLUR = math.log(1.0 / 1e-4 - 1.0) * 1e-4
LIGHT_LOC = (0.5, 1.0, -2.0)

# name: (flip, H, W, N, K, blur, focal length in px or None for the 60 degree field of view)
ICO = {
    "ico2_K4": (False, 40, 56, 2, 4, 2e-4, None),
    "ico2_K8": (False, 32, 32, 2, 8, BLUR, None),
    "flip_K1": (True, 64, 64, 2, 1, 0.0, None),
    "flip_wide": (True, 16, 2052, 1, 1, 0.0, 32.0),  # 257 x 2 tiles: wider than the per-view binning takes
}


def _camera(Kc, H, W, device, **kw):
    return PerspectiveCameras(focal_length=((Kc[0, 0].item(), Kc[1, 1].item()),),
                              principal_point=((Kc[0, 2].item(), Kc[1, 2].item()),), in_ndc=False,
                              image_size=torch.tensor([[H, W]]), device=device, **kw)


@functools.lru_cache(maxsize=None)
def _ico(name):
    """(verts, faces, R, T, Kc, intr) of an ICO case on the CPU (never modified). intr is the camera's own
    NDC affine, so both sides rasterize bitwise the same projected vertices."""
    flip, H, W, N, K, blur, focal = ICO[name]
    verts, faces = jittered_ico(2, flip)
    fov = 60.0 if focal is None else math.degrees(2.0 * math.atan((W / 2.0) / focal))
    R, T, _, (_, _, Kc) = canonical_views(verts, N, H, W, fov_deg=fov)
    intr = _camera(Kc, H, W, "cpu").ndc_affine((H, W)).expand(N, 4).contiguous()
    return verts, faces, R, T, Kc, intr


def _packed(N, Fn):
    return torch.arange(N) * Fn, torch.full((N,), Fn)


@functools.lru_cache(maxsize=None)
def _ico_fragments(name, cull):
    """The oracle's (pix_to_face, zbuf, bary, dists) of an ICO case (never modified)."""
    flip, H, W, N, K, blur, _ = ICO[name]
    verts, faces, R, T, _, intr = _ico(name)
    fv = O.project_faces_torch(verts, faces, R, T, intr)
    return O.raster_fwd(fv, *_packed(N, faces.shape[0]), H, W, K, blur, True, blur > 0, cull)


def _culling_matters(tag, off, on):
    """The precondition, from the oracle's pix_to_face without / with culling. K > 1: the filled (pixel, k)
    slots drop by >= 25 %. K = 1 on a closed mesh: the nearest face differs on >= half of >= 100 covered
    pixels (there culling cannot empty a pixel, it shows the far side instead)."""
    if off.shape[-1] > 1:
        a, b = int((off >= 0).sum()), int((on >= 0).sum())
        print(f"[cull] {tag}: {a} -> {b} filled slots")
        assert b >= 100 and b <= 0.75 * a, (tag, a, b)
    else:
        cov = off[..., 0] >= 0
        ch = cov & (off[..., 0] != on[..., 0])
        print(f"[cull] {tag}: {int(ch.sum())} of {int(cov.sum())} covered pixels change")
        assert int(cov.sum()) >= 100 and 2 * int(ch.sum()) >= int(cov.sum()), (tag, int(ch.sum()), int(cov.sum()))


def _removes(tag, off, on):
    """The cut cow's precondition: culling removes >= 25 % of the filled slots (K = 1: of the covered pixels
    — the cut shows the interior, which is back faces) and leaves >= 100."""
    a, b = int((off >= 0).sum()), int((on >= 0).sum())
    print(f"[cull] {tag}: {a} -> {b} filled slots")
    assert b >= 100 and b <= 0.75 * a, (tag, a, b)


def _bitwise(tag, got, ref):
    assert torch.equal(got[0].cpu(), ref[0]), f"{tag}: pix_to_face"
    for a, b, nm in zip(got[1:], ref[1:], ("zbuf", "bary", "dists")):
        assert torch.equal(a.detach().cpu().view(torch.int32), b.detach().view(torch.int32)), f"{tag}: {nm} not bitwise"


def _zero_rows_stay_zero(tag, got, ref, at_least):
    """No fragment of a culled face may leak a contribution: every vertex row that is exactly zero in the
    oracle's gradient is exactly zero on the GPU."""
    z = (ref == 0).all(1)
    print(f"[cull] {tag}: {int(z.sum())} of {ref.shape[0]} gradient rows are zero in the oracle")
    assert int(z.sum()) >= at_least, (tag, int(z.sum()))
    leaked = (got.detach().cpu()[z] != 0).any(1)
    assert not bool(leaked.any()), f"{tag}: {int(leaked.sum())} rows the oracle leaves at zero got a gradient"


def _upstream(shapes, seed=5):
    """Random upstream gradients on zbuf / bary / dists (tests/test_gpu_clip.py)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shapes[0], generator=g), torch.rand(shapes[1], generator=g) - 0.5,
            torch.rand(shapes[2], generator=g) * 1e-3)


# ------------------------------------------------------------------------------------------ (a) fragments
@pytest.mark.parametrize("name", ["ico2_K4", "ico2_K8", "flip_K1"])
def test_culled_fragments_bitwise(name):
    """World path (MeshRasterizer) and face_verts path (rasterize_meshes_fwd) with cull on AND off against the
    oracle's: a flag wired backwards, ignored, or culling the wrong winding cannot pass both."""
    from torch_renderer_amd.kernels import rasterize_meshes_fwd

    flip, H, W, N, K, blur, _ = ICO[name]
    verts, faces, R, T, Kc, intr = _ico(name)
    _culling_matters(name, _ico_fragments(name, False)[0], _ico_fragments(name, True)[0])
    cams = _camera(Kc, H, W, DEV, R=R.to(DEV), T=T.to(DEV))
    fv = O.project_faces_torch(verts, faces, R, T, intr).to(DEV)
    first, count = (t.to(DEV) for t in _packed(N, faces.shape[0]))
    for cull in (True, False):
        ref = _ico_fragments(name, cull)
        rs = RasterizationSettings(image_size=(H, W), blur_radius=blur, faces_per_pixel=K, cull_backfaces=cull)
        fr = MeshRasterizer(cams, rs)(Meshes([verts.to(DEV)], [faces.to(DEV)]).extend(N))
        _bitwise(f"{name} cull={cull} world", (fr.pix_to_face, fr.zbuf, fr.bary_coords, fr.dists), ref)
        got = rasterize_meshes_fwd(fv, first, count, H, W, K, blur, True, blur > 0, cull=cull)
        _bitwise(f"{name} cull={cull} face_verts", got, ref)


# ------------------------------------------------------------------------------------------ (b) backward
@pytest.mark.parametrize("name", ["ico2_K4", "flip_K1"])
def test_culled_fragments_backward(name):
    flip, H, W, N, K, blur, _ = ICO[name]
    verts, faces, R, T, Kc, intr = _ico(name)
    _culling_matters(name, _ico_fragments(name, False)[0], _ico_fragments(name, True)[0])
    vr = verts.clone().requires_grad_(True)
    Rr, Tr = R.clone().requires_grad_(True), T.clone().requires_grad_(True)
    fv = O.project_faces_torch(vr, faces, Rr, Tr, intr)
    p2f, zbuf, bary, dists = O.RasterizeRef.apply(fv, *_packed(N, faces.shape[0]), H, W, K, blur, True, blur > 0,
                                                  True)
    gz, gb, gd = _upstream((zbuf.shape, bary.shape, dists.shape))
    ((zbuf * gz).sum() + (bary * gb).sum() + (dists * gd).sum()).backward()
    cams = _camera(Kc, H, W, DEV)
    rs = RasterizationSettings(image_size=(H, W), blur_radius=blur, faces_per_pixel=K, cull_backfaces=True)
    vg = verts.to(DEV).requires_grad_(True)
    Rg, Tg = R.to(DEV).requires_grad_(True), T.to(DEV).requires_grad_(True)
    fr = MeshRasterizer(cams, rs)(meshes_world=Meshes([vg], [faces.to(DEV)]).extend(N), R=Rg, T=Tg)
    assert torch.equal(fr.pix_to_face.cpu(), p2f)
    ((fr.zbuf * gz.to(DEV)).sum() + (fr.bary_coords * gb.to(DEV)).sum() + (fr.dists * gd.to(DEV)).sum()).backward()
    report(f"cull {name} grad verts", vg.grad, vr.grad)
    report(f"cull {name} grad R", Rg.grad, Rr.grad)
    report(f"cull {name} grad T", Tg.grad, Tr.grad)


def test_culled_rasterize_meshes_bwd_direct():
    """rasterize_meshes_bwd(..., cull=True) on the oracle's own culled fragments against RasterizeRef's
    backward (orc_raster_bwd), per face_verts entry."""
    from torch_renderer_amd.kernels import rasterize_meshes_bwd

    name = "ico2_K4"
    flip, H, W, N, K, blur, _ = ICO[name]
    verts, faces, R, T, _, intr = _ico(name)
    _culling_matters(name, _ico_fragments(name, False)[0], _ico_fragments(name, True)[0])
    p2f, zbuf, bary, dists = _ico_fragments(name, True)
    fv = O.project_faces_torch(verts, faces, R, T, intr)
    gz, gb, gd = _upstream((zbuf.shape, bary.shape, dists.shape), seed=6)
    ref = O.raster_bwd(fv, p2f, gz, gb, gd, True, True)
    got = rasterize_meshes_bwd(fv.to(DEV), p2f.to(DEV), gz.to(DEV), gb.to(DEV), gd.to(DEV), H, W, K, True, True, blur,
                               cull=True)
    assert (ref != 0).any(-1).any(-1).sum() > 100
    report("cull rasterize_meshes_bwd grad face_verts", got, ref)


# ------------------------------------------------------------------------------------------ (c) near-plane clipping
def _cow_poses(N, dist):
    return look_at_view_transform(dist, torch.linspace(-10.0, 35.0, N), torch.linspace(0.0, 300.0, N))


@pytest.mark.parametrize("K,blur", [(1, 0.0), (3, 2e-4)])
def test_culled_clipped_fragments_match_oracle(K, blur):
    """The cut cow of tests/test_gpu_clip.py with cull_backfaces: the forward culls the clipped sub-triangles
    with their face, and the clipped backward recomputes the same ones."""
    H, W, N = 96, 96, 3
    verts, faces, _ = mesh_arrays("cow")
    R, T = _cow_poses(N, 0.52)
    intr = torch.tensor([[FOV_T, 0.0, FOV_T, 0.0]]).expand(N, 4)
    vr = verts.clone().requires_grad_(True)
    Rr, Tr = R.clone().requires_grad_(True), T.clone().requires_grad_(True)
    fv = O.project_faces_torch(vr, faces, Rr, Tr, intr)
    cf = O.clip_faces_ref(fv, *_packed(N, faces.shape[0]), 0.5, persp=True)
    assert int((cf["neighbor"] >= 0).sum()) > 50, "the views must cut the mesh with the near plane"
    pair_mode = 1 if (K > 1 and blur > 0) else 0  # one candidate per split face, as the kernels (test_gpu_clip.py)
    off = O.raster_fwd(cf["face_verts"], cf["first"], cf["count"], H, W, K, blur, True, blur > 0, False,
                       cf["neighbor"], None, pair_mode)[0]
    p2f_c, zbuf, bary_c, dists = O.RasterizeRef.apply(cf["face_verts"], cf["first"], cf["count"], H, W, K, blur,
                                                      True, blur > 0, True, cf["neighbor"], None, pair_mode)
    _removes(f"cut cow K={K}", off, p2f_c)
    p2f, bary = O.unclip_fragments(p2f_c, bary_c, cf)
    split = torch.zeros(cf["neighbor"].shape[0] + 1, dtype=torch.bool)
    split[:-1] = cf["neighbor"] >= 0
    print(f"[cull] cut cow K={K}: {int(split[p2f_c].sum())} fragments of clipped sub-triangles after culling")
    assert int(split[p2f_c].sum()) > 0, "clipped sub-triangles must survive the culling"
    cams = FoVPerspectiveCameras(device=DEV)
    rs = RasterizationSettings(image_size=(H, W), blur_radius=blur, faces_per_pixel=K, cull_backfaces=True)
    vg = verts.to(DEV).requires_grad_(True)
    Rg, Tg = R.to(DEV).requires_grad_(True), T.to(DEV).requires_grad_(True)
    fr = MeshRasterizer(cams, rs)(meshes_world=Meshes([vg], [faces.to(DEV)]).extend(N), R=Rg, T=Tg)
    _bitwise(f"cut cow K={K} cull", (fr.pix_to_face, fr.zbuf, fr.bary_coords, fr.dists), (p2f, zbuf, bary, dists))
    gz, gb, gd = _upstream((zbuf.shape, bary.shape, dists.shape))
    ((fr.zbuf * gz.to(DEV)).sum() + (fr.bary_coords * gb.to(DEV)).sum() + (fr.dists * gd.to(DEV)).sum()).backward()
    ((zbuf * gz).sum() + (bary * gb).sum() + (dists * gd).sum()).backward()
    report(f"cull clip K={K} grad verts", vg.grad, vr.grad)
    report(f"cull clip K={K} grad R", Rg.grad, Rr.grad)
    report(f"cull clip K={K} grad T", Tg.grad, Tr.grad)


# ------------------------------------------------------------------------------------------ (d, e, f) renders
NAMES = ("image", "grad verts", "grad R", "grad T")


def _oracle_render(tag, verts, faces, R, T, intr, H, W, shader, go, **kw):
    """oracle_runs of render_ref(cull=True) + backward of (image * go).sum(): (ref, ref64, spread), each
    (image, grad verts, grad R, grad T); with the cap on the oracle's own spread asserted here, before any
    GPU output exists."""
    def run(precision):
        vr = verts.clone().requires_grad_(True)
        Rr, Tr = R.clone().requires_grad_(True), T.clone().requires_grad_(True)
        ref = O.render_ref(vr, faces, Rr, Tr, intr, H, W, cull=True, precision=precision, **kw)
        img = ref["rgba"] if shader == "phong" else ref["sil"]
        gg = go.to(img.dtype)
        (img * (gg if shader == "phong" else gg[..., 3])).sum().backward()
        return img, vr.grad, Rr.grad, Tr.grad

    runs = oracle_runs(run)
    for i, nm in enumerate(NAMES):
        assert_cap(f"{tag} {nm}", runs[0][i], runs[2][i], share=i < 2)
    return runs


def _check_render(tag, shader, out, leaves, go, runs, zero_rows):
    """Image and grad verts / R / T by report, then the zero rows."""
    ref, r64, sp = runs
    names = NAMES
    report(f"{tag} image", out if shader == "phong" else out[..., 3], ref[0], ref64=r64[0], sens=sp[0])
    (out * go.to(DEV)).sum().backward()
    for i, leaf in enumerate(leaves):
        report(f"{tag} {names[i + 1]}", leaf.grad, ref[i + 1], ref64=r64[i + 1], sens=sp[i + 1])
    _zero_rows_stay_zero(tag, leaves[0].grad, ref[1], zero_rows)


@functools.lru_cache(maxsize=None)
def _vcol(V):
    return torch.rand((V, 3), generator=torch.Generator().manual_seed(11))


def _shader(shader, cams, blend):
    if shader == "phong":
        return SoftPhongShader(device=DEV, cameras=cams, lights=PointLights(device=DEV, location=[LIGHT_LOC]),
                               blend_params=blend)
    return SoftSilhouetteShader(blend_params=blend)


def _fused_ico(name, shader):
    """MeshRenderer (one fused launch: K = 1, blur = 0) of an ICO case with cull_backfaces, R / T per call (the
    specular camera centre is the camera object's own: the origin)."""
    flip, H, W, N, K, blur, _ = ICO[name]
    assert K == 1 and blur == 0.0
    verts, faces, R, T, Kc, intr = _ico(name)
    _culling_matters(name, _ico_fragments(name, False)[0], _ico_fragments(name, True)[0])
    vcol = _vcol(verts.shape[0])
    go = torch.rand(N, H, W, 4, generator=torch.Generator().manual_seed(9)) - 0.5
    light = dict(O.DEFAULT_LIGHT, location=LIGHT_LOC)
    runs = _oracle_render(f"cull fused {name} {shader}", verts, faces, R, T, intr, H, W, shader, go,
                          texture=("vertex", vcol), light=light, bg=(0.2, 0.3, 0.4))
    cams = _camera(Kc, H, W, DEV)
    blend = BlendParams(sigma=1e-4, gamma=1e-4, background_color=(0.2, 0.3, 0.4))
    rs = RasterizationSettings(image_size=(H, W), cull_backfaces=True)
    renderer = MeshRenderer(MeshRasterizer(cams, rs), _shader(shader, cams, blend))
    vg = verts.to(DEV).requires_grad_(True)
    Rg, Tg = R.to(DEV).requires_grad_(True), T.to(DEV).requires_grad_(True)
    out = renderer(meshes_world=Meshes([vg], [faces.to(DEV)], TexturesVertex([vcol.to(DEV)])).extend(N), R=Rg, T=Tg)
    # two views from opposite sides leave few vertices without any gradient (7 with Phong, whose vertex normals
    # spread it to the neighbours, 19 for the silhouette); the single wide view leaves half of them
    _check_render(f"cull fused {name} {shader}", shader, out, (vg, Rg, Tg), go, runs, zero_rows=5 if N > 1 else 20)


@pytest.mark.parametrize("shader", ["phong", "silhouette"])
def test_fused_render_culled_flipped_sphere(shader):
    _fused_ico("flip_K1", shader)


def test_fused_render_culled_count_scan_binning():
    """(e) One 16 x 2052 view (focal length 32 px, tests/test_gpu_api.py): too wide for the per-view binning, so
    the flag is read by the count -> scan path's record builder."""
    from torch_renderer_amd import _lib

    flip, H, W, N, _, _, _ = ICO["flip_wide"]
    assert _lib.load().mr_per_view_binning(N, N * _ico("flip_wide")[1].shape[0], H, W) == 0
    _fused_ico("flip_wide", "phong")


@pytest.mark.parametrize("shader", ["phong", "silhouette"])
def test_fused_render_culled_clipped_cow(shader):
    """The cut cow of test_fused_renderer_clipped_matches_oracle (128 x 128: at 96 x 96 only 124 pixels stay
    covered) with cull_backfaces: the interior the cut shows is gone, and with it most vertices' gradient.
    Vertex colours, not that test's UV map: with the map the f32 oracle's own spread on the vertex gradient is
    57 x the bar here (cap 10: tests.helpers.assert_cap), with vertex colours 1.6 x."""
    H, W, N = 128, 128, 2
    verts, faces, _ = mesh_arrays("cow")
    R, T = _cow_poses(N, 0.5)
    intr = torch.tensor([[FOV_T, 0.0, FOV_T, 0.0]]).expand(N, 4).contiguous()
    vcol = _vcol(verts.shape[0])
    off = O.render_ref(verts, faces, R, T, intr, H, W, z_clip=0.5)["p2f"]
    on = O.render_ref(verts, faces, R, T, intr, H, W, z_clip=0.5, cull=True)["p2f"]
    _removes("fused cut cow", off, on)
    go = torch.rand(N, H, W, 4, generator=torch.Generator().manual_seed(9)) - 0.5
    runs = _oracle_render(f"cull fused cut cow {shader}", verts, faces, R, T, intr, H, W, shader, go,
                          texture=("vertex", vcol), bg=(0.0, 0.0, 0.0), z_clip=0.5)
    cams = FoVPerspectiveCameras(device=DEV)
    blend = BlendParams(sigma=1e-4, gamma=1e-4, background_color=(0.0, 0.0, 0.0))
    sh = (SoftPhongShader(device=DEV, cameras=cams, lights=PointLights(device=DEV, location=[[0.0, 0.0, -3.0]]),
                          blend_params=blend) if shader == "phong" else SoftSilhouetteShader(blend_params=blend))
    renderer = MeshRenderer(MeshRasterizer(cams, RasterizationSettings(image_size=(H, W), cull_backfaces=True)), sh)
    tex = TexturesVertex([vcol.to(DEV)])
    vg = verts.to(DEV).requires_grad_(True)
    Rg, Tg = R.to(DEV).requires_grad_(True), T.to(DEV).requires_grad_(True)
    out = renderer(meshes_world=Meshes([vg], [faces.to(DEV)], tex).extend(N), R=Rg, T=Tg)
    _check_render(f"cull fused cut cow {shader}", shader, out, (vg, Rg, Tg), go, runs, zero_rows=verts.shape[0] // 2)


def test_fused_soft_silhouette_culled():
    """(f) SoftSilhouetteWorld (MeshRenderer + SoftSilhouetteShader, K = 8) with cull_backfaces: alpha and
    gradients against the oracle, the zero rows, and bitwise the two-step path (tests/test_gpu_soft_fused.py)."""
    name = "ico2_K8"
    flip, H, W, N, K, blur, _ = ICO[name]
    verts, faces, R, T, Kc, intr = _ico(name)
    _culling_matters(name, _ico_fragments(name, False)[0], _ico_fragments(name, True)[0])
    go = torch.rand(N, H, W, 4, generator=torch.Generator().manual_seed(7)) - 0.5
    runs = _oracle_render("cull fused soft silhouette K=8", verts, faces, R, T, intr, H, W, "silhouette", go, K=K,
                          blur=blur, clip=True)
    cams = _camera(Kc, H, W, DEV)
    rs = RasterizationSettings(image_size=(H, W), blur_radius=blur, faces_per_pixel=K, cull_backfaces=True)
    shader = SoftSilhouetteShader(blend_params=BlendParams(sigma=1e-4))
    rasterizer = MeshRasterizer(cams, rs)
    renderer = MeshRenderer(rasterizer, shader)

    def run(fused):
        v = verts.to(DEV).requires_grad_(True)
        Rg, Tg = R.to(DEV).requires_grad_(True), T.to(DEV).requires_grad_(True)
        m = Meshes([v], [faces.to(DEV)]).extend(N)
        img = renderer(m, R=Rg, T=Tg) if fused else shader(rasterizer(m, R=Rg, T=Tg), m)
        return img, (v, Rg, Tg)

    out, leaves = run(True)
    two, leaves2 = run(False)
    assert torch.equal(out.detach(), two.detach())
    _check_render("cull fused soft silhouette K=8", "silhouette", out, leaves, go, runs, zero_rows=20)
    (two * go.to(DEV)).sum().backward()
    again, leaves3 = run(False)
    (again * go.to(DEV)).sum().backward()
    for nm, a, b, b2 in zip(("verts", "R", "T"), leaves, leaves2, leaves3):
        # the same per-fragment gradients summed per face in another grouping and float-atomic order: a tenth
        # of the oracle bar, with the two-step path's own run-to-run spread as the conditioning (test_gpu_soft_fused)
        report(f"cull fused soft silhouette vs two-step grad {nm}", a.grad, b.grad, tol=1e-5,
               sens=(b.grad - b2.grad).abs())
    _zero_rows_stay_zero("cull two-step soft silhouette", leaves2[0].grad, runs[0][1], 20)
