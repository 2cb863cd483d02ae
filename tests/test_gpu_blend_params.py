"""Blend and rasterization settings no other GPU test sets away from their defaults.

BlendParams.gamma and sigma and the blend's znear / zfar (call kwargs, or the FoV camera's own): make_shade
precomputes inv_gamma and inv_zrange on the host and the K-deep soft shader uses them forward and backward
(mr_frag_shade.h); every other test runs gamma = 1e-4 and the range 1 / 100, where a swapped or stale value
is invisible. Each case renders MeshRenderer + SoftPhongShader K-deep (HIP raster, then the HIP shader over
the fragments) against oracle.render_ref, values and grad verts / R / T within tests.helpers.report's bar,
after asserting from the oracle alone (a) that its own f32 spread stays within tests.helpers.assert_cap and
(b) that putting any one of the case's settings back to its default moves the reference image by more than
100 x the bar somewhere: a kernel that ignored the setting fails.

Inputs: the teapot and the jittered level-1 ico-sphere (the icosahedron for sigma = 3e-4: see CASES). The
level-2 sphere with Phong at gamma >= 1e-3 has an edge-on face whose f32 oracle gradient is 2e4 x the bar
from its float64 value, and gamma = 1e-4 with a tight z range is 304 x on the teapot: both break the cap and
are not used.

clip_barycentric_coords given explicitly (it is otherwise derived from blur_radius > 0): True without blur
and False with blur, fragments bitwise against the oracle's and the vertex gradient through them."""
import functools
import math

import pytest
import torch

from oracle import oracle as O
from tests.helpers import assert_cap, canonical_views, jittered_ico, mesh_arrays, oracle_runs, report
from tests.test_gpu_cull import FOV_T, LIGHT_LOC, _bitwise, _camera, _packed, _upstream
from torch_renderer_amd import Meshes, TexturesVertex
from torch_renderer_amd.cameras import FoVPerspectiveCameras
from torch_renderer_amd.mesh_renderer import (BlendParams, MeshRasterizer, MeshRenderer, PointLights,
                                              RasterizationSettings, SoftPhongShader)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BG = (0.2, 0.3, 0.4)
N = 2
DEFAULTS = {"sigma": 1e-4, "gamma": 1e-4, "zrange": (1.0, 100.0)}

# name: (mesh, H, W, K, camera, seed of canonical_views, settings away from DEFAULTS)
CASES = {
    "teapot_gamma1e-2": ("teapot", 40, 56, 4, "persp", 0, {"gamma": 1e-2}),
    "ico1_gamma1e-2": ("ico1", 32, 32, 8, "persp", 0, {"gamma": 1e-2}),
    "ico1_gamma1e-3": ("ico1", 32, 32, 8, "persp", 0, {"gamma": 1e-3}),
    "ico1_zrange_kwargs": ("ico1", 32, 32, 8, "persp", 0, {"gamma": 1e-2, "zrange": (3.0, 6.5)}),
    "ico1_zrange_fov": ("ico1", 32, 32, 8, "fov", 0, {"gamma": 1e-2, "zrange": (3.0, 6.5)}),
    # sigma = 3e-4 widens the blur radius to ln(1/1e-4 - 1) * sigma = 2.8e-3, so faces collect fragments further
    # outside them (presumably the cause of what follows). Measured on the oracle at this sigma: the f32 vertex and
    # pose gradients are 1e4 .. 1e9 x the bar from their float64 values at gamma >= 1e-3 on the teapot and the
    # level-1 / level-2 ico-spheres (49 x on the sphere asset), on the level-1 sphere for canonical_views seeds
    # 0..5 and distances 3 and 6, and at gamma = 1e-4 more than a third of the entries are ill-conditioned: all
    # break the cap. The jittered icosahedron seen from canonical_views(seed=2) does not (max spread 0.3 x the
    # bar; seeds 0, 1 and 3 do).
    "ico0_sigma3e-4": ("ico0", 32, 32, 8, "persp", 2, {"gamma": 1e-2, "sigma": 3e-4}),
}


@functools.lru_cache(maxsize=None)
def _scene(mesh, H, W, cam, seed):
    """(verts, faces, vcol, R, T, Kc, intr) on the CPU (never modified)."""
    verts, faces = jittered_ico(int(mesh[3])) if mesh.startswith("ico") else mesh_arrays(mesh)[:2]
    R, T, _, (_, _, Kc) = canonical_views(verts, N, H, W, seed=seed)
    if cam == "fov":  # FoVPerspectiveCameras(fov=60), square image
        intr = torch.tensor([[FOV_T, 0.0, FOV_T, 0.0]]).expand(N, 4).contiguous()
    else:
        intr = _camera(Kc, H, W, "cpu").ndc_affine((H, W)).expand(N, 4).contiguous()
    vcol = torch.rand(verts.shape, generator=torch.Generator().manual_seed(13))
    return verts, faces, vcol, R, T, Kc, intr


def _render_ref(name, settings, precision="f32", leaves=None):
    mesh, H, W, K, cam, seed, own = CASES[name]
    verts, faces, vcol, R, T, _, intr = _scene(mesh, H, W, cam, seed)
    s = {**DEFAULTS, **settings}
    v, Rr, Tr = leaves if leaves is not None else (verts, R, T)
    # the fragments are the case's own (blur_radius from ITS sigma) whatever `settings` blends them with
    blur = math.log(1.0 / 1e-4 - 1.0) * {**DEFAULTS, **own}["sigma"]
    zc = {**DEFAULTS, **own}["zrange"][0] / 2.0 if cam == "fov" else None  # MeshRasterizer: znear / 2
    return O.render_ref(v, faces, Rr, Tr, intr, H, W, texture=("vertex", vcol), light=dict(O.DEFAULT_LIGHT,
                        location=LIGHT_LOC), bg=BG, sigma=s["sigma"], gamma=s["gamma"], znear=s["zrange"][0],
                        zfar=s["zrange"][1], K=K, blur=blur, clip=True, z_clip=zc, precision=precision)


@pytest.mark.parametrize("name", list(CASES))
def test_soft_phong_blend_settings_match_oracle(name):
    mesh, H, W, K, cam, seed, settings = CASES[name]
    verts, faces, vcol, R, T, Kc, intr = _scene(mesh, H, W, cam, seed)
    s = {**DEFAULTS, **settings}
    go = torch.rand(N, H, W, 4, generator=torch.Generator().manual_seed(17)) - 0.5

    def run(precision):
        vr = verts.clone().requires_grad_(True)
        Rr, Tr = R.clone().requires_grad_(True), T.clone().requires_grad_(True)
        ref = _render_ref(name, settings, precision, (vr, Rr, Tr))
        (ref["rgba"] * go.to(ref["rgba"].dtype)).sum().backward()
        return ref["rgba"], vr.grad, Rr.grad, Tr.grad

    ref, r64, sp = oracle_runs(run)
    names = ("rgba", "grad verts", "grad R", "grad T")
    for i, nm in enumerate(names):
        assert_cap(f"blend {name} {nm}", ref[i], sp[i], share=i < 2)
    # each setting matters: back at its default (the others kept) the reference moves by > 100 x the bar
    for key in settings:
        other = _render_ref(name, {k: v for k, v in settings.items() if k != key})["rgba"]
        moved = (other - ref[0]).abs().max().item()
        print(f"[blend] {name}: {key} at its default moves the reference image by {moved:.3e}")
        assert moved > 100 * 1e-4, (name, key, moved)
    moved = (_render_ref(name, {})["rgba"] - ref[0]).abs().max().item()  # every blend setting at its default
    assert moved > 100 * 1e-4, (name, moved)
    if cam == "fov":
        fvz = O.project_faces_torch(verts, faces, R, T, intr)[..., 2]
        assert float(fvz.min()) > s["zrange"][0] / 2.0, "the mesh must lie in front of the near clip plane"

    kwargs = {}
    if cam == "fov":
        cams = FoVPerspectiveCameras(znear=s["zrange"][0], zfar=s["zrange"][1], device=DEV)
    else:
        cams = _camera(Kc, H, W, DEV)
        if "zrange" in settings:
            kwargs = {"znear": s["zrange"][0], "zfar": s["zrange"][1]}
    blend = BlendParams(sigma=s["sigma"], gamma=s["gamma"], background_color=BG)
    rs = RasterizationSettings(image_size=(H, W), blur_radius=math.log(1.0 / 1e-4 - 1.0) * s["sigma"],
                               faces_per_pixel=K)
    shader = SoftPhongShader(device=DEV, cameras=cams, lights=PointLights(device=DEV, location=[LIGHT_LOC]),
                             blend_params=blend)
    renderer = MeshRenderer(MeshRasterizer(cams, rs), shader)
    vg = verts.to(DEV).requires_grad_(True)
    Rg, Tg = R.to(DEV).requires_grad_(True), T.to(DEV).requires_grad_(True)
    out = renderer(meshes_world=Meshes([vg], [faces.to(DEV)], TexturesVertex([vcol.to(DEV)])).extend(N), R=Rg, T=Tg,
                   **kwargs)
    report(f"blend {name} rgba", out, ref[0], ref64=r64[0], sens=sp[0])
    (out * go.to(DEV)).sum().backward()
    for i, leaf in enumerate((vg, Rg, Tg)):
        report(f"blend {name} {names[i + 1]}", leaf.grad, ref[i + 1], ref64=r64[i + 1], sens=sp[i + 1])


@pytest.mark.parametrize("clip,blur", [(True, 0.0), (False, 2e-4)])
def test_explicit_clip_barycentric_coords(clip, blur):
    """clip_barycentric_coords set against what blur_radius > 0 would derive: the jittered level-2 ico-sphere
    at 40 x 56, K = 4. The oracle's barycentrics with and without the flag differ, so a rasterizer that
    derived the flag from the blur fails the bitwise comparison."""
    H, W, K = 40, 56, 4
    verts, faces = jittered_ico(2)
    R, T, _, (_, _, Kc) = canonical_views(verts, N, H, W)
    intr = _camera(Kc, H, W, "cpu").ndc_affine((H, W)).expand(N, 4).contiguous()
    first, count = _packed(N, faces.shape[0])
    vr = verts.clone().requires_grad_(True)
    fv = O.project_faces_torch(vr, faces, R, T, intr)
    derived = O.raster_fwd(fv, first, count, H, W, K, blur, True, blur > 0)
    p2f, zbuf, bary, dists = O.RasterizeRef.apply(fv, first, count, H, W, K, blur, True, clip, False)
    n_diff = int((bary.detach().view(torch.int32) != derived[2].view(torch.int32)).any(-1).sum())
    print(f"[clip-bary] clip={clip} blur={blur}: {n_diff} of {int((p2f >= 0).sum())} fragments' barycentrics differ "
          f"from the derived setting's")
    assert n_diff >= 100
    rs = RasterizationSettings(image_size=(H, W), blur_radius=blur, faces_per_pixel=K, clip_barycentric_coords=clip)
    vg = verts.to(DEV).requires_grad_(True)
    cams = _camera(Kc, H, W, DEV, R=R.to(DEV), T=T.to(DEV))
    fr = MeshRasterizer(cams, rs)(Meshes([vg], [faces.to(DEV)]).extend(N))
    _bitwise(f"clip_barycentric_coords={clip} blur={blur}", (fr.pix_to_face, fr.zbuf, fr.bary_coords, fr.dists),
             (p2f, zbuf, bary, dists))
    gz, gb, gd = _upstream((zbuf.shape, bary.shape, dists.shape), seed=8)
    ((fr.zbuf * gz.to(DEV)).sum() + (fr.bary_coords * gb.to(DEV)).sum() + (fr.dists * gd.to(DEV)).sum()).backward()
    ((zbuf * gz).sum() + (bary * gb).sum() + (dists * gd).sum()).backward()
    report(f"clip_barycentric_coords={clip} blur={blur} grad verts", vg.grad, vr.grad)
