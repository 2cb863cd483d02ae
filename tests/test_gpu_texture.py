"""The UV-texture sampler (csrc/mr_shade.h: tex_locate, tex_taps, tex_taps_raw, taps_from_raw, tex_blend,
tex_sample_bwd, tex_map_bwd) away from the cow's square 1024 x 1024 map and its in-range UVs, and the
verts_uvs gradient (mr_shade_fragments_backward's g_verts_uvs) that no other test reads.

Inputs: the jittered ico-sphere (tests.helpers.jittered_ico) with spherical UVs computed here
(u = atan2(x, z) / 2 pi + 1/2, v = asin(y) / pi + 1/2 of the normalised vertex, mapped to [lo, hi]; the faces
across the +-pi seam sweep the whole map and are kept: the steep case), "stretched" to [-0.25, 1.25] so that a
quarter or more of the samples clamp at the border, or "interior" [0, 1]; tiny random maps that are neither
square nor large — (5, 7), (9, 4), one texel high or wide (1, 6), (6, 1), and (1, 1) — as float values or as
exact k / 255 values (which TexturesUV.u8_map turns into the 8-bit copy the SPEC kernels read).

1. the K-deep shaders over the oracle's own fragments (tests/test_gpu_soft.py), with the map AND verts_uvs as
   leaves: rgba and six gradients;
2. the fused K = 1 render (MeshRenderer, DepthColorRender, kernels.render_views with the 8-bit copy withheld);
3. a learned texture end to end (TexturesUV whose map and uvs require grad: the modular routing of
   MeshRenderer.forward and DepthColorRender.render, the union path for distinct meshes sharing one map and
   the per-mesh loop for maps that differ).

Everything is held to tests.helpers.report's bar against the oracle (oracle_runs: f32 oracle, float64 shadow,
conditioning spread). Before any GPU output is read each case asserts, from the oracle alone: the share of
clamping samples (stretched), a non-zero verts_uvs gradient (exactly zero on the (1, 1) map), that no sample
sits exactly on the first or last texel of an axis (there torch's scalar and vectorised grid_sample kernels
disagree on whether the position gradient passes; the kernels follow the vectorised one and this file does not
depend on it), and tests.helpers.assert_cap on every tensor compared."""
import functools
import math

import pytest
import torch

from oracle import oracle as O
from tests.helpers import assert_cap, canonical_views, cv_to_p3d, jittered_ico, oracle_runs, report
from tests.test_gpu_cull import _camera
from torch_renderer_amd import Meshes, TexturesUV
from torch_renderer_amd.cameras import PerspectiveCameras
from torch_renderer_amd.mesh_renderer import (BlendParams, Fragments, HardPhongShader, Materials, MeshRasterizer,
                                              MeshRenderer, PointLights, RasterizationSettings, SoftPhongShader)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BLUR = math.log(1.0 / 1e-4 - 1.0) * 1e-4
N = 2
STRETCHED, INTERIOR = (-0.25, 1.25), (0.0, 1.0)
# the non-default light, material, camera centre and background of tests/test_gpu_soft.py
LIGHT = {"kind": "point", "location": (0.3, 0.8, -2.5), "ambient": (0.5, 0.4, 0.3), "diffuse": (0.3, 0.4, 0.5),
         "specular": (0.2, 0.25, 0.3)}
MAT = {"ambient": (1.0, 0.9, 0.8), "diffuse": (1.0, 1.0, 0.7), "specular": (0.6, 1.0, 1.0), "shininess": 32.0}
CC = torch.tensor([[0.1, -0.2, 0.3]])
BG = (0.1, 0.2, 0.3)


def _leaf(t, grad=True):
    return t.detach().clone().requires_grad_(grad)


def synthetic_uvs(verts, lo, hi):
    d = verts / verts.norm(dim=1, keepdim=True)
    u = torch.atan2(d[:, 0], d[:, 2]) / (2.0 * math.pi) + 0.5
    v = torch.asin(d[:, 1]) / math.pi + 0.5
    return (torch.stack([u, v], 1) * (hi - lo) + lo).contiguous()


def random_map(Ht, Wt, exact8):
    """(Ht, Wt, 3) float32: uniform values, or exact k / 255 ones (a PNG read as uint8 / 255)."""
    g = torch.Generator().manual_seed(100 * Ht + Wt)
    if exact8:
        return torch.randint(0, 256, (Ht, Wt, 3), generator=g).float() / 255.0
    return torch.rand((Ht, Wt, 3), generator=g)


@functools.lru_cache(maxsize=None)
def _scene(level, H, W):
    """(verts, faces, R, T, R_cv, t_cv, Kc, intr) on the CPU (never modified); intr is the camera's own NDC
    affine (tests/test_gpu_cull.py), R, T the PyTorch3D form of the OpenCV poses R_cv, t_cv."""
    verts, faces = jittered_ico(level)
    R, T, _, (R_cv, t_cv, Kc) = canonical_views(verts, N, H, W)
    intr = _camera(Kc, H, W, "cpu").ndc_affine((H, W)).expand(N, 4).contiguous()
    Rp, Tp = cv_to_p3d(R_cv, t_cv)
    assert torch.equal(Rp, R) and torch.equal(Tp, T)
    return verts, faces, R, T, R_cv, t_cv, Kc, intr


@functools.lru_cache(maxsize=None)
def _fragments(level, H, W, K):
    """The oracle's K-deep fragments of a scene (never modified): blur and barycentric clipping for K > 1."""
    verts, faces, R, T, _, _, _, intr = _scene(level, H, W)
    ref = O.render_ref(verts, faces, R, T, intr, H, W, K=K, blur=BLUR, clip=K > 1)
    return ref["p2f"], ref["zbuf"], ref["bary"], ref["dists"]


def _local(p2f, Fn):
    local = p2f.clone()
    local[p2f >= 0] = p2f[p2f >= 0] % Fn
    return local


def _uv_conditions(tag, p2f, bary, Fn, vuv, fuv, shape, stretched):
    """From the oracle's fragments alone: enough samples clamp (stretched), and none sits exactly on the first
    or last texel of an axis longer than one texel. The positions are grid_sample's own float32 expression
    ((2 uv - 1 + 1) / 2) (size - 1) of interpolate_face_attributes' uv."""
    uv = O.interpolate_face_attributes(_local(p2f, Fn), bary, vuv[fuv])[p2f >= 0]
    assert uv.shape[0] >= 100, (tag, uv.shape[0])
    out = ((uv < 0) | (uv > 1)).any(-1).float().mean().item()
    print(f"[texture] {tag}: {uv.shape[0]} samples, {out:.2f} of them outside [0, 1]^2")
    if stretched:
        assert out >= 0.25, (tag, out)
    g = uv * 2.0 - 1.0
    for axis, size in ((0, shape[1]), (1, shape[0])):
        if size > 1:
            pos = ((g[:, axis] + 1.0) / 2.0) * (size - 1)
            assert not bool(((pos == 0) | (pos == size - 1)).any()), f"{tag}: a sample on the border texel, axis {axis}"


def _caps(tag, names, share, runs, skip=()):
    for i, nm in enumerate(names):
        if nm not in skip:
            assert_cap(f"{tag} {nm}", runs[0][i], runs[2][i], share=share[i])


def _uv_grad_conditions(tag, guv, shape, unreferenced=0):
    """From the oracle alone: some verts_uvs gradient row is non-zero — except on the (1, 1) map, where every
    position is x * 0 and the gradient exactly zero — and rows no face references carry none."""
    if shape == (1, 1):
        assert not bool(guv.any()), f"{tag}: the oracle's uv gradient on a 1 x 1 map must be exactly zero"
    else:
        assert int((guv != 0).any(1).sum()) >= 1, f"{tag}: the oracle's uv gradient is all zero"
    if unreferenced:
        assert not bool(guv[-unreferenced:].any())


def _lights_materials():
    lights = PointLights(location=[LIGHT["location"]], ambient_color=[LIGHT["ambient"]],
                         diffuse_color=[LIGHT["diffuse"]], specular_color=[LIGHT["specular"]])
    mats = Materials(ambient_color=[MAT["ambient"]], diffuse_color=[MAT["diffuse"]],
                     specular_color=[MAT["specular"]], shininess=MAT["shininess"])
    return lights, mats


# ------------------------------------------------------------------ 1. the shaders over the oracle's fragments
FRAG_NAMES = ("rgba", "grad zbuf", "grad bary", "grad dists", "grad verts", "grad map", "grad uvs")
FRAG_SHARE = (True, False, False, False, True, True, True)
# name: (level, H, W, K, shader, map shape, uv range, per-corner uvs)
SHADER_CASES = {
    "K1_5x7": (1, 32, 40, 1, "phong", (5, 7), STRETCHED, False),
    "K3_5x7": (1, 32, 40, 3, "phong", (5, 7), STRETCHED, False),
    "K3_9x4_level2": (2, 48, 40, 3, "phong", (9, 4), STRETCHED, False),
    "K3_5x7_hard": (1, 32, 40, 3, "hard", (5, 7), STRETCHED, False),
    "K3_1x6": (1, 32, 40, 3, "phong", (1, 6), INTERIOR, False),
    "K3_6x1": (1, 32, 40, 3, "phong", (6, 1), INTERIOR, False),
    "K1_1x1": (1, 32, 40, 1, "phong", (1, 1), INTERIOR, False),
    "K3_5x7_per_corner": (1, 32, 40, 3, "phong", (5, 7), STRETCHED, True),
}
# BlendParams.gamma by K. At K = 3 with test_gpu_soft.py's gamma = 1e-4 two fragments of nearly equal depth weigh
# exp(dz_inv / gamma) against each other: one ulp of the f32 100 - z (7.6e-6) moves that ratio by 8e-4, and the f32
# oracle's own dists gradient is 11 .. 73 x the bar from its float64 value (measured on canonical_views seeds 0, 1, 2,
# distances 3 and 6 and both image orientations; assert_cap's cap is 10). gamma = 1e-2 keeps every tensor within the
# cap (worst 7.1 x, at K = 1), and the sampler does not depend on it.
GAMMA = {1: 1e-4, 3: 1e-2}
UNREFERENCED = 5  # trailing verts_uvs rows of the per-corner case that no face references


@pytest.mark.parametrize("name", list(SHADER_CASES))
def test_hip_shader_samples_small_maps_on_oracle_fragments(name):
    level, H, W, K, shader, shape, rng, per_corner = SHADER_CASES[name]
    verts, faces = _scene(level, H, W)[:2]
    Fn = faces.shape[0]
    p2f, zbuf0, bary0, dists0 = _fragments(level, H, W, K)
    frag0 = {"zbuf": zbuf0, "bary": bary0, "dists": dists0}
    vuv, fuv = synthetic_uvs(verts, *rng), faces
    unref = 0
    if per_corner:  # one uv row per face corner, then rows that no face references
        tail = torch.rand((UNREFERENCED, 2), generator=torch.Generator().manual_seed(3)) * 1.5 - 0.25
        vuv = torch.cat([vuv[faces].reshape(-1, 2), tail], 0)
        fuv = torch.arange(3 * Fn).view(Fn, 3)
        unref = UNREFERENCED
    map0 = random_map(*shape, exact8=False)
    local = _local(p2f, Fn)
    go = torch.rand((N, H, W, 4), generator=torch.Generator().manual_seed(K)) - 0.5
    tag = f"texture shader {name}"
    gamma = GAMMA[K]
    _uv_conditions(tag, p2f, bary0, Fn, vuv, fuv, shape, rng == STRETCHED)

    def flat(precision):  # oracle shading on leaves; float64: its shadow (tests.helpers.report's conditioning)
        dt = torch.float32 if precision == "f32" else torch.float64
        L = {k: _leaf(frag0[k].to(dt)) for k in ("zbuf", "bary", "dists")}
        zbf, bry, dst = (O._jitter(L[k]) for k in ("zbuf", "bary", "dists"))  # probe (inside O.perturbed only)
        L["verts"], L["map"], L["uvs"] = _leaf(verts.to(dt)), _leaf(map0.to(dt)), _leaf(vuv.to(dt))
        texels = O.sample_textures_uv(local, bry, L["uvs"], fuv, L["map"])
        colors = O.phong_colors(local, bry, L["verts"], faces, texels, LIGHT, MAT, CC.to(dt))
        if shader == "phong":
            o = O.softmax_rgb_blend(colors, p2f, zbf, dst, 1e-4, gamma, BG)
        else:  # HardPhongShader: hard_rgb_blend of the same Phong colours
            o = O.hard_rgb_blend(colors, p2f, BG)
        o = O._jitter(o, False)
        (o * go.to(dt)).sum().backward()
        z = torch.zeros(1)
        return (o,) + tuple(L[k].grad if L[k].grad is not None else z for k in ("zbuf", "bary", "dists", "verts",
                                                                                 "map", "uvs"))

    runs = oracle_runs(flat)
    ref, r64, sp = runs
    skip = ("grad zbuf", "grad dists") if shader == "hard" else ()  # no depth / distance dependence
    _caps(tag, FRAG_NAMES, FRAG_SHARE, runs, skip)
    _uv_grad_conditions(tag, ref[6], shape, unref)

    def gpu(map_grad=True, uv_grad=True, scale=1.0):  # the HIP shader on the same fragments
        zg, bg_, dg = (_leaf(frag0[k].to(DEV)) for k in ("zbuf", "bary", "dists"))
        vg, mg, ug = _leaf(verts.to(DEV)), _leaf(map0.to(DEV), map_grad), _leaf(vuv.to(DEV), uv_grad)
        tex = TexturesUV(maps=[mg], faces_uvs=[fuv.to(DEV)], verts_uvs=[ug])
        meshes = Meshes([vg], [faces.to(DEV)], tex).extend(N)
        cams = PerspectiveCameras(device=DEV, R=torch.eye(3)[None], T=-CC @ torch.eye(3))
        lights, mats = _lights_materials()
        cls = SoftPhongShader if shader == "phong" else HardPhongShader
        sh = cls(device=DEV, cameras=cams, lights=lights, materials=mats,
                 blend_params=BlendParams(sigma=1e-4, gamma=gamma, background_color=BG))
        out = sh(Fragments(p2f.to(DEV), zg, bg_, dg), meshes)
        (out * (go * scale).to(DEV)).sum().backward()
        return out, (zg, bg_, dg, vg, mg, ug)

    out, leaves = gpu()
    report(f"{tag} rgba", out, ref[0], ref64=r64[0], sens=sp[0])
    for i, leaf in enumerate(leaves, start=1):
        if FRAG_NAMES[i] in skip:
            assert leaf.grad is None
            continue
        report(f"{tag} {FRAG_NAMES[i]}", leaf.grad, ref[i], ref64=r64[i], sens=sp[i])
    guv = leaves[5].grad.cpu()
    if shape == (1, 1):
        assert not bool(guv.any()), "a 1 x 1 map has no uv gradient"
    if unref:  # the (Vt, 2) buffer is cleared over its whole length
        assert not bool(guv[-unref:].any()), "verts_uvs rows that no face references got a gradient"
    if name != "K3_5x7":
        return
    # only one of the two texture leaves requires grad (g_tex_rgba / g_verts_uvs NULL): the surviving gradients
    # are the both-leaves run's — fragment gradients bitwise, the rest within 1e-6, the allowance
    # tests/test_gpu_soft.py gives the float atomics' summation order. These three runs take the upstream
    # gradient times 1/8 (exact in float32): at full scale a uv row's partial sums reach 4 .. 8, where one
    # rounding is 4.8e-7 and 1e-6 is two of them (the comparison measured 0.42 and 0.60 of its limit in two
    # runs); at 1/8 they stay below 1 and the same 1e-6 is sixteen roundings.
    out8, leaves8 = gpu(scale=0.125)
    for map_grad, uv_grad in ((False, True), (True, False)):
        out1, leaves1 = gpu(map_grad, uv_grad, scale=0.125)
        which = "uvs only" if uv_grad else "map only"
        assert torch.equal(out1, out8)
        assert (leaves1[4].grad is None) == (not map_grad) and (leaves1[5].grad is None) == (not uv_grad)
        for i, (a, b) in enumerate(zip(leaves1, leaves8), start=1):
            if a.grad is None:
                continue
            if i <= 3:
                assert torch.equal(a.grad, b.grad), f"{which}: {FRAG_NAMES[i]} not bitwise"
            else:
                report(f"{tag} {which} vs both leaves {FRAG_NAMES[i]}", a.grad, b.grad, tol=1e-6)


# ------------------------------------------------------------------ 2, 3. renders through the public classes
# name: (map shape, exact 8-bit values, uv range); level 2, 48 x 40
RENDER_CASES = {
    "u8_5x7": ((5, 7), True, STRETCHED),
    "f32_5x7": ((5, 7), False, STRETCHED),
    "u8_1x6": ((1, 6), True, INTERIOR),
    "f32_6x1": ((6, 1), False, INTERIOR),
}
LEVEL, RH, RW = 2, 48, 40
RENDERER_NAMES = ("rgba", "grad verts", "grad R", "grad T", "grad map", "grad uvs")
RENDERER_SHARE = (True, True, False, False, True, True)
CV_NAMES = ("depth", "sil", "rgb", "grad verts", "grad R_cv", "grad t_cv", "grad map", "grad uvs")
CV_SHARE = (True, True, True, True, False, False, True, True)


def _upstream_renderer(seed=21):
    return torch.rand((N, RH, RW, 4), generator=torch.Generator().manual_seed(seed)) - 0.5


def _upstream_cv(seed=22):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((N, RH, RW), generator=g) - 0.5, torch.rand((N, RH, RW), generator=g) - 0.5,
            torch.rand((N, RH, RW, 3), generator=g) - 0.5)


def _oracle_renderer(tag, parts, R, T, intr, go, learned):
    """oracle_runs of render_ref with this file's light, material, camera centre and background, one call per
    (verts, faces, vuv, fuv, map index) of `parts` (view n renders part n; one part: every view renders it),
    backward of (rgba * go).sum(). Flat: rgba, then per part grad verts, grad R, grad T and — learned — one
    gradient per map (maps shared by index: summed) and one per part's uvs."""
    maps0 = parts[0][5]

    def run(precision):
        vs = [_leaf(p[0]) for p in parts]
        Rr, Tr = _leaf(R), _leaf(T)
        maps = [_leaf(m, learned) for m in maps0]
        uvs = [_leaf(p[2], learned) for p in parts]
        imgs = []
        for i, p in enumerate(parts):
            sl = slice(i, i + 1) if len(parts) > 1 else slice(None)
            imgs.append(O.render_ref(vs[i], p[1], Rr[sl], Tr[sl], intr[sl].contiguous(), RH, RW,
                                     texture=("uv", uvs[i], p[3], maps[p[4]]), light=LIGHT, mat=MAT, cam_center=CC,
                                     bg=BG, precision=precision)["rgba"])
        img = torch.cat(imgs, 0)
        (img * go.to(img.dtype)).sum().backward()
        tex = tuple(m.grad for m in maps) + tuple(u.grad for u in uvs) if learned else ()
        return (img,) + tuple(v.grad for v in vs) + (Rr.grad, Tr.grad) + tex

    return oracle_runs(run)


def _render_scene(name):
    shape, exact8, rng = RENDER_CASES[name]
    verts, faces = _scene(LEVEL, RH, RW)[:2]
    return shape, exact8, rng, synthetic_uvs(verts, *rng), faces, random_map(*shape, exact8)


def _fused_conditions(tag, name):
    """_uv_conditions on the oracle's K = 1 fragments of a RENDER_CASES scene; returns its pix_to_face."""
    shape, _, rng, vuv, fuv, _ = _render_scene(name)
    verts, faces, R, T, _, _, _, intr = _scene(LEVEL, RH, RW)
    fr = O.raster_fwd(O.project_faces_torch(verts, faces, R, T, intr), torch.arange(N) * faces.shape[0],
                      torch.full((N,), faces.shape[0]), RH, RW)
    _uv_conditions(tag, fr[0], fr[2], faces.shape[0], vuv, fuv, shape, rng == STRETCHED)
    return fr[0]


def _phong_renderer(Kc):
    """MeshRenderer(MeshRasterizer, SoftPhongShader), K = 1 and no blur; the camera object's own pose puts the
    specular camera centre at CC, the views' R, T are per call."""
    cams = _camera(Kc, RH, RW, DEV, R=torch.eye(3)[None].to(DEV), T=(-CC).to(DEV))
    lights, mats = _lights_materials()
    shader = SoftPhongShader(device=DEV, cameras=cams, lights=lights, materials=mats,
                             blend_params=BlendParams(sigma=1e-4, gamma=1e-4, background_color=BG))
    return MeshRenderer(MeshRasterizer(cams, RasterizationSettings(image_size=(RH, RW))), shader)


def _oracle_cv(R_cv, t_cv, intr, verts, faces, vuv, fuv, tmap, go, learned):
    """oracle_runs of DepthColorRender's frame (depth, silhouette, Phong rgb with its light at (0, 0, -3), the
    default material, camera centre and white background) from OpenCV poses. Flat: CV_NAMES."""
    gD, gS, gC = go

    def run(precision):
        vr, Rr, tr = _leaf(verts), _leaf(R_cv), _leaf(t_cv)
        mr, ur = _leaf(tmap, learned), _leaf(vuv, learned)
        Rp, Tp = cv_to_p3d(Rr, tr)
        ref = O.render_ref(vr, faces, Rp, Tp, intr, RH, RW, texture=("uv", ur, fuv, mr), precision=precision)
        dt = ref["rgba"].dtype
        ((ref["depth"] * gD.to(dt)).sum() + (ref["sil"] * gS.to(dt)).sum() +
         (ref["rgba"][..., :3] * gC.to(dt)).sum()).backward()
        tex = (mr.grad, ur.grad) if learned else ()
        return (ref["depth"], ref["sil"], ref["rgba"][..., :3], vr.grad, Rr.grad, tr.grad) + tex

    return oracle_runs(run)


def _report_all(tag, names, runs, got):
    ref, r64, sp = runs
    for i, x in enumerate(got):
        report(f"{tag} {names[i]}", x, ref[i], ref64=r64[i], sens=sp[i])


@pytest.mark.parametrize("name", list(RENDER_CASES))
def test_fused_render_samples_small_maps(name):
    """2. Nothing in the texture requires grad: MeshRenderer and DepthColorRender are each one fused launch.
    An exact 8-bit map has TexturesUV.u8_map, so drop_in_shading selects the SPEC kernels (raw texel words
    kept across forward and backward); the same map through kernels.render_views with the 8-bit copy and the
    table withheld takes the float loads, and is held to the oracle too."""
    from torch_renderer_amd import kernels as Kn
    from torch_renderer_amd.torch_renderer import DepthColorRender

    shape, exact8, rng, vuv, fuv, tmap = _render_scene(name)
    verts, faces, R, T, R_cv, t_cv, Kc, intr = _scene(LEVEL, RH, RW)
    tag = f"texture fused {name}"
    p2f = _fused_conditions(tag, name)
    go, go_cv = _upstream_renderer(), _upstream_cv()
    runs = _oracle_renderer(tag, [(verts, faces, vuv, fuv, 0, [tmap])], R, T, intr, go, False)
    _caps(tag, RENDERER_NAMES[:4], RENDERER_SHARE, runs)
    runs_cv = _oracle_cv(R_cv, t_cv, intr, verts, faces, vuv, fuv, tmap, go_cv, False)
    _caps(f"{tag} cv", CV_NAMES[:6], CV_SHARE, runs_cv)

    tex = TexturesUV(maps=[tmap.to(DEV)], faces_uvs=[fuv.to(DEV)], verts_uvs=[vuv.to(DEV)])
    assert (tex.u8_map(0) is not None) == exact8  # which load path the fused kernels take

    def mesh():
        vg = _leaf(verts.to(DEV))
        return vg, Meshes([vg], [faces.to(DEV)], tex).extend(N)

    renderer = _phong_renderer(Kc)
    vg, meshes = mesh()
    Rg, Tg = _leaf(R.to(DEV)), _leaf(T.to(DEV))
    with torch.no_grad():
        assert torch.equal(renderer.rasterizer(meshes, R=Rg, T=Tg).pix_to_face.cpu(), p2f)
    out = renderer(meshes_world=meshes, R=Rg, T=Tg)
    (out * go.to(DEV)).sum().backward()
    _report_all(tag, RENDERER_NAMES, runs, (out, vg.grad, Rg.grad, Tg.grad))

    def cv_frame(render):
        vg, meshes = mesh()
        Rc, tc = _leaf(R_cv.to(DEV)), _leaf(t_cv.to(DEV))
        o = render(vg, meshes, Rc, tc)
        ((o[0] * go_cv[0].to(DEV)).sum() + (o[1] * go_cv[1].to(DEV)).sum() + (o[2] * go_cv[2].to(DEV)).sum()).backward()
        return tuple(x.detach() for x in o[:3]) + (vg.grad, Rc.grad, tc.grad) + tuple(o[3:])

    dcr = DepthColorRender(Kc.to(DEV), (RH, RW), device=DEV)
    got = cv_frame(lambda vg, meshes, Rc, tc: dcr.render(meshes, Rc, tc))
    _report_all(f"{tag} DepthColorRender", CV_NAMES, runs_cv, got)
    if not exact8:
        return
    rgba = torch.zeros(shape + (4,))
    rgba[..., :3] = tmap
    float_only = Kn.TextureArgs(2, vuv.to(DEV), fuv.to(torch.int32).to(DEV), rgba.to(DEV))  # no tex_u8 / tex_lut
    cfg = Kn.ShadeConfig(H=RH, W=RW, light_location=(0.0, 0.0, -3.0), want_p2f=True)

    def by_hand(vg, meshes, Rc, tc):
        o = Kn.render_views(vg, Rc, tc, faces.to(DEV), intr.to(DEV), torch.zeros(1, 3, device=DEV), cfg, float_only,
                            pose_cv=True)
        return o["depth"], o["sil"], o["rgb"], o["pix_to_face32"]

    got_f = cv_frame(by_hand)
    assert torch.equal(got_f[6].cpu().long(), p2f[..., 0])
    _report_all(f"{tag} render_views float loads", CV_NAMES, runs_cv, got_f[:6])
    for i in range(6):  # information only
        d = (got[i] - got_f[i]).abs().max().item()
        print(f"[texture] {tag} 8-bit vs float loads {CV_NAMES[i]}: max |difference| = {d:.3e}, "
              f"bitwise equal: {torch.equal(got[i], got_f[i])}")


@pytest.mark.parametrize("name", list(RENDER_CASES))
def test_learned_texture_end_to_end(name):
    """3. The map and verts_uvs require grad: textures_need_modular routes MeshRenderer.forward and
    DepthColorRender.render to the world rasterizer and ShadeFragments at K = 1, and both backwards run."""
    from torch_renderer_amd.torch_renderer import DepthColorRender, textures_need_modular

    shape, _, rng, vuv, fuv, tmap = _render_scene(name)
    verts, faces, R, T, R_cv, t_cv, Kc, intr = _scene(LEVEL, RH, RW)
    tag = f"texture learned {name}"
    _fused_conditions(tag, name)
    go, go_cv = _upstream_renderer(), _upstream_cv()
    runs = _oracle_renderer(tag, [(verts, faces, vuv, fuv, 0, [tmap])], R, T, intr, go, True)
    _caps(tag, RENDERER_NAMES, RENDERER_SHARE, runs)
    _uv_grad_conditions(tag, runs[0][5], shape)
    runs_cv = _oracle_cv(R_cv, t_cv, intr, verts, faces, vuv, fuv, tmap, go_cv, True)
    _caps(f"{tag} cv", CV_NAMES, CV_SHARE, runs_cv)
    _uv_grad_conditions(f"{tag} cv", runs_cv[0][7], shape)

    def mesh():
        vg, mg, ug = _leaf(verts.to(DEV)), _leaf(tmap.to(DEV)), _leaf(vuv.to(DEV))
        meshes = Meshes([vg], [faces.to(DEV)], TexturesUV(maps=[mg], faces_uvs=[fuv.to(DEV)], verts_uvs=[ug])).extend(N)
        assert textures_need_modular(meshes)
        return vg, mg, ug, meshes

    vg, mg, ug, meshes = mesh()
    Rg, Tg = _leaf(R.to(DEV)), _leaf(T.to(DEV))
    out = _phong_renderer(Kc)(meshes_world=meshes, R=Rg, T=Tg)
    (out * go.to(DEV)).sum().backward()
    _report_all(tag, RENDERER_NAMES, runs, (out, vg.grad, Rg.grad, Tg.grad, mg.grad, ug.grad))

    vg, mg, ug, meshes = mesh()
    Rc, tc = _leaf(R_cv.to(DEV)), _leaf(t_cv.to(DEV))
    d, s, c = DepthColorRender(Kc.to(DEV), (RH, RW), device=DEV).render(meshes, Rc, tc)
    ((d * go_cv[0].to(DEV)).sum() + (s * go_cv[1].to(DEV)).sum() + (c * go_cv[2].to(DEV)).sum()).backward()
    _report_all(f"{tag} DepthColorRender", CV_NAMES, runs_cv, (d, s, c, vg.grad, Rc.grad, tc.grad, mg.grad, ug.grad))


@pytest.mark.parametrize("shared", [True, False])
def test_learned_texture_distinct_meshes(shared):
    """3. A batch of two distinct meshes (the level-2 and level-1 spheres, view n rendering mesh n) with a
    learned texture. One map object for both: shade_fragments' union path (uv rows concatenated, faces_uvs
    shifted), the map's gradient the sum over the meshes. Two maps — (5, 7) and (9, 4) —: the per-mesh loop,
    each map's gradient from its own mesh only. Reference: one render_ref per mesh. (The level-2 sphere takes
    view 0: of the level-1 sphere's samples only 0.22 clamp there, 0.58 in view 1.)"""
    verts2, faces2, R, T, _, _, Kc, intr = _scene(LEVEL, RH, RW)
    verts1, faces1 = jittered_ico(1)
    maps0 = [random_map(5, 7, False)] if shared else [random_map(5, 7, False), random_map(9, 4, False)]
    parts = [(verts2, faces2, synthetic_uvs(verts2, *STRETCHED), faces2, 0, maps0),
             (verts1, faces1, synthetic_uvs(verts1, *STRETCHED), faces1, 0 if shared else 1, maps0)]
    tag = f"texture learned batch {'one map' if shared else 'two maps'}"
    for i, p in enumerate(parts):
        sl = slice(i, i + 1)
        fr = O.raster_fwd(O.project_faces_torch(p[0], p[1], R[sl], T[sl], intr[sl]), torch.zeros(1, dtype=torch.int64),
                          torch.tensor([p[1].shape[0]]), RH, RW)
        _uv_conditions(f"{tag} mesh {i}", fr[0], fr[2], p[1].shape[0], p[2], p[3], tuple(maps0[p[4]].shape[:2]), True)
    go = _upstream_renderer(seed=23)
    runs = _oracle_renderer(tag, parts, R, T, intr, go, True)
    nm = len(maps0)
    names = (("rgba", "grad verts 0", "grad verts 1", "grad R", "grad T") + tuple(f"grad map {i}" for i in range(nm)) +
             ("grad uvs 0", "grad uvs 1"))
    share = (True, True, True, False, False) + (True,) * (nm + 2)
    _caps(tag, names, share, runs)
    for i in (1, 2):
        _uv_grad_conditions(f"{tag} mesh {i - 1}", runs[0][-3 + i], (5, 7))

    vs = [_leaf(p[0].to(DEV)) for p in parts]
    ms = [_leaf(m.to(DEV)) for m in maps0]
    us = [_leaf(p[2].to(DEV)) for p in parts]
    tex = TexturesUV(maps=[ms[p[4]] for p in parts], faces_uvs=[p[3].to(DEV) for p in parts], verts_uvs=us)
    Rg, Tg = _leaf(R.to(DEV)), _leaf(T.to(DEV))
    out = _phong_renderer(Kc)(meshes_world=Meshes(vs, [p[1].to(DEV) for p in parts], tex), R=Rg, T=Tg)
    (out * go.to(DEV)).sum().backward()
    _report_all(tag, names, runs, (out, vs[0].grad, vs[1].grad, Rg.grad, Tg.grad) + tuple(m.grad for m in ms) +
                tuple(u.grad for u in us))
