"""The face-to-tile rectangles round inward (ndc_range_to_pix: ceil(pf0) .. floor(pf1)): geometry built to sit on
the rule's edges must still rasterize bit-exactly as the C oracle does, the fused render must still match its
oracle with the slot numbering that results, and the work counters must have moved — as far as the rule
allows and no farther.

Scenes: 400 NDC triangles of five kinds in rotation — corners exactly on pixel centres; the same moved one ulp
either way; triangles strictly between four centres (they cover nothing and now get no list entry); random
0.3 - 3 px triangles; triangles with a corner on the centre of a tile-boundary pixel (column 8k or 8k + 7)
reaching 0 - 0.4 px past it, i.e. not as far as the neighbouring tile's first centre. Anchors run from -1 to S,
so some faces hang off the image. Bars: test_gpu_raster.py's (pix_to_face, zbuf, bary, dists bitwise) and
test_gpu_render.py's (tests.helpers.report)."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.helpers import canonical_views, cv_to_p3d, intr_from_K, jittered_ico, mesh_arrays, oracle_runs, report
from tests.pixel_range_ref import F32, centre_ndc, pitch, tile_counts
from torch_renderer_amd import Meshes, TexturesVertex
from torch_renderer_amd import kernels as Kn
from torch_renderer_amd.torch_renderer import DepthColorRender

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NTRI = 400
SIZES = [(16, 16), (24, 40), (40, 24), (20, 36)]  # 20 x 36: W % 8 == 4


def _cont_ndc(x, S1, S2):
    """NDC of the continuous pixel coordinate x (an integer is a pixel centre), float32."""
    return (((S1 - 1) / 2.0 - np.asarray(x, np.float64)) * pitch(S1, S2)).astype(F32)


def adversarial_scene(H, W, seed=0):
    """face_verts (NTRI, 3, 3) float32: NDC x, y and view z."""
    rng = np.random.default_rng(seed)
    fv = np.empty((NTRI, 3, 3), dtype=F32)
    inf = F32(np.inf)
    for f in range(NTRI):
        kind = f % 5
        ax, ay = int(rng.integers(-1, W + 1)), int(rng.integers(-1, H + 1))
        if kind in (0, 1):  # corners on pixel centres, legs of 1 - 3 px (leaning by up to a pixel)
            lx, ly = int(rng.integers(1, 4)), int(rng.integers(1, 4))
            sx, sy = int(rng.integers(-1, 2)), int(rng.integers(-1, 2))
            if lx * ly - sx * sy == 0:
                sx = 0
            px = np.array([ax, ax + lx, ax + sx])
            py = np.array([ay, ay + sy, ay + ly])
            x, y = centre_ndc(px, W, H), centre_ndc(py, H, W)
            if kind == 1:  # one ulp either way, each coordinate on its own
                x = np.nextafter(x, np.where(rng.random(3) < 0.5, inf, -inf).astype(F32))
                y = np.nextafter(y, np.where(rng.random(3) < 0.5, inf, -inf).astype(F32))
        elif kind == 2:  # strictly between four centres
            x = _cont_ndc(ax + 0.08 + 0.84 * rng.random(3), W, H)
            y = _cont_ndc(ay + 0.08 + 0.84 * rng.random(3), H, W)
        elif kind == 3:  # random, 0.3 - 3 px
            s = 0.3 + 2.7 * rng.random()
            x = _cont_ndc(ax + rng.random() + s * (rng.random(3) - 0.5), W, H)
            y = _cont_ndc(ay + rng.random() + s * (rng.random(3) - 0.5), H, W)
        else:  # a corner on the centre of a tile-boundary pixel; the box reaches 0 - 0.4 px past it
            k = int(rng.integers(0, (W + 7) // 8))
            left = bool(rng.integers(0, 2))
            bx = 8 * k if left else min(8 * k + 7, W - 1)
            out = -1.0 if left else 1.0  # towards the neighbouring tile
            over = 0.4 * rng.random() * (rng.random() < 0.8)
            x = np.array([centre_ndc(bx, W, H), _cont_ndc(bx + out * over, W, H),
                          _cont_ndc(bx - out * (1.0 + 1.5 * rng.random()), W, H)], dtype=F32)
            y = np.array([centre_ndc(ay, H, W), _cont_ndc(ay + 1.0 + 1.5 * rng.random(), H, W),
                          _cont_ndc(ay + 2.0 * rng.random() - 1.0, H, W)], dtype=F32)
        if rng.random() < 0.5:  # either winding
            x, y = x[::-1], y[::-1]
        fv[f, :, 0], fv[f, :, 1] = x, y
        fv[f, :, 2] = 0.5 + 2.5 * rng.random(3)
    return torch.from_numpy(fv)


@functools.lru_cache(maxsize=None)
def _scene(H, W, K, blur):
    fv = adversarial_scene(H, W)
    first, count = torch.zeros(1, dtype=torch.int64), torch.full((1,), NTRI)
    return fv, first, count, O.raster_fwd(fv, first, count, H, W, K, blur, True, blur > 0.0)


@pytest.mark.parametrize("H,W", SIZES)
def test_scene_is_not_degenerate(H, W):
    """Of the oracle's own output: at K = 1 a quarter of the pixels covered, 100 distinct faces visible."""
    p2f = _scene(H, W, 1, 0.0)[3][0]
    cov = (p2f >= 0).float().mean().item()
    vis = int(torch.unique(p2f[p2f >= 0]).numel())
    print(f"[scene] {H}x{W}: covered {cov:.3f}, distinct faces {vis}")
    assert cov >= 0.25 and vis >= 100


@pytest.mark.parametrize("K,blur", [(1, 0.0), (4, 0.035)])
@pytest.mark.parametrize("H,W", SIZES)
def test_adversarial_scene_matches_oracle(H, W, K, blur):
    fv, first, count, ref = _scene(H, W, K, blur)
    got = Kn.rasterize_meshes_fwd(fv.to(DEV), first.to(DEV), count.to(DEV), H, W, K, blur, True, blur > 0.0)
    got = [t.cpu() for t in got]
    assert torch.equal(got[0], ref[0]), f"pix_to_face mismatch at {(got[0] != ref[0]).sum()} entries"
    for a, b, nm in zip(got[1:], ref[1:], ("zbuf", "bary", "dists")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{nm}: max diff {(a - b).abs().max()}"


def test_fused_render_of_pixel_sized_faces():
    """DepthColorRender (k_tile_raster MODE 1's rectangle, the slot kernels) on faces 1 - 3 px across."""
    H, W, N = 24, 40, 2
    verts, faces = jittered_ico(2)
    vcol = torch.rand(verts.shape, generator=torch.Generator().manual_seed(5))
    _, _, _, (R_cv, t_cv, K) = canonical_views(verts, N, H, W)
    R_cv, t_cv = R_cv.float(), t_cv.float()
    g = torch.Generator().manual_seed(3)
    gD, gS, gC = (torch.rand(N, H, W, generator=g) - 0.5, torch.rand(N, H, W, generator=g) - 0.5,
                  torch.rand(N, H, W, 3, generator=g) - 0.5)

    def run(precision):
        vr = verts.clone().requires_grad_(True)
        Rr = R_cv.clone().requires_grad_(True)
        tr = t_cv.clone().requires_grad_(True)
        Rp, Tp = cv_to_p3d(Rr, tr)
        ref = O.render_ref(vr, faces, Rp, Tp, intr_from_K(K, H, W, N), H, W, texture=("vertex", vcol),
                           precision=precision)
        dt = ref["rgba"].dtype
        ((ref["depth"] * gD.to(dt)).sum() + (ref["sil"] * gS.to(dt)).sum()
         + (ref["rgba"][..., :3] * gC.to(dt)).sum()).backward()
        return ref["depth"], ref["sil"], ref["rgba"][..., :3], vr.grad, Rr.grad, tr.grad

    ref, r64, sp = oracle_runs(run)
    assert (ref[1] > 0.5).float().mean() > 0.1, "degenerate test: almost nothing covered"
    vg = verts.to(DEV).requires_grad_(True)
    Rg = R_cv.to(DEV).requires_grad_(True)
    tg = t_cv.to(DEV).requires_grad_(True)
    m = Meshes([vg], [faces.to(DEV)], TexturesVertex([vcol.to(DEV)])).extend(N)
    d, s, c = DepthColorRender(K.to(DEV), (H, W), device=DEV).render(m, Rg, tg)
    ((d * gD.to(DEV)).sum() + (s * gS.to(DEV)).sum() + (c * gC.to(DEV)).sum()).backward()
    names = ("depth", "sil", "rgb", "grad verts", "grad R_cv", "grad t_cv")
    for i, x in enumerate((d, s, c, vg.grad, Rg.grad, tg.grad)):
        report(f"tight rects 24x40 {names[i]}", x, ref[i], rel_above_one=i >= 3, ref64=r64[i], sens=sp[i])


def test_counters_moved_as_far_as_the_rule_allows():
    """kernels.render_stats() of cow at 64x64, 2 views, against numpy restatements of the rule at 0.04 / 0.05 /
    0.06 px of slack (the bracket takes up the device's float32 inverse against numpy's float64 one) and of the
    outward rounding it replaced."""
    H = W = 64
    N = 2
    verts, faces, _ = mesh_arrays("cow")
    R, T, intr, _ = canonical_views(verts, N, H, W)
    F = faces.shape[0]
    fv = O.project_faces_c(verts, faces, O.views_tensor(R, T, intr))
    p2f = O.raster_fwd(fv, torch.arange(N) * F, torch.full((N,), F), H, W)[0]
    fvn = fv.numpy().reshape(N, F, 3, 3)
    x, y = fvn[..., 0].astype(np.float64), fvn[..., 1].astype(np.float64)
    area = (x[..., 2] - x[..., 0]) * (y[..., 1] - y[..., 0]) - (y[..., 2] - y[..., 0]) * (x[..., 1] - x[..., 0])
    valid = np.isfinite(fvn).all(axis=(2, 3)) & (fvn[..., 2].max(-1) >= 0) & (np.abs(area) > 1e-8)

    def count(slack, tight=True):
        e = t = 0
        for n in range(N):
            a, b = tile_counts(fvn[n], valid[n], H, W, slack, tight)
            e, t = e + a, t + b
        return e, t

    (e_lo, t_lo), (e_mid, t_mid), (e_hi, t_hi), (e_old, t_old) = count(0.04), count(0.05), count(0.06), count(0.05, False)
    cfg = Kn.ShadeConfig(H=H, W=W)
    out = Kn.render_views(verts.to(DEV).requires_grad_(True), R.to(DEV), T.to(DEV), faces.to(DEV), intr.to(DEV),
                          torch.zeros(1, 3, device=DEV), cfg)
    st = Kn.render_stats()
    print(f"[counters] GPU {st}; rule at 0.04 / 0.05 / 0.06 px: entries {e_lo} / {e_mid} / {e_hi}, tiles {t_lo} / "
          f"{t_mid} / {t_hi}; outward rounding: entries {e_old}, tiles {t_old}")
    del out
    assert e_lo <= st["entries"] <= e_hi
    assert t_lo <= st["tiles"] <= t_hi
    assert st["entries"] < 0.8 * e_old
    assert st["covered"] == int((p2f >= 0).sum())
