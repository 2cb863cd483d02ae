"""The count -> scan -> fill binning (k_bin_count_* / k_bin_scan / k_bin_fill_*), which tile grids the per-view
binning refuses fall back to, at the two grids that take its two variants:

  16 x 2056   257 tile columns (more than the per-view binning's 256), 514 tiles: the LDS-histogram variants;
  136 x 8192  17 x 1024 = 17,408 tiles, above the LDS histogram's 16,384: the global-atomic variants, at the
              library's maximum width.

face_verts mode (rasterize_meshes_fwd) against the oracle on the same face_verts, to tests/test_gpu_raster.py's
bar: pix_to_face equal, zbuf / bary / dists bitwise. Three distinct meshes (ico-spheres) per batch, in two
orderings of their face counts: 20, 1280, 80 — the first 512-face workgroup straddles meshes 0 and 1, the second
lies inside mesh 1 (and alone takes the LDS histogram), the third straddles meshes 1 and 2 — and 20, 320, 80 —
one workgroup, mesh 1 strictly inside it (its entry total is added per face). Also with three faces per pixel and a
blur (the K-deep consumer of the filled lists) and with a near plane that splits faces (the lists' second-triangle
entries). World mode (the fused render, shared mesh and distinct meshes) against the modular rasterizer at the same
settings, which the tests above pin to the oracle.

Geometry: unit ico-spheres stretched to ellipses one image high and many tiles wide, each mesh (view) shifted
along NDC x so that the three land in different tile columns and the last reaches the right-most ones (> 255)."""
import functools

import pytest
import torch

from oracle import oracle as O
from torch_renderer_amd import _lib
from torch_renderer_amd import kernels as Kn
from torch_renderer_amd.utils import ico_sphere

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (H, W): NDC half-width of a mesh, NDC x of the three meshes' centres. NDC spans +-1 over the H rows and
# +-W / H over the columns (128.5 and 60.2), x decreasing to the right: the last mesh crosses the right edge.
GRIDS = {
    (16, 2056): (40.0, (85.0, 0.0, -100.0)),
    (136, 8192): (10.0, (45.0, 0.0, -52.0)),
}
LEVELS = {"20_1280_80": (0, 3, 1), "20_320_80": (0, 2, 1)}
Z_CLIP = 2.0  # view z of the meshes spans 1.5 .. 2.5


@functools.lru_cache(maxsize=None)
def _sphere(level):
    m = ico_sphere(level)
    return m.verts_list()[0].float(), m.faces_list()[0].long()


@functools.lru_cache(maxsize=None)
def _face_verts(grid, order):
    """(face_verts (F,3,3) in NDC, first, count) of the three meshes (never modified)."""
    half, centres = GRIDS[grid]
    fvs, counts = [], []
    for level, cx in zip(LEVELS[order], centres):
        v, f = _sphere(level)
        ndc = torch.stack([v[:, 0] * half + cx, v[:, 1] * 0.95, v[:, 2] * 0.5 + 2.0], 1)
        fvs.append(ndc[f])
        counts.append(f.shape[0])
    count = torch.tensor(counts)
    return torch.cat(fvs, 0).contiguous(), torch.cumsum(count, 0) - count, count


def _falls_back(N, NF, H, W):
    assert _lib.load().mr_per_view_binning(N, NF, H, W) == 0, "the per-view binning must refuse this grid"


def _covered(tag, p2f, W):
    """Every view covers something, and the batch reaches the tile columns past 255."""
    cov = (p2f[..., 0] >= 0)
    per_view = cov.flatten(1).sum(1).tolist()
    print(f"[fallback] {tag}: covered pixels per view {per_view}")
    assert min(per_view) > 0, (tag, per_view)
    assert bool(cov[:, :, 2048:].any()), f"{tag}: no face in the tile columns above 255"


def _bitwise(tag, got, ref):
    assert torch.equal(got[0].cpu(), ref[0]), f"{tag}: pix_to_face"
    for a, b, nm in zip(got[1:], ref[1:], ("zbuf", "bary", "dists")):
        assert torch.equal(a.cpu().view(torch.int32), b.view(torch.int32)), f"{tag}: {nm} not bitwise"


# ------------------------------------------------------------------------------------------ face_verts mode
@pytest.mark.parametrize("order", list(LEVELS))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_face_verts_fragments_bitwise(grid, order):
    H, W = grid
    fv, first, count = _face_verts(grid, order)
    _falls_back(3, fv.shape[0], H, W)
    ref = O.raster_fwd(fv, first, count, H, W, 1, 0.0, True, False, False)
    _covered(f"{H}x{W} {order}", ref[0], W)
    got = Kn.rasterize_meshes_fwd(fv.to(DEV), first.to(DEV), count.to(DEV), H, W, 1, 0.0, True, False)
    _bitwise(f"{H}x{W} {order}", got, ref)


@pytest.mark.parametrize("order", list(LEVELS))
def test_face_verts_three_per_pixel_blurred(order):
    """faces_per_pixel = 3 with a blur: k_raster_k reads the filled lists through the per-tile ranges."""
    H, W, K, blur = 16, 2056, 3, 2e-4
    fv, first, count = _face_verts((H, W), order)
    _falls_back(3, fv.shape[0], H, W)
    ref = O.raster_fwd(fv, first, count, H, W, K, blur, True, True, False)
    _covered(f"K=3 {order}", ref[0], W)
    assert int((ref[0][..., 1] >= 0).sum()) > 1000, "the second layer must be filled"
    got = Kn.rasterize_meshes_fwd(fv.to(DEV), first.to(DEV), count.to(DEV), H, W, K, blur, True, True)
    _bitwise(f"K=3 {order}", got, ref)


@pytest.mark.parametrize("order", list(LEVELS))
def test_face_verts_near_plane_clipped(order):
    """z_clip through the meshes (tests/test_gpu_clip.py's oracle chain: clip_faces -> rasterize with the
    neighbour rule -> convert back): the split faces' second triangles are listed by the fill's q = 1 entries."""
    H, W = 16, 2056
    fv, first, count = _face_verts((H, W), order)
    _falls_back(3, fv.shape[0], H, W)
    cf = O.clip_faces_ref(fv, first, count, Z_CLIP, persp=True)
    n_split = int((cf["neighbor"] >= 0).sum())
    print(f"[fallback] clip {order}: {n_split} sub-triangles of split faces")
    assert n_split > 0, "the near plane must split at least one face"
    p2f_c, zbuf, bary_c, dists = O.raster_fwd(cf["face_verts"], cf["first"], cf["count"], H, W, 1, 0.0, True, False,
                                              False, cf["neighbor"])
    p2f, bary = O.unclip_fragments(p2f_c, bary_c, cf)
    _covered(f"clip {order}", p2f, W)
    got = Kn.rasterize_meshes_fwd(fv.to(DEV), first.to(DEV), count.to(DEV), H, W, 1, 0.0, True, False, z_clip=Z_CLIP)
    _bitwise(f"clip {order}", got, (p2f, zbuf, bary, dists))


# ------------------------------------------------------------------------------------------ world mode
def _world_views(grid):
    """R, T, intr of three views whose NDC affine (ax x / z + bx) stretches the unit sphere at z = 2 to the
    GRIDS ellipse and shifts it to the three centres."""
    half, centres = GRIDS[grid]
    R = torch.eye(3).expand(3, 3, 3).contiguous()
    T = torch.tensor([[0.0, 0.0, 2.0]]).expand(3, 3).contiguous()
    intr = torch.tensor([[2.0 * half, cx, 1.9, 0.0] for cx in centres])
    return R, T, intr


def _world_mesh(levels):
    """Union (verts, faces) of the spheres squeezed to half depth, with the ranges render_views takes."""
    vs, fs, counts, voff = [], [], [], 0
    for level in levels:
        v, f = _sphere(level)
        vs.append(v * torch.tensor([1.0, 1.0, 0.5]))
        fs.append(f + voff)
        voff += v.shape[0]
        counts.append(f.shape[0])
    first = [0]
    for c in counts:
        first.append(first[-1] + c)
    vfirst = [0]
    for v in vs:
        vfirst.append(vfirst[-1] + v.shape[0])
    return (torch.cat(vs, 0).contiguous(), torch.cat(fs, 0).contiguous(), torch.tensor(first), torch.tensor(counts),
            max(counts), torch.tensor(vfirst), max(v.shape[0] for v in vs))


def _check_fused(tag, out, frag, W):
    p2f, zbuf = frag[0], frag[1]
    _covered(tag, p2f.cpu(), W)
    assert torch.equal(out["pix_to_face32"].long(), p2f[..., 0]), f"{tag}: pix_to_face"
    assert torch.equal(out["depth"], torch.relu(zbuf[..., 0])), f"{tag}: depth"


@pytest.mark.parametrize("grid", list(GRIDS))
def test_fused_render_shared_mesh(grid):
    H, W = grid
    verts, faces = _world_mesh((3,))[:2]
    R, T, intr = (t.to(DEV) for t in _world_views(grid))
    N, Fn = 3, faces.shape[0]
    _falls_back(N, N * Fn, H, W)
    fv = Kn.ProjectFaces.apply(verts.to(DEV), R, T, faces.to(DEV), intr)
    frag = Kn.rasterize_meshes_fwd(fv, torch.arange(N, device=DEV) * Fn, torch.full((N,), Fn, device=DEV), H, W)
    out = Kn.render_views(verts.to(DEV), R, T, faces.to(DEV), intr, torch.zeros(1, 3, device=DEV),
                          Kn.ShadeConfig(H=H, W=W, want_p2f=True))
    _check_fused(f"fused shared {H}x{W}", out, frag, W)


@pytest.mark.parametrize("order", list(LEVELS))
def test_fused_render_distinct_meshes(order):
    H, W = 16, 2056
    verts, faces, first, count, fmax, vfirst, vmax = _world_mesh(LEVELS[order])
    R, T, intr = (t.to(DEV) for t in _world_views((H, W)))
    _falls_back(3, faces.shape[0], H, W)
    first, count, vfirst = first.to(DEV), count.to(DEV), vfirst.to(DEV)
    fv = Kn.ProjectFacesMeshes.apply(verts.to(DEV), R, T, faces.to(DEV), intr, first, fmax, vfirst, vmax)
    frag = Kn.rasterize_meshes_fwd(fv, first[:-1].contiguous(), count, H, W)
    out = Kn.render_views(verts.to(DEV), R, T, faces.to(DEV), intr, torch.zeros(1, 3, device=DEV),
                          Kn.ShadeConfig(H=H, W=W, want_p2f=True), ranges=(first, count, fmax))
    _check_fused(f"fused distinct {order}", out, frag, W)
