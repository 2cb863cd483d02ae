"""Who writes the fused render's background, at the edges of the chunk arithmetic.

The forward's background (every pixel; k_shade_render overwrites the covered ones afterwards) is split over
k_bin_view's spare workgroups (the first ``fill_first`` 64-lane chunks) and k_tile_raster's waves (the rest:
a loop after the wave's raster units; for the depth + silhouette + RGB output set without clipping, one chunk
after each unit first, through fill_chunk_static). A pixel nobody writes keeps the caller's bytes; these cases fill the
caller-owned outputs with NaN, call ``mr_render_forward_opencv`` through the C ABI and require

* no NaN left, and every uncovered pixel exactly the background (depth 0, silhouette 0, the background colour,
  whose three channels differ so that a mis-phased RGB word shows);
* depth, silhouette and RGB bitwise those of ``mr_render_reshade`` over the same workspace (k_fill + k_shade:
  independent background code) and of a forward that also returns pix_to_face (the generic chunk writer);
* a second run bitwise equal to the first.

The shapes: one chunk per view; a partial last chunk; W % 4 != 0 (one pixel per lane, the old order); more
waves than chunks; views that look away from the mesh (no raster units: all of a wave's chunks after its empty
unit loop); and batches of at least as many views as the GPU has compute units, which leave k_bin_view no spare
workgroup, so that k_tile_raster writes the whole background: fewer chunks than units, many chunks per unit (a
far camera: one after each unit, the rest in the loop after the units), and views whose last chunk is partial
(20x36: 180 quads, the third chunk has 52; 12x20: one chunk of 60 quads), so that fill_chunk_static's lanes past
the view's end are exercised, with and without views that have no units.
"""
import ctypes

import pytest
import torch

from tests.helpers import canonical_views, jittered_ico
from torch_renderer_amd import _lib
from torch_renderer_amd import kernels as Kn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BG = (0.25, 0.5, 0.75)

# id: (H, W, N, views looking away, camera distance (None: the canonical one), outputs)
CASES = {
    "8x8_one_chunk_per_view": (8, 8, 1, "none", None, "all"),
    "20x36_partial_last_chunk": (20, 36, 3, "none", None, "all"),
    "7x9_w_not_multiple_of_4": (7, 9, 2, "none", None, "all"),
    "64x64_n17_unit_order": (64, 64, 17, "none", None, "all"),
    "64x64_n300_raster_writes_all": (64, 64, 300, "none", None, "all"),
    "128x128_n64_half_away": (128, 128, 64, "half", None, "all"),
    "64x64_n20_all_away": (64, 64, 20, "all", None, "all"),
    "96x96_n264_far_many_chunks_per_unit": (96, 96, 264, "none", 12.0, "all"),
    "64x64_n300_half_away": (64, 64, 300, "half", None, "all"),
    "64x64_n300_all_away": (64, 64, 300, "all", None, "all"),
    "20x36_n300_partial_chunks_in_the_raster": (20, 36, 300, "none", None, "all"),
    "20x36_n300_partial_chunks_half_away": (20, 36, 300, "half", None, "all"),
    "12x20_n520_partial_single_chunk_views": (12, 20, 520, "none", None, "all"),
    "20x36_depth_only": (20, 36, 3, "none", None, "depth"),
    "64x64_n300_depth_only": (64, 64, 300, "none", None, "depth"),
}


def _scene(H, W, N, away, dist):
    verts, faces = jittered_ico(1)  # 42 vertices, 80 faces
    _, _, intr, (R_cv, t_cv, _) = canonical_views(verts, N, H, W, dist=dist)
    R_cv, t_cv = R_cv.float(), t_cv.float()
    if away != "none":  # turn the camera round its y axis: the mesh lies behind it
        flip = torch.tensor([-1.0, 1.0, -1.0])
        sel = torch.arange(N) % 2 == 1 if away == "half" else torch.ones(N, dtype=torch.bool)
        R_cv[sel] = R_cv[sel] * flip[None, :, None]
        t_cv[sel] = t_cv[sel] * flip[None, :]
    return (verts.to(DEV).contiguous(), faces.to(DEV), R_cv.to(DEV).contiguous(), t_cv.to(DEV).contiguous(),
            intr.to(DEV).contiguous())


class _Render:
    """One scene's C ABI calls over caller-owned, NaN-filled outputs."""

    def __init__(self, H, W, N, away, dist, outputs):
        self.lib = _lib.load()
        self.H, self.W, self.N = H, W, N
        self.v, faces, self.R, self.t, self.intr = _scene(H, W, N, away, dist)
        self.f, self.vptr, self.vadj = Kn.mesh_topology(faces, self.v.shape[0])
        self.mesh = Kn._mesh_struct(self.v, self.f, self.vptr, self.vadj, None, Kn.TextureArgs(), None)
        want = outputs == "all"
        self.cfg = Kn.ShadeConfig(H=H, W=W, light_kind=1, background=BG, want_sil=want, want_rgb=want)
        self.cc = torch.zeros(1, 3, device=DEV)
        self.stream = _lib.stream_handle(DEV)
        self.names = ("depth", "sil", "rgb") if want else ("depth",)

    def outputs(self, p2f=False):
        o = {"depth": torch.full((self.N, self.H, self.W), float("nan"), device=DEV)}
        if "sil" in self.names:
            o["sil"] = torch.full((self.N, self.H, self.W), float("nan"), device=DEV)
            o["rgb"] = torch.full((self.N, self.H, self.W, 3), float("nan"), device=DEV)
        if p2f:
            o["p2f"] = torch.full((self.N, self.H, self.W), -7, dtype=torch.int32, device=DEV)
        return o

    def workspace(self):
        ws, wsb = Kn._workspace(self.lib.mr_render_workspace, DEV, self.N, self.f.shape[0], self.H, self.W, 0)
        return ws, wsb, torch.empty(self.N, 16, device=DEV)

    def forward(self, ws, wsb, views, o):
        rs, sp = self.cfg.raster_struct(), self.cfg.shade_struct()
        poses = _lib.MrOpencvPoses(self.R.data_ptr(), 9, self.t.data_ptr(), 3, self.intr.data_ptr(), 4)
        _lib.check(self.lib.mr_render_forward_opencv(
            ctypes.byref(self.mesh), ctypes.byref(poses), _lib.ptr(views), self.N, _lib.ptr(self.cc), 1,
            ctypes.byref(rs), ctypes.byref(sp), _lib.ptr(o["depth"]), _lib.ptr(o.get("sil")), _lib.ptr(o.get("rgb")),
            _lib.ptr(o.get("p2f")), _lib.ptr(ws), wsb, self.stream))
        torch.cuda.synchronize()
        return o

    def reshade(self, ws, wsb, views, o):
        rs, sp = self.cfg.raster_struct(), self.cfg.shade_struct()
        sp.out_flags |= 1 << _lib.MR_SREC_SLOT_SHIFT  # its own shading-record slot
        _lib.check(self.lib.mr_render_reshade(
            ctypes.byref(self.mesh), _lib.ptr(views), self.N, _lib.ptr(self.cc), 1, ctypes.byref(rs), ctypes.byref(sp),
            _lib.ptr(o["depth"]), _lib.ptr(o.get("sil")), _lib.ptr(o.get("rgb")), None, _lib.ptr(ws), wsb, self.stream))
        torch.cuda.synchronize()
        return o


@pytest.mark.parametrize("case", list(CASES))
def test_every_pixel_written_once_with_the_right_value(case):
    H, W, N, away, dist, outputs = CASES[case]
    r = _Render(H, W, N, away, dist, outputs)
    share = int(r.lib.mr_binning_background_pixels(N, r.f.shape[0], H, W, 1))
    print(f"[background] {case}: k_bin_view writes {share} of {N * H * W} background pixels")
    assert 0 <= share <= N * H * W
    ws, wsb, views = r.workspace()
    first = r.forward(ws, wsb, views, r.outputs())
    again = r.forward(ws, wsb, views, r.outputs())
    shaded = r.reshade(ws, wsb, views, r.outputs())
    generic = r.forward(*r.workspace(), r.outputs(p2f=True))
    covered = generic["p2f"] >= 0
    assert int((generic["p2f"] == -7).sum()) == 0, "pix_to_face pixels nobody wrote"
    ncov = int(covered.sum())
    print(f"[background] {case}: {ncov} covered pixels")
    if away == "all":
        assert ncov == 0
    elif dist is None:
        assert ncov > 0, "the case is meant to cover some pixels"
    expect = {"depth": torch.zeros((), device=DEV), "sil": torch.zeros((), device=DEV), "rgb": torch.tensor(BG, device=DEV)}
    for nm in r.names:
        a = first[nm]
        assert not bool(torch.isnan(a).any()), f"{nm}: pixels nobody wrote"
        unc = a[~covered]
        assert bool((unc == expect[nm]).all()), f"{nm}: an uncovered pixel is not the background"
        assert torch.equal(a, again[nm]), f"{nm}: two runs differ"
        assert torch.equal(a, shaded[nm]), f"{nm}: differs from mr_render_reshade (k_fill + k_shade)"
        assert torch.equal(a, generic[nm]), f"{nm}: differs from the forward that also writes pix_to_face"
        if ncov:
            assert bool((first["depth"][covered] > 0).all()), "a covered pixel without depth"
