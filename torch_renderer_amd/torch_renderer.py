"""Drop-in for the reference's ``torch_renderer.py`` renderer classes.

Same constructor signatures, argument meaning, outputs and error behaviour as
torch_renderer.py:39-159 (DifferentiableRenderer, DepthRender, ColorRender),
but every render is ONE fused HIP launch (project + bin + rasterize + shade)
and the autograd backward is one fused HIP launch + vertex gathers. The
reference's DepthRender with return_silhouette=True rasterizes twice
(torch_renderer.py:113 and :120); here depth and silhouette come from the same
pass. ``DepthColorRender`` adds the benchmark's frame: depth + silhouette +
RGB from one raster pass.

``AlphaPointRender`` / ``NormPointRender`` (torch_renderer.py:162-207) run on the point
rasterizer and compositors of ``points_renderer``; they do what the reference evidently
meant (its ``render`` passes an undefined ``Ts``). ``PulsarPointRender`` (:209-230) is out
of scope and raises.
"""
from __future__ import annotations

import torch

from .cameras import PerspectiveCameras, cached_camera_center, view_batch
from .kernels import ShadeConfig, TextureArgs, render_views
from .structures import Meshes, TexturesUV, TexturesVertex
from .transforms import opencv_to_pytorch3d


def texture_args(meshes: Meshes, need_color: bool):
    """(TextureArgs, vcolors tensor or None) for the mesh batch."""
    tex = meshes.textures
    if not need_color:
        return TextureArgs(0), None
    if tex is None:
        raise ValueError("Meshes does not have textures")  # upstream Meshes.sample_textures
    if isinstance(tex, TexturesUV):
        vuv, fuv = tex.kernel_uvs(0)
        u8 = tex.u8_map(0)
        return TextureArgs(2, vuv, fuv, tex.rgba_map(0), *(u8 if u8 is not None else (None, None))), None
    if isinstance(tex, TexturesVertex):
        vc = tex.verts_features_list()[0]
        if vc.shape[-1] != 3:
            raise NotImplementedError("TexturesVertex: only 3-channel features are supported")
        return TextureArgs(1), vc
    raise NotImplementedError(f"textures of type {type(tex).__name__}")


_UNION_CACHE = {}


def _union_topology(meshes: Meshes):
    """(faces (F,3) int64 of the union, view_face_first (N+1), view_face_count (N) int64 device
    tensors, largest face count, view_vert_first (N+1), largest vertex count) of a batch of distinct
    meshes, cached on the identity and version of the faces tensors and the identity and vertex count
    of the verts tensors — not their version: the union depends on faces and vertex counts only, so an
    in-place vertex update (an optimiser step on distinct meshes' verts) keeps the entry, and with it
    the union faces tensor's identity and its cached CSR. The entry holds the source tensors themselves
    and is matched by `is`, so a garbage-collected batch cannot hand its ids to a new one."""
    fl, vl = meshes.faces_list(), meshes.verts_list()
    hit = _UNION_CACHE.get(id(meshes))
    if hit is not None and _same_sources(hit[0], fl, vl, b_values=False):
        return hit[1]
    voff, out = 0, []
    for v, f in zip(vl, fl):
        out.append(f.to(torch.int64) + voff)
        voff += v.shape[0]
    counts = [f.shape[0] for f in fl]
    vcounts = [v.shape[0] for v in vl]
    first, vfirst = [0], [0]
    for c, vc in zip(counts, vcounts):
        first.append(first[-1] + c)
        vfirst.append(vfirst[-1] + vc)
    dev = fl[0].device
    res = (torch.cat(out, 0).contiguous(), torch.tensor(first, dtype=torch.int64, device=dev),
           torch.tensor(counts, dtype=torch.int64, device=dev), max(counts),
           torch.tensor(vfirst, dtype=torch.int64, device=dev), max(vcounts))
    if len(_UNION_CACHE) > 16:
        _UNION_CACHE.clear()
    _UNION_CACHE[id(meshes)] = (_sources(fl, vl, b_values=False), res)
    return res


def _sources(al, bl, b_values=True):
    """Cache-entry record of two tensor lists: the tensors (kept alive) and their versions (for the
    second list with b_values=False, its leading size instead: only its shape matters)."""
    return tuple((a, a._version, b, b._version if b_values else b.shape[0]) for a, b in zip(al, bl)), len(al)


def _same_sources(rec, al, bl, b_values=True):
    entries, n = rec
    return n == len(al) == len(bl) and all(
        a is a0 and a._version == va and b is b0 and (b._version if b_values else b.shape[0]) == vb
        for (a0, va, b0, vb), a, b in zip(entries, al, bl))


def union_texture_args(meshes: Meshes, need_color: bool):
    """texture_args for the union of a batch of distinct meshes, or None when the textures cannot be
    joined (UV maps that differ between meshes: one fused launch per mesh then)."""
    tex = meshes.textures
    if not need_color:
        return TextureArgs(0), None
    if tex is None:
        raise ValueError("Meshes does not have textures")
    if isinstance(tex, TexturesVertex):
        vcs = tex.verts_features_list()
        if any(vc.shape[-1] != 3 for vc in vcs):
            raise NotImplementedError("TexturesVertex: only 3-channel features are supported")
        return TextureArgs(1), torch.cat(list(vcs), 0)
    if isinstance(tex, TexturesUV):
        maps = tex.maps_list()
        if any(m is not maps[0] and (m.data_ptr() != maps[0].data_ptr() or m.shape != maps[0].shape) for m in maps):
            return None
        vl = meshes.verts_list()
        vul, ful = list(tex.verts_uvs_list()), list(tex.faces_uvs_list())
        hit = _UNION_CACHE.get(("uv", id(tex)))
        if hit is None or not _same_sources(hit[0], vul, ful):
            vus, fus, off = [], [], 0
            for i in range(len(vl)):
                vu, fu = tex.verts_uvs_list()[i], tex.faces_uvs_list()[i]
                vus.append(vu.float())
                fus.append(fu.to(torch.int32) + off)
                off += vu.shape[0]
            hit = (_sources(vul, ful), (torch.cat(vus, 0).contiguous(), torch.cat(fus, 0).contiguous()))
            _UNION_CACHE[("uv", id(tex))] = hit
        vuv, fuv = hit[1]
        u8 = tex.u8_map(0)
        return TextureArgs(2, vuv, fuv, tex.rgba_map(0), *(u8 if u8 is not None else (None, None))), None
    raise NotImplementedError(f"textures of type {type(tex).__name__}")


def textures_need_modular(meshes: Meshes) -> bool:
    """A TexturesUV map / uv set that requires grad cannot go through the fused K=1 kernels
    (they read a cached detached RGBA copy): route the render through the modular path instead of
    silently dropping the gradient (never silently differ)."""
    tex = meshes.textures
    return tex is not None and getattr(tex, "requires_grad", lambda: False)()


def render_mesh_batch(meshes: Meshes, cameras, image_size, R, T, cfg: ShadeConfig, cam_center=None,
                      pose_cv=False, views=None):
    """Render every view of `meshes` (shared mesh or per-view meshes) with the fused kernels.
    Returns dict(depth, sil, rgb[, pix_to_face32 if cfg.want_p2f]) with tensors of batch N.
    pose_cv: R, T are OpenCV poses; the PyTorch3D conversion of torch_renderer.py:73-80 runs
    on the GPU inside the render (mr_views_from_opencv) and gradients come back in kind."""
    H, W = image_size
    if views is not None:  # (R, T, intr) already broadcast by the caller's view_batch
        Rb, Tb, intr = views
        n = Rb.shape[0]
    else:
        n = max(len(meshes), R.reshape(-1, 3, 3).shape[0], T.reshape(-1, 3).shape[0])
        Rb, Tb, intr = view_batch(cameras, (H, W), R, T, n_views=n)
    if cam_center is None:
        cam_center = cached_camera_center(cameras, Rb.device)
    need_color = cfg.want_rgb
    if meshes.is_shared():
        tex, vcol = texture_args(meshes, need_color)
        return render_views(meshes.shared_verts(), Rb, Tb, meshes.shared_faces(), intr, cam_center,
                            cfg, tex, vcolors=vcol, pose_cv=pose_cv)
    if len(meshes) != n:
        raise ValueError(f"Meshes batch ({len(meshes)}) and camera batch ({n}) differ")
    ut = union_texture_args(meshes, need_color)
    if ut is not None:  # distinct meshes: their union in one launch, view n rendering mesh n
        faces_u, first, count, fmax = _union_topology(meshes)[:4]
        if ut[0].kind == 2 and ut[0].faces_uvs.shape[0] != faces_u.shape[0]:
            raise RuntimeError(f"union faces_uvs ({ut[0].faces_uvs.shape[0]}) and faces ({faces_u.shape[0]}) differ")
        return render_views(torch.cat(list(meshes.verts_list()), 0), Rb, Tb, faces_u, intr, cam_center, cfg, ut[0],
                            vcolors=ut[1], pose_cv=pose_cv, ranges=(first, count, fmax))
    outs = []
    for i in range(n):  # UV maps that differ between meshes: one fused launch per view
        mi = meshes[i]
        tex, vcol = texture_args(mi, need_color)
        cc = cam_center[i:i + 1] if cam_center.shape[0] > 1 else cam_center
        outs.append(render_views(mi.shared_verts(), Rb[i:i + 1], Tb[i:i + 1], mi.shared_faces(),
                                 intr[i:i + 1].contiguous(), cc, cfg, tex, vcolors=vcol, pose_cv=pose_cv))
    return {k: torch.cat([o[k] for o in outs], 0) for k in outs[0]}


def _soft_renderers(r, faces_per_pixel, light_location):
    """(MeshRasterizer, MeshRenderer) for faces_per_pixel > 1, as torch_renderer.py:90-108 (depth and
    silhouette) and :132-153 (Phong, PointLights at `light_location`) build them."""
    from .mesh_renderer import (MeshRasterizer, MeshRenderer, PointLights, RasterizationSettings,
                                SoftPhongShader, SoftSilhouetteShader)

    rasterizer = MeshRasterizer(cameras=r._cameras, raster_settings=RasterizationSettings(
        image_size=r._image_size, blur_radius=0.0, faces_per_pixel=faces_per_pixel))
    if light_location is None:
        shader = SoftSilhouetteShader()
    else:
        shader = SoftPhongShader(device=r._device, cameras=r._cameras,
                                 lights=PointLights(device=r._device, location=[list(light_location)]))
    return rasterizer, MeshRenderer(rasterizer=rasterizer, shader=shader)


class DifferentiableRenderer:
    """torch_renderer.py:39-80."""

    def __init__(self, K, image_size, device="cuda:0"):
        assert isinstance(K, torch.Tensor), "[Error] DifferentiableRenderer.__init__: K must be a torch.Tensor"
        if len(K.shape) == 2:
            K = K.unsqueeze(0)
        self._K = K
        if not isinstance(image_size, tuple):
            print("ERROR: DifferentiableRenderer.__init__: image_size must be a tuple, e.g, (720, 1280)")
            raise RuntimeError("image_size must be a tuple")
        self._image_size = image_size
        self._device = device
        self._initialize_perspective_cameras()

    def _initialize_perspective_cameras(self):
        camera_matrix = self._K
        focal_length = torch.stack([camera_matrix[:, 0, 0], camera_matrix[:, 1, 1]], dim=-1)
        principal_point = camera_matrix[:, :2, 2]
        self._cameras = PerspectiveCameras(focal_length=focal_length, principal_point=principal_point,
                                           device=self._device, in_ndc=False,
                                           image_size=torch.tensor([self._image_size]))

    @staticmethod
    def _camera_pose_from_opencv_to_pytorch(R, tvec):
        return opencv_to_pytorch3d(R, tvec)

    def _check_meshes(self, meshes):
        assert isinstance(meshes, Meshes), "[Error] PointRender.render, meshes must be pytorch3d.structures.Meshes"


class DepthRender(DifferentiableRenderer):
    """torch_renderer.py:83-121: relu(zbuf) depth, optional soft silhouette (not binary)."""

    def __init__(self, K, image_size, faces_per_pixel=1, device="cuda:0"):
        super().__init__(K, image_size, device)
        print("INFO: Initializing DepthRender ...")
        self._faces_per_pixel = int(faces_per_pixel)
        if self._faces_per_pixel != 1:
            # K-deep soft path (torch_renderer.py:90-108): modular rasterizer + SoftSilhouetteShader
            self._rasterizer, self._silhouette_renderer = _soft_renderers(self, self._faces_per_pixel, None)

    def render(self, meshes, R, tvec, return_silhouette=False):
        self._check_meshes(meshes)
        if self._faces_per_pixel != 1:
            Rs, ts = self._camera_pose_from_opencv_to_pytorch(R, tvec)
            depths = torch.relu(self._rasterizer(meshes, R=Rs, T=ts).zbuf[..., 0])
            if not return_silhouette:
                return depths
            return depths, self._silhouette_renderer(meshes, R=Rs, T=ts)[..., 3]
        cfg = ShadeConfig(H=self._image_size[0], W=self._image_size[1], want_depth=True,
                          want_sil=bool(return_silhouette), want_rgb=False)
        out = render_mesh_batch(meshes, self._cameras, self._image_size, R, tvec, cfg, pose_cv=True)
        if not return_silhouette:
            return out["depth"]
        return out["depth"], out["sil"]


class ColorRender(DifferentiableRenderer):
    """torch_renderer.py:124-159: SoftPhongShader, PointLights((0,0,-3)), images[..., :3]."""

    def __init__(self, K, image_size, blur_radius=0., faces_per_pixel=1, device="cuda:0"):
        super().__init__(K, image_size, device)
        print("INFO: Initializing ColorRender ...")
        if blur_radius != 0.0:
            # Upstream passes a BlendParams object as RasterizationSettings.blur_radius here
            # (torch_renderer.py:129,137), which cannot rasterize; refuse instead of guessing.
            raise NotImplementedError("ColorRender: blur_radius != 0 is broken in the reference; only 0 is supported")
        self._light_location = (0.0, 0.0, -3.0)
        self._faces_per_pixel = int(faces_per_pixel)
        if self._faces_per_pixel != 1:
            _, self._phong_renderer = _soft_renderers(self, self._faces_per_pixel, self._light_location)

    def render(self, meshes, R, tvec):
        self._check_meshes(meshes)
        if self._faces_per_pixel != 1 or textures_need_modular(meshes):
            if self._faces_per_pixel == 1 and not hasattr(self, "_phong_renderer"):
                _, self._phong_renderer = _soft_renderers(self, 1, self._light_location)
            Rs, ts = self._camera_pose_from_opencv_to_pytorch(R, tvec)
            return self._phong_renderer(meshes, R=Rs, T=ts)[..., :3]
        cfg = ShadeConfig(H=self._image_size[0], W=self._image_size[1], light_location=self._light_location,
                          want_depth=False, want_sil=False, want_rgb=True)
        return render_mesh_batch(meshes, self._cameras, self._image_size, R, tvec, cfg, pose_cv=True)["rgb"]


class DepthColorRender(DifferentiableRenderer):
    """Depth + silhouette + Phong RGB from ONE raster pass (what the reference obtains with
    DepthRender.render(..., return_silhouette=True) followed by ColorRender.render: three passes)."""

    def __init__(self, K, image_size, device="cuda:0"):
        super().__init__(K, image_size, device)
        self._light_location = (0.0, 0.0, -3.0)

    def render(self, meshes, R, tvec):
        self._check_meshes(meshes)
        if textures_need_modular(meshes):
            if not hasattr(self, "_soft"):
                self._soft = (_soft_renderers(self, 1, None), _soft_renderers(self, 1, self._light_location))
            (rast, sil_r), (_, phong_r) = self._soft
            Rs, ts = self._camera_pose_from_opencv_to_pytorch(R, tvec)
            # one raster pass feeds all three (the three renderers' rasterizers are identical)
            frags = rast(meshes, R=Rs, T=ts).materialize()  # the shaders read every field: one pass
            depth = torch.relu(frags.zbuf[..., 0])
            sil = sil_r.shader(frags, meshes, R=Rs, T=ts)[..., 3]
            return depth, sil, phong_r.shader(frags, meshes, R=Rs, T=ts)[..., :3]
        cfg = ShadeConfig(H=self._image_size[0], W=self._image_size[1], light_location=self._light_location)
        out = render_mesh_batch(meshes, self._cameras, self._image_size, R, tvec, cfg, pose_cv=True)
        return out["depth"], out["sil"], out["rgb"]


class _PointRender(DifferentiableRenderer):
    """torch_renderer.py:163-207: PointsRenderer over PointsRasterizationSettings(radius, points_per_pixel) with the
    subclass's compositor. ``render(points, R, tvec, features)`` takes OpenCV poses as DepthRender does and returns
    images[..., :3]; the features come with the call (Pointclouds here holds none)."""
    _compositor = None

    def __init__(self, K, image_size, radius=0.003, points_per_pixel=10, background_color=(0, 0, 0), device="cuda:0"):
        super().__init__(K, image_size, device=device)
        print(f"INFO: Initializing {type(self).__name__} ...")
        from .points_renderer import PointsRasterizationSettings, PointsRasterizer, PointsRenderer

        raster_settings = PointsRasterizationSettings(image_size=self._image_size, radius=radius,
                                                      points_per_pixel=points_per_pixel)
        self._renderer = PointsRenderer(rasterizer=PointsRasterizer(cameras=self._cameras,
                                                                    raster_settings=raster_settings),
                                        compositor=self._compositor(background_color=background_color))

    def render(self, points, R, tvec, features=None):
        from .structures import Pointclouds

        assert isinstance(points, Pointclouds), \
            "[Error] PointRender.render, points must be pytorch3d.structures.Pointclouds"
        Rs, ts = self._camera_pose_from_opencv_to_pytorch(R, tvec)
        return self._renderer(points, features=features, R=Rs, T=ts)[..., :3]


def _alpha_compositor(**kw):
    from .points_renderer import AlphaCompositor

    return AlphaCompositor(**kw)


def _norm_compositor(**kw):
    from .points_renderer import NormWeightedCompositor

    return NormWeightedCompositor(**kw)


class AlphaPointRender(_PointRender):
    """torch_renderer.py:163-184 (AlphaCompositor)."""
    _compositor = staticmethod(_alpha_compositor)


class NormPointRender(_PointRender):
    """torch_renderer.py:186-207 (NormWeightedCompositor)."""
    _compositor = staticmethod(_norm_compositor)


class PulsarPointRender(DifferentiableRenderer):
    """torch_renderer.py:209-230: the Pulsar sphere renderer is not built."""

    def __init__(self, K, image_size, radius=0.003, points_per_pixel=10, device="cuda:0"):
        raise NotImplementedError("PulsarPointRender: the Pulsar renderer is not implemented on the MI355X path")
