"""Host runtime of the C ABI, without a GPU: every entry point that takes a workspace size enforces the size its
query reports (the query and the entry point read one layout), the timing table's names are unique and complete,
and the library's translation units share one error text. Every check here fails before the first memset or
launch: the pointers are host memory that is never dereferenced."""
import ctypes
import os

import pytest

from torch_renderer_amd import _lib

MR_EINVAL, MR_EWORKSPACE = 1, 4

# (N, F = V, H = W, P): the smallest valid shape and the headline's
SHAPES = {"smallest": (1, 1, 8, 1), "headline": (64, 5856, 512, 1000)}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from torch_renderer_amd import _build

        _build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(256)
    yield ctypes.addressof(buf)  # non-NULL, never dereferenced
    del buf


def settings(S, K=1):
    s = _lib.MrRasterSettings()
    s.H, s.W, s.faces_per_pixel, s.blur_radius = S, S, K, 0.0
    return s


def mesh_and_shade(p, F, flags):
    m = _lib.MrMesh()
    m.verts = m.faces = m.vadj_ptr = m.vadj = p
    m.V = m.F = F
    sp = _lib.MrShadeParams()
    sp.light_kind, sp.out_flags, sp.rgb_channels = 1, flags, 3  # ambient light: no normals, no camera centres
    sp.sigma_rgb = sp.gamma = sp.sigma_sil = 1e-4
    sp.znear, sp.zfar = 1.0, 100.0
    return m, sp


ALL_OUT = _lib.MR_OUT_DEPTH | _lib.MR_OUT_SIL | _lib.MR_OUT_RGB


# Each case: (size query, call taking ws_bytes) for one shape; `p` stands for every pointer argument.
def rasterize_meshes(lib, p, N, F, S, P):
    s = settings(S)
    return (lib.mr_rasterize_meshes_workspace(N, N * F, S, S, 0),
            lambda b: lib.mr_rasterize_meshes(p, p, p, N, N * F, ctypes.byref(s), p, p, p, p, p, b, None))


def rasterize_meshes_world(lib, p, N, F, S, P):
    s, ps = settings(S), _lib.MrPoses(p, 0, p, 0, p, 0)
    return (lib.mr_rasterize_meshes_world_workspace(N, F, S, S, 0),
            lambda b: lib.mr_rasterize_meshes_world(p, F, p, F, ctypes.byref(ps), N, ctypes.byref(s), p, p, p, p, p, p,
                                                    p, b, None))


def soft_silhouette_forward(lib, p, N, F, S, P):
    s, ps = settings(S, K=2), _lib.MrPoses(p, 0, p, 0, p, 0)
    return (lib.mr_soft_silhouette_workspace(N, F, S, S, 2, 0),
            lambda b: lib.mr_soft_silhouette_forward(p, F, p, F, ctypes.byref(ps), N, ctypes.byref(s), 1e-4, p, p, p, p,
                                                     b, None))


def render_forward_like(entry):
    def case(lib, p, N, F, S, P):
        s = settings(S)
        m, sp = mesh_and_shade(p, F, ALL_OUT)
        tail = (N, None, 0, ctypes.byref(s), ctypes.byref(sp), p, p, p, None, p)
        if entry == "mr_render_forward_poses":
            head = (ctypes.byref(m), ctypes.byref(_lib.MrPoses(p, 0, p, 0, p, 0)), p)
        elif entry == "mr_render_forward_opencv":
            head = (ctypes.byref(m), ctypes.byref(_lib.MrOpencvPoses(p, 0, p, 0, p, 0)), p)
        else:
            head = (ctypes.byref(m), p)
        return (lib.mr_render_workspace(N, F, S, S, 0), lambda b: getattr(lib, entry)(*head, *tail, b, None))

    case.__name__ = entry[3:]
    return case


def render_backward_like(entry):
    def case(lib, p, N, F, S, P):
        s = settings(S)
        m, sp = mesh_and_shade(p, F, ALL_OUT)
        grads = (p, p, p) if entry == "mr_render_backward_opencv" else (p, p)  # gverts, then gviews or gR, gt
        return (lib.mr_render_backward_workspace(N, F, F, S, S),
                lambda b: getattr(lib, entry)(ctypes.byref(m), None, p, N, None, 0, ctypes.byref(s), ctypes.byref(sp), p,
                                              p, p, p, p, b, *grads, None, None))

    case.__name__ = entry[3:]
    return case


def shade_fragments_forward(lib, p, N, F, S, P):
    m, sp = mesh_and_shade(p, F, _lib.MR_OUT_RGB)
    return (lib.mr_shade_fragments_workspace(F),
            lambda b: lib.mr_shade_fragments_forward(ctypes.byref(m), p, p, p, p, N, S, S, 2, None, 0, ctypes.byref(sp), p,
                                                     p, b, None))


def shade_fragments_backward(lib, p, N, F, S, P):
    m, sp = mesh_and_shade(p, F, _lib.MR_OUT_RGB)
    return (lib.mr_shade_fragments_backward_workspace(F, F),
            lambda b: lib.mr_shade_fragments_backward(ctypes.byref(m), None, p, p, p, p, N, S, S, 2, None, 0,
                                                      ctypes.byref(sp), p, p, p, b, p, p, p, p, None, None, None, 0, None))


def pose_loss_forward(lib, p, N, F, S, P):
    npix = N * S * S
    return (lib.mr_pose_loss_workspace(npix),
            lambda b: lib.mr_pose_loss_forward(p, p, 1, p, 3, p, p, p, npix, 0.1, 1.0, p, p, b, None))


def pose_loss_forward_grad(lib, p, N, F, S, P):
    npix = N * S * S
    return (lib.mr_pose_loss_workspace(npix),
            lambda b: lib.mr_pose_loss_forward_grad(p, p, 1, p, 3, p, p, p, npix, 0.1, 1.0, p, p, p, b, p, p, p, None))


def mesh_priors_forward(lib, p, N, F, S, P):
    V, E, Pr = F, (3 * F + 1) // 2, (3 * F + 1) // 2
    return (lib.mr_mesh_priors_workspace(V, E, Pr),
            lambda b: lib.mr_mesh_priors_forward(p, V, p, p, E, p, p, p, p, p, Pr, 0.0, 7, 1, p, p, b, None))


def nearest_points(lib, p, N, F, S, P):
    return (lib.mr_nearest_points_workspace(N, P, P),
            lambda b: lib.mr_nearest_points(p, p, N, P, P, None, None, 2, p, p, p, p, p, b, None))


def chamfer_forward(lib, p, N, F, S, P):
    return (lib.mr_chamfer_workspace(N, P, P),
            lambda b: lib.mr_chamfer_forward(p, p, N, P, P, None, None, None, 2, 3, p, p, p, p, p, b, None))


def chamfer_backward(lib, p, N, F, S, P):
    return (lib.mr_chamfer_backward_workspace(N, P, P),
            lambda b: lib.mr_chamfer_backward(p, p, N, P, P, 2, 3, p, p, p, p, p, p, p, b, None))


def sample_points_backward(lib, p, N, F, S, P):
    return (lib.mr_sample_points_backward_workspace(F),
            lambda b: lib.mr_sample_points_backward(F, p, F, p, p, N * P, p, p, p, b, None))


CASES = [rasterize_meshes, rasterize_meshes_world, soft_silhouette_forward, render_forward_like("mr_render_forward"),
         render_forward_like("mr_render_forward_poses"), render_forward_like("mr_render_forward_opencv"),
         render_forward_like("mr_render_reshade"), render_backward_like("mr_render_backward"),
         render_backward_like("mr_render_backward_opencv"), shade_fragments_forward, shade_fragments_backward,
         pose_loss_forward, pose_loss_forward_grad, mesh_priors_forward, nearest_points, chamfer_forward,
         chamfer_backward, sample_points_backward]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_entry_point_enforces_its_workspace_query(lib, p, case, shape):
    """One byte less than the queried size is refused with MR_EWORKSPACE and a "too small" text, by the entry
    point's own reading of the layout, before any device work. (That the queried size is enough is what the GPU
    suite shows: the Python wrappers allocate exactly that size.)"""
    need, call = case(lib, p, *SHAPES[shape])
    assert need > 0 and need % 256 == 0
    rc = call(need - 1)
    assert rc == MR_EWORKSPACE, (rc, lib.mr_last_error())
    assert b"too small" in lib.mr_last_error()


LIVE_KERNEL_NAMES = {
    "k_bin_count", "k_bin_scan", "k_bin_fill", "k_tile_raster", "k_shade<0>", "k_shade<1>", "k_raster_bwd",
    "k_rt_vgrad_b", "k_vgrad_b", "k_vertex_normals", "k_project_faces", "k_project_faces_bwd", "k_shade_rec",
    "k_fill<0>", "k_raster_k", "k_bwd_fused", "k_rt_vgrad_a", "k_frag_shade_fwd", "k_frag_shade_bwd", "k_setup_zero",
    "k_bin_rect", "k_bin_view", "k_band_bucket", "k_pose_loss_fused", "k_pose_loss_scale", "k_unit_order"}


def test_timing_names_are_unique_and_complete(lib):
    """bench.py, tools/collect_profiles.py and the profiles look kernels up by these strings."""
    n = lib.mr_timing_kernel_count()
    names = [lib.mr_timing_kernel_name(k).decode() for k in range(n)]
    assert all(names) and len(set(names)) == n
    assert len(LIVE_KERNEL_NAMES) == 26 and set(names) == LIVE_KERNEL_NAMES
    assert lib.mr_timing_kernel_name(n) == b"" and lib.mr_timing_kernel_name(-1) == b""


def test_one_error_text_across_translation_units(lib, p):
    """mr_points.hip, mr_priors.hip and mr_raster.hip write the one text mr_last_error() returns; a formatted
    value survives."""
    big = 1 << 40
    assert lib.mr_nearest_points(p, p, 0, 4, 4, None, None, 2, p, p, p, p, p, big, None) == MR_EINVAL
    assert lib.mr_last_error() == b"nearest points: N, P1 and P2 must be >= 1"
    s = settings(8)
    assert lib.mr_rasterize_meshes(p, p, p, 0, 1, ctypes.byref(s), p, p, p, p, p, big, None) == MR_EINVAL
    assert lib.mr_last_error() == b"num_meshes must be in [1, 65535] (got 0)"
    assert lib.mr_mesh_priors_forward(p, 1, p, p, 1, p, p, p, p, p, 1, 0.0, 8, 1, p, p, big, None) == MR_EINVAL
    assert b"unknown bits in terms" in lib.mr_last_error()
    assert lib.mr_chamfer_forward(p, p, 1, 4, 4, None, None, None, 3, 3, p, p, p, p, p, big, None) == MR_EINVAL
    assert lib.mr_last_error() == b"chamfer: norm must be 1 or 2"
