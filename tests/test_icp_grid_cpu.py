"""The ICP loops through a PointGrid (mr_icp_iterate_grid / mr_icp_plane_iterate_grid, k_icp_nn_grid of
csrc/mr_points.hip) without a GPU: the exported names and argument counts, the C ABI's checks before any launch, and
the Python layer's refusals with a PointGrid as ``Y``."""
import ctypes
import gc
import inspect
import os
import re

import pytest
import torch

from torch_renderer_amd import Pointclouds, _lib, kernels, ops
from torch_renderer_amd.ops import SimilarityTransform, iterative_closest_point, iterative_closest_point_to_plane

MR_EINVAL, MR_EUNSUPPORTED, MR_EWORKSPACE = 1, 3, 4
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355r.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from torch_renderer_amd import _build

        _build.build()
    return _lib.load()


def test_symbols_are_exported_with_the_expected_argument_counts(lib):
    with open(HEADER) as fh:
        src = fh.read()
    for name, nargs, sibling in (("mr_icp_iterate_grid", 21, "mr_icp_iterate"),
                                 ("mr_icp_plane_iterate_grid", 22, "mr_icp_plane_iterate")):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs == len(getattr(lib, sibling).argtypes) + 3
        decl = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl is not None, name
        params = [a.strip() for a in decl.group(1).split(",")]
        assert len(params) == nargs
        assert "const void* grid" in params and "size_t grid_bytes" in params and "uint64_t* visited" in params
        assert params[-3:] == ["void* ws", "size_t ws_bytes", "void* stream"]
    # the siblings' signatures are what they were
    assert len(lib.mr_icp_iterate.argtypes) == 18 and len(lib.mr_icp_plane_iterate.argtypes) == 19
    assert "mr_icp_iterate" in src and "the same key in `ws`" in src
    for fn in (kernels.icp, kernels.icp_plane):
        p = inspect.signature(fn).parameters
        assert p["grid"].default is None and p["visited"].default is None and "status_batch" in p


def _calls(lib, buf):
    """(icp, plane): the two entry points on a 2 x 4 -> 4 batch with every pointer `p` (host memory that is never
    dereferenced), one keyword per argument under test."""
    p = ctypes.addressof(buf)
    gb = lib.mr_point_grid_bytes(2, 4)

    def icp(**k):
        N, P2 = k.get("N", 2), k.get("P2", 4)
        return lib.mr_icp_iterate_grid(k.get("x", p), k.get("y", p), N, k.get("P1", 4), P2, None, None, k.get("grid", p),
                                       k.get("gb", gb), k.get("flags", 0), 1e-6, k.get("max_it", 10), k.get("its", 1),
                                       k.get("rts", p), k.get("hist", p), k.get("rmse", p), k.get("status", p),
                                       k.get("visited", None), k.get("ws", p), k.get("wsb", 1 << 40), None)

    def plane(**k):
        N, P2 = k.get("N", 2), k.get("P2", 4)
        return lib.mr_icp_plane_iterate_grid(k.get("x", p), k.get("y", p), k.get("yn", p), N, k.get("P1", 4), P2, None,
                                             None, k.get("grid", p), k.get("gb", gb), k.get("r2", float("inf")), 1e-6,
                                             k.get("max_it", 10), k.get("its", 1), k.get("rts", p), k.get("hist", p),
                                             k.get("rmse", p), k.get("status", p), k.get("visited", None),
                                             k.get("ws", p), k.get("wsb", 1 << 40), None)

    return icp, plane, gb


def test_abi_rejects_bad_arguments_without_touching_the_gpu(lib):
    """Every check returns before any launch (there is no GPU here): the grid argument under mr_knn_points_grid's
    contract, everything else as the siblings."""
    buf = ctypes.create_string_buffer(256)
    icp, plane, gb = _calls(lib, buf)

    def err():
        return lib.mr_last_error()

    for call in (icp, plane):
        assert call(grid=None) == MR_EINVAL and b"grid is NULL" in err()
        assert call(gb=gb - 1) == MR_EWORKSPACE and b"grid buffer too small" in err()
        assert call(gb=0) == MR_EWORKSPACE
        assert call(gb=gb, its=0) == 0 and call(gb=gb + 256, its=0) == 0  # nothing to enqueue
        for key in ("x", "y", "rts", "hist", "rmse", "status", "ws"):
            assert call(**{key: None}) == MR_EINVAL and b"NULL" in err(), key
        assert call(N=0) == MR_EINVAL and b">= 1" in err()
        assert call(P1=0) == MR_EINVAL and call(P2=0) == MR_EINVAL and call(N=-3) == MR_EINVAL
        assert call(N=70000, gb=1 << 40) == MR_EUNSUPPORTED and b"65535" in err()
        assert call(max_it=0) == MR_EINVAL and b"max_iterations" in err()
        assert call(its=-1) == MR_EINVAL
        assert call(wsb=16) == MR_EWORKSPACE and b"too small" in err()
        # the sizes are judged before the grid, the grid before the workspace
        assert call(N=0, grid=None) == MR_EINVAL and b">= 1" in err()
        assert call(grid=None, wsb=16) == MR_EINVAL and call(gb=gb - 1, wsb=16) == MR_EWORKSPACE and b"grid" in err()
    assert icp(flags=4) == MR_EINVAL and b"flags" in err()
    assert icp(flags=3, its=0) == 0
    assert plane(yn=None) == MR_EINVAL and b"NULL" in err()
    for r2 in (0.0, -1.0, float("nan")):
        assert plane(r2=r2) == MR_EINVAL and b"max_dist2" in err()
    assert plane(r2=0.25, its=0) == 0
    with pytest.raises(NotImplementedError):
        _lib.check(icp(N=70000, gb=1 << 40))


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 300, 200), (300, 2000, 400)])
def test_entry_points_enforce_the_size_queries_they_share(lib, shape):
    """The workspaces are the siblings' (mr_icp_workspace, mr_icp_plane_workspace), the grid buffer is
    mr_point_grid_bytes(N, P2): one byte less than either is refused before any device work."""
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    N, P1, P2 = shape
    gb = lib.mr_point_grid_bytes(N, P2)

    def icp(g, w):
        return lib.mr_icp_iterate_grid(p, p, N, P1, P2, None, None, p, g, 0, 1e-6, 10, 0, p, p, p, p, None, p, w, None)

    def plane(g, w):
        return lib.mr_icp_plane_iterate_grid(p, p, p, N, P1, P2, None, None, p, g, float("inf"), 1e-6, 10, 0, p, p, p, p,
                                             None, p, w, None)

    for call, need in ((icp, lib.mr_icp_workspace(N, P1, P2)), (plane, lib.mr_icp_plane_workspace(N, P1, P2))):
        assert call(gb, need) == 0
        assert call(gb, need - 1) == MR_EWORKSPACE and b"workspace too small" in lib.mr_last_error()
        assert call(gb - 1, need) == MR_EWORKSPACE and b"grid buffer too small" in lib.mr_last_error()


def _remembered(points, lengths=None):
    """A PointGrid that remembers its source and has no buffer: what a refusal needs, without a device."""
    grid = ops.PointGrid.__new__(ops.PointGrid)
    grid._remember(points, lengths)
    grid.buffer = torch.empty(0, dtype=torch.uint8)
    return grid


def _clouds(N=2, P1=5, P2=7, D=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, P1, D, generator=g), torch.randn(N, P2, D, generator=g), torch.randn(N, P2, D, generator=g)


def _both(x, grid, n, **kw):
    """The two calls with ``grid`` as Y."""
    return (lambda: iterative_closest_point(x, grid, **kw), lambda: iterative_closest_point_to_plane(x, grid, n, **kw))


def test_point_grid_hands_back_what_it_was_built_from():
    x, y, _ = _clouds()
    l2 = torch.tensor([7, 3])
    p, l, c = _remembered(y).points()
    assert p is y and l is None and c is None
    p, l, c = _remembered(y, l2).points()
    assert p is y and l is l2 and c is None
    pc = Pointclouds([y[0], y[1, :3]])
    p, l, c = _remembered(pc).points()
    assert p is pc.points_padded() and l is pc.num_points_per_cloud() and c == [7, 3]
    g = _remembered(y, l2)
    l2[1] = 4  # the lengths modified in place since
    with pytest.raises(ValueError, match="modified in place"):
        g.points()


def test_a_stale_grid_is_refused_by_both_ops():
    x, y, n = _clouds()
    grid = _remembered(y)
    for call in _both(x, grid, n):  # a fitting grid passes every check, up to the device
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    y.mul_(2.0)
    for call in _both(x, grid, n):
        with pytest.raises(ValueError, match="modified in place"):
            call()
    fresh = torch.randn(2, 7, 3)
    grid = _remembered(fresh)
    del fresh
    gc.collect()
    for call in _both(x, grid, n):
        with pytest.raises(ValueError, match="freed"):
            call()
    with pytest.raises(ValueError, match="freed"):
        iterative_closest_point_to_plane(x, grid)  # also where the normals would be estimated from the points


def test_argument_errors_are_those_of_the_call_with_points():
    x, y, n = _clouds()
    grid = _remembered(y)
    for call in _both(x[:1], grid, n):
        with pytest.raises(ValueError, match="same number of batches and data dimensions"):
            call()
    x2, y2, n2 = _clouds(D=2)
    for call in _both(x2, grid, n):
        with pytest.raises(ValueError, match="same number of batches and data dimensions"):
            call()
    for call in _both(x2, _remembered(y2), n2):
        with pytest.raises(NotImplementedError, match="D = 3"):
            call()
    good = SimilarityTransform(torch.eye(3)[None].repeat(2, 1, 1), torch.zeros(2, 3), torch.ones(2))
    for call in _both(x, grid, n, init_transform=(good.R[:1], good.T, good.s)):
        with pytest.raises(ValueError, match="The initial transformation init_transform has to be"):
            call()
    for bad in (n[:, :6], n[:1], n[..., :2], n[0], "normals"):
        with pytest.raises(ValueError, match="Y_normals"):
            iterative_closest_point_to_plane(x, grid, bad)
    pc = Pointclouds([y[0], y[1, :4]])
    with pytest.raises(ValueError, match="Y_normals"):  # the padded shape of the grid's points
        iterative_closest_point_to_plane(x, _remembered(pc), n[:, :4])
    with pytest.raises(ValueError, match="max_correspondence_distance"):
        iterative_closest_point_to_plane(x, grid, n, max_correspondence_distance=0.0)
    for call in _both(x.clone().requires_grad_(True), grid, n):
        with pytest.raises(NotImplementedError, match="requires grad"):
            call()
    yg = y.clone().requires_grad_(True)
    for call in _both(x, _remembered(yg), n):
        with pytest.raises(NotImplementedError, match="requires grad"):
            call()
    # the counts of a Pointclouds' grid: an empty target beside a source that is not
    empty = Pointclouds([y[0], y[1, :0]])
    for call in _both(Pointclouds([x[0], x[1, :2]]), _remembered(empty), n):
        with pytest.raises(ValueError, match="target cloud is empty"):
            call()
    for call in _both(Pointclouds([x[0], x[1, :0]]), _remembered(empty), n):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # the normals' own error, from the grid's points: 7 points, K = 50
    with pytest.raises(ValueError, match="neighborhood_size"):
        iterative_closest_point_to_plane(x, grid)
    with pytest.raises(ValueError, match="neighborhood_size"):
        iterative_closest_point_to_plane(x, _remembered(pc), neighborhood_size=5)
    with pytest.raises(NotImplementedError, match="verbose"):
        iterative_closest_point(x, grid, verbose=True)
    with pytest.raises(TypeError):
        iterative_closest_point(x, y, grid=grid)  # Y carries the grid: there is no keyword


def test_kernel_level_refusals():
    x, y, n = _clouds()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.icp(x, y, grid=torch.empty(0, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.icp_plane(x, y, n, grid=torch.empty(0, dtype=torch.uint8))
