"""estimate_pointcloud_normals / ball_query through a PointGrid (k_frames_grid of csrc/mr_normals.hip,
k_ball_query_grid of csrc/mr_ballquery.hip) without a GPU: the exported names, the C ABI's checks before any device
work, the workspace sizes, and the Python layer's refusals."""
import os

import pytest
import torch

from torch_renderer_amd import _lib, kernels, ops


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from torch_renderer_amd import _build

        _build.build()
    return _lib.load()


NEW_SYMBOLS = {"mr_point_frames_grid_workspace": 3, "mr_point_frames_grid": 15, "mr_ball_query_grid_workspace": 4,
               "mr_ball_query_grid": 17}


def test_names_are_exported(lib):
    for name, nargs in NEW_SYMBOLS.items():
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    for name in ("ball_query_grid", "BallQueryGrid", "BALL_GRID_MAX_K"):
        assert hasattr(kernels, name), name
    assert issubclass(kernels.BallQueryGrid, kernels._NeighbourDists)
    assert kernels.BallQueryGrid._backward == kernels.BallQuery._backward == "mr_ball_query_backward"
    assert kernels.BALL_GRID_MAX_K == 64
    names = {lib.mr_timing_kernel_name(k).decode() for k in range(lib.mr_timing_kernel_count())}
    assert not any("grid" in n for n in names)  # the timing table gained nothing


def test_workspaces_are_multiples_of_256_and_zero_out_of_range(lib):
    for N, P, K in ((1, 9, 8), (1, 200000, 16), (300, 2000, 50), (256, 70, 64), (1, 3, 2)):
        ws = lib.mr_point_frames_grid_workspace(N, P, K)
        assert ws > 0 and ws % 256 == 0, (N, P, K)
    for args in ((1, 100, 1), (1, 100, 65), (1, 50, 50), (1, 8, 16), (0, 100, 8), (70000, 100, 8), (1, 2 ** 31, 8)):
        assert lib.mr_point_frames_grid_workspace(*args) == 0, args
    for N, P1, P2, K in ((1, 1, 1, 1), (1, 200, 3000, 8), (32, 512, 4096, 32), (1, 10, 10, 64)):
        ws = lib.mr_ball_query_grid_workspace(N, P1, P2, K)
        assert ws > 0 and ws % 256 == 0, (N, P1, P2, K)
    for args in ((0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (1, 4, 4, 65), (1, 4, 4, 500), (70000, 4, 4, 1)):
        assert lib.mr_ball_query_grid_workspace(*args) == 0, args


def test_frames_grid_rejects_bad_arguments_without_touching_the_gpu(lib):
    one = 1  # any non-NULL pointer value: the checks below return before anything is read
    f = lib.mr_point_frames_grid
    gb, ws = lib.mr_point_grid_bytes(2, 100), lib.mr_point_frames_grid_workspace(2, 100, 8)

    def call(points=one, N=2, P=100, grid=one, grid_bytes=gb, K=8, flags=1, cur=one, frm=one, ws_ptr=one, ws_bytes=ws):
        return f(points, N, P, None, grid, grid_bytes, K, flags, cur, frm, None, None, ws_ptr, ws_bytes, None)

    for kw in ({"points": None}, {"grid": None}, {"cur": None}, {"frm": None}, {"ws_ptr": None}):
        assert call(**kw) == 1 and b"NULL" in lib.mr_last_error(), kw
    for kw in ({"N": 0}, {"P": 0}, {"K": 1}, {"K": 0}, {"K": 64, "P": 64}, {"P": 8}):
        assert call(**kw) == 1, kw
    assert call(K=1) == 1 and b"K" in lib.mr_last_error()
    assert call(flags=2) == 1 and b"flags" in lib.mr_last_error()
    rc = call(K=65, P=1000, grid_bytes=1 << 40)
    assert rc == 3 and b"K" in lib.mr_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc)
    assert call(N=70000, grid_bytes=1 << 40) == 3
    assert call(grid_bytes=gb - 1) == 4 and b"too small" in lib.mr_last_error()
    assert call(ws_bytes=ws - 1) == 4 and b"too small" in lib.mr_last_error()


def test_ball_grid_rejects_bad_arguments_without_touching_the_gpu(lib):
    one = 1
    f = lib.mr_ball_query_grid
    gb, ws = lib.mr_point_grid_bytes(1, 4), lib.mr_ball_query_grid_workspace(1, 4, 4, 2)

    def call(p1=one, p2=one, N=1, P1=4, P2=4, grid=one, grid_bytes=gb, radius=0.5, K=2, dists=one, idx=one, ws_ptr=one,
             ws_bytes=ws):
        return f(p1, p2, N, P1, P2, None, None, grid, grid_bytes, radius, K, dists, idx, None, ws_ptr, ws_bytes, None)

    for kw in ({"p1": None}, {"p2": None}, {"grid": None}, {"dists": None}, {"idx": None}, {"ws_ptr": None}):
        assert call(**kw) == 1 and b"NULL" in lib.mr_last_error(), kw
    for kw in ({"N": 0}, {"P1": 0}, {"P2": 0}, {"K": 0}):
        assert call(**kw) == 1, kw
    for radius in (-0.5, float("inf"), float("nan")):
        assert call(radius=radius) == 1 and b"radius" in lib.mr_last_error(), radius
    rc = call(K=65)
    assert rc == 3 and b"K" in lib.mr_last_error() and b"64" in lib.mr_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc)
    assert call(N=70000, grid_bytes=1 << 40) == 3
    assert call(grid_bytes=gb - 1) == 4 and b"too small" in lib.mr_last_error()
    assert call(ws_bytes=ws - 1) == 4 and b"too small" in lib.mr_last_error()


def _remembered(points, lengths=None):
    """A PointGrid that remembers its source and has no buffer: what a refusal needs, without a device."""
    grid = ops.PointGrid.__new__(ops.PointGrid)
    grid._remember(points, lengths)
    grid.buffer = torch.empty(0, dtype=torch.uint8)
    return grid


def test_ball_query_refusals_come_before_any_device_use():
    g = torch.Generator().manual_seed(0)
    p1, p2 = torch.randn(2, 5, 3, generator=g), torch.randn(2, 7, 3, generator=g)
    l2 = torch.tensor([7, 3])
    grid = _remembered(p2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a fitting grid passes the checks
        ops.ball_query(p1, p2, K=4, grid=grid)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.ball_query_grid(p1, p2, torch.empty(0, dtype=torch.uint8), K=2)
    # a wrong type for grid=
    for bad in (torch.empty(4, dtype=torch.uint8), "grid", 3):
        with pytest.raises(ValueError, match="PointGrid"):
            ops.ball_query(p1, p2, K=4, grid=bad)
    # a grid from another tensor, also an equal one and a view of the same memory
    for other in (torch.randn(2, 7, 3, generator=g), p2.clone(), p2.detach(), p2[:, :6]):
        with pytest.raises(ValueError, match="ball_query: the grid was not built from this p2"):
            ops.ball_query(p1, other, K=4, grid=grid)
    # other lengths
    with pytest.raises(ValueError, match="ball_query: the grid was not built with these lengths2"):
        ops.ball_query(p1, p2, lengths2=l2, K=4, grid=grid)
    with_l = _remembered(p2, l2)
    with pytest.raises(ValueError, match="lengths2"):
        ops.ball_query(p1, p2, K=4, grid=with_l)
    with pytest.raises(ValueError, match="lengths2"):
        ops.ball_query(p1, p2, lengths2=l2.clone(), K=4, grid=with_l)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ball_query(p1, p2, lengths2=l2, K=4, grid=with_l)
    # K > 64 with a grid names the limit; the default K = 500 is above it
    with pytest.raises(NotImplementedError, match="64"):
        ops.ball_query(p1, p2, K=65, grid=grid)
    with pytest.raises(NotImplementedError, match="64"):
        ops.ball_query(p1, p2, grid=grid)
    with pytest.raises(NotImplementedError, match="64"):
        kernels.ball_query_grid(p1, p2, torch.empty(0, dtype=torch.uint8), K=65)
    # the other arguments are checked as without a grid
    for kw in ({"K": 0}, {"radius": -1.0}, {"radius": float("inf")}, {"radius": float("nan")},
               {"lengths1": torch.tensor([5])}):
        with pytest.raises(ValueError):
            ops.ball_query(p1, p2, **{"K": 4, **kw})
        with pytest.raises(ValueError):
            ops.ball_query(p1, p2, **{"K": 4, **kw}, grid=grid)
    with pytest.raises(ValueError):
        ops.ball_query(p1[0], p2, K=4, grid=grid)
    # knn_points' messages are what they were
    with pytest.raises(ValueError, match="knn_points: the grid was not built from this p2"):
        ops.knn_points(p1, p2.clone(), K=2, grid=grid)
    # a tensor modified in place since the build
    p2.mul_(2.0)
    with pytest.raises(ValueError, match="modified in place"):
        ops.ball_query(p1, p2, K=4, grid=grid)


@pytest.mark.parametrize("fn", [ops.estimate_pointcloud_local_coord_frames, ops.estimate_pointcloud_normals])
def test_frames_refusals_come_before_any_device_use(fn):
    g = torch.Generator().manual_seed(1)
    p = torch.randn(2, 12, 3, generator=g)
    grid = _remembered(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a fitting grid passes the checks
        fn(grid, 5)
    # argument errors are those of the call with the points
    for K, err in ((1, ValueError), (65, NotImplementedError), (12, ValueError), (20, ValueError)):
        with pytest.raises(err) as with_points:
            fn(p, K)
        with pytest.raises(err) as with_grid:
            fn(grid, K)
        assert str(with_points.value) == str(with_grid.value)
    pc = ops.Pointclouds([p[0], p[1, :4]])
    with pytest.raises(ValueError) as with_points:
        fn(pc, 5)  # a cloud of 4 points
    with pytest.raises(ValueError) as with_grid:
        fn(_remembered(pc), 5)
    assert str(with_points.value) == str(with_grid.value)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(_remembered(pc), 3)
    needs = torch.randn(1, 12, 3, generator=g).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        fn(_remembered(needs), 5)
    # the kernels layer: a grid that is no tensor, visited without a grid
    with pytest.raises(ValueError, match="grid"):
        kernels.point_frames(p, None, 5, grid="grid")
    with pytest.raises(ValueError, match="visited"):
        kernels.point_frames(p, None, 5, visited=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.point_frames(p, None, 5, grid=torch.empty(0, dtype=torch.uint8))
    # a freed tensor, a tensor modified in place
    gone = _remembered(torch.randn(1, 12, 3, generator=g))
    with pytest.raises(ValueError, match="freed"):
        fn(gone, 5)
    p.add_(1.0)
    with pytest.raises(ValueError, match="modified in place"):
        fn(grid, 5)


def test_plane_icp_with_a_grid_and_no_normals_reaches_the_grid_route():
    g = torch.Generator().manual_seed(2)
    X, Y = torch.randn(1, 10, 3, generator=g), torch.randn(1, 12, 3, generator=g)
    grid = _remembered(Y)
    with pytest.raises(ValueError) as with_grid:  # the normals' own error propagates: 12 points, K = 16
        ops.iterative_closest_point_to_plane(X, grid, None, neighborhood_size=16)
    with pytest.raises(ValueError) as with_points:
        ops.iterative_closest_point_to_plane(X, Y, None, neighborhood_size=16)
    assert str(with_grid.value) == str(with_points.value)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.iterative_closest_point_to_plane(X, grid, None, neighborhood_size=5)
