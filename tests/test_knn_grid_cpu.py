"""PointGrid / knn_points(grid=) (csrc/mr_grid.hip) without a GPU: the exported names, the C ABI's checks before any
device work, the sizes of the grid buffer and the workspaces, and the Python layer's refusals."""
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


GRID_SYMBOLS = ("mr_point_grid_bytes", "mr_point_grid_build_workspace", "mr_point_grid_build",
                "mr_knn_points_grid_workspace", "mr_knn_points_grid", "mr_point_grid_describe")


def test_names_are_exported(lib):
    from torch_renderer_amd.ops import PointGrid, knn_points

    assert PointGrid is ops.PointGrid and knn_points is ops.knn_points
    for name in ("point_grid_build", "point_grid_describe", "knn_points_grid", "KnnPointsGrid"):
        assert hasattr(kernels, name), name
    assert issubclass(kernels.KnnPointsGrid, kernels._NeighbourDists)
    assert kernels.KnnPointsGrid._backward == kernels.KnnPoints._backward == "mr_knn_points_backward"
    for name in GRID_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    names = {lib.mr_timing_kernel_name(k).decode() for k in range(lib.mr_timing_kernel_count())}
    assert not any("grid" in n for n in names)  # the timing table gained nothing


def test_sizes_are_multiples_of_256_and_zero_out_of_range(lib):
    for N, P in ((1, 1), (1, 3000), (4, 1000), (1, 1000000), (300, 400), (65535, 1)):
        gb, ws = lib.mr_point_grid_bytes(N, P), lib.mr_point_grid_build_workspace(N, P)
        assert gb > 0 and gb % 256 == 0 and ws > 0 and ws % 256 == 0, (N, P, gb, ws)
        # a head per cloud, cell_start over at most P cells, a float4 per point; counters over at most P cells
        assert 16 * N * P <= gb <= 16 * N * P + 4 * N * (P + 1) + 64 * N + 3 * 256, (N, P, gb)
        assert ws <= 4 * N * P + 4 + 256, (N, P, ws)
    for N, P1, P2, K in ((1, 1, 1, 1), (1, 200, 3000, 8), (4, 257, 1000, 32)):
        ws = lib.mr_knn_points_grid_workspace(N, P1, P2, K)
        assert ws > 0 and ws % 256 == 0
    for N, P in ((0, 10), (10, 0), (-1, 10), (70000, 10), (1, 2 ** 31)):
        assert lib.mr_point_grid_bytes(N, P) == 0 and lib.mr_point_grid_build_workspace(N, P) == 0, (N, P)
    for args in ((0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (1, 4, 4, 33), (70000, 4, 4, 1)):
        assert lib.mr_knn_points_grid_workspace(*args) == 0, args


def test_build_rejects_bad_arguments_without_touching_the_gpu(lib):
    one = 1  # any non-NULL pointer value: the checks below return before anything is read
    f = lib.mr_point_grid_build
    gb, ws = lib.mr_point_grid_bytes(2, 100), lib.mr_point_grid_build_workspace(2, 100)
    for args in ((None, 2, 100, None, one, gb, one, ws, None), (one, 2, 100, None, None, gb, one, ws, None),
                 (one, 2, 100, None, one, gb, None, ws, None)):
        assert f(*args) == 1 and b"NULL" in lib.mr_last_error(), args
    assert f(one, 0, 100, None, one, gb, one, ws, None) == 1 and f(one, 2, 0, None, one, gb, one, ws, None) == 1
    assert f(one, 2, -5, None, one, gb, one, ws, None) == 1
    rc = f(one, 70000, 100, None, one, 1 << 40, one, 1 << 40, None)
    assert rc == 3 and b"65535" in lib.mr_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc)
    assert f(one, 2, 100, None, one, gb - 1, one, ws, None) == 4 and b"too small" in lib.mr_last_error()
    assert f(one, 2, 100, None, one, gb, one, ws - 1, None) == 4 and b"too small" in lib.mr_last_error()
    d = lib.mr_point_grid_describe
    assert d(None, 2, 100, None, None, None, None) == 1 and b"NULL" in lib.mr_last_error()
    assert d(one, 0, 100, None, None, None, None) == 1 and d(one, 70000, 100, None, None, None, None) == 3


def test_search_rejects_bad_arguments_without_touching_the_gpu(lib):
    one = 1
    f = lib.mr_knn_points_grid
    gb, ws = lib.mr_point_grid_bytes(1, 4), lib.mr_knn_points_grid_workspace(1, 4, 4, 1)

    def call(p1=one, p2=one, N=1, P1=4, P2=4, grid=one, grid_bytes=gb, norm=2, K=1, dists=one, idx=one, ws_ptr=one,
             ws_bytes=ws):
        return f(p1, p2, N, P1, P2, None, None, grid, grid_bytes, norm, K, dists, idx, None, ws_ptr, ws_bytes, None)

    for kw in ({"p1": None}, {"p2": None}, {"grid": None}, {"dists": None}, {"idx": None}, {"ws_ptr": None}):
        assert call(**kw) == 1 and b"NULL" in lib.mr_last_error(), kw
    for kw in ({"N": 0}, {"P1": 0}, {"P2": 0}, {"K": 0}, {"norm": 3}, {"norm": 0}):
        assert call(**kw) == 1, kw
    assert call(K=0) == 1 and b"K" in lib.mr_last_error()
    rc = call(K=33)
    assert rc == 3 and b"K" in lib.mr_last_error()
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


def test_python_refusals_come_before_any_device_use():
    g = torch.Generator().manual_seed(0)
    p1, p2 = torch.randn(2, 5, 3, generator=g), torch.randn(2, 7, 3, generator=g)
    l2 = torch.tensor([7, 3])
    # CPU tensors: the build and the search are device-only
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.PointGrid(p2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.PointGrid(ops.Pointclouds([p2[0], p2[1, :3]]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.point_grid_build(p2, l2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.knn_points_grid(p1, p2, torch.empty(0, dtype=torch.uint8), K=2)
    grid = _remembered(p2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a fitting grid passes the checks
        ops.knn_points(p1, p2, K=2, grid=grid)
    # the build's own argument errors
    with pytest.raises(ValueError):
        ops.PointGrid(ops.Pointclouds([p2[0], p2[1, :3]]), lengths=l2)
    with pytest.raises(ValueError):
        ops.PointGrid(p2[0])
    with pytest.raises(ValueError):
        ops.PointGrid(p2, lengths=torch.tensor([7]))
    with pytest.raises(ValueError):
        ops.PointGrid([p2])
    with pytest.raises(NotImplementedError):
        kernels.point_grid_build(p2[..., :2])
    # a grid from another tensor, also an equal one and a view of the same memory
    for other in (torch.randn(2, 7, 3, generator=g), p2.clone(), p2.detach(), p2[:, :6]):
        with pytest.raises(ValueError, match="not built from this p2"):
            ops.knn_points(p1, other, K=2, grid=grid)
    # other lengths
    with pytest.raises(ValueError, match="lengths2"):
        ops.knn_points(p1, p2, lengths2=l2, K=2, grid=grid)
    with_l = _remembered(p2, l2)
    with pytest.raises(ValueError, match="lengths2"):
        ops.knn_points(p1, p2, K=2, grid=with_l)
    with pytest.raises(ValueError, match="lengths2"):
        ops.knn_points(p1, p2, lengths2=l2.clone(), K=2, grid=with_l)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.knn_points(p1, p2, lengths2=l2, K=2, grid=with_l)
    l2[1] = 4  # the lengths modified in place since
    with pytest.raises(ValueError, match="lengths2"):
        ops.knn_points(p1, p2, lengths2=l2, K=2, grid=with_l)
    # a Pointclouds' grid fits its padded tensor, with its lengths (without them only if every cloud is full)
    pc = ops.Pointclouds([p2[0], p2[1, :3]])
    pg = _remembered(pc)
    assert pg.lengths is pc.num_points_per_cloud() and not pg.full and pg.shape == (2, 7, 3)
    with pytest.raises(ValueError, match="lengths2"):
        ops.knn_points(p1, pc.points_padded(), K=2, grid=pg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.knn_points(p1, pc.points_padded(), lengths2=pc.num_points_per_cloud(), K=2, grid=pg)
    assert _remembered(ops.Pointclouds(p2)).full
    # a tensor modified in place since the build
    p2.mul_(2.0)
    with pytest.raises(ValueError, match="modified in place"):
        ops.knn_points(p1, p2, K=2, grid=grid)
    # a wrong type for grid=
    for bad in (torch.empty(4, dtype=torch.uint8), "grid", 3):
        with pytest.raises(ValueError, match="PointGrid"):
            ops.knn_points(p1, p2, K=2, grid=bad)
    # the other arguments are checked as without a grid
    fresh = _remembered(p2)
    with pytest.raises(ValueError):
        ops.knn_points(p1, p2, K=0, grid=fresh)
    with pytest.raises(NotImplementedError):
        ops.knn_points(p1, p2, K=33, grid=fresh)
    with pytest.raises(ValueError):
        ops.knn_points(p1, p2, norm=3, grid=fresh)
