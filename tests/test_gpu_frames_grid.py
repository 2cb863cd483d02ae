"""estimate_pointcloud_local_coord_frames / estimate_pointcloud_normals through a PointGrid on the MI355X
(k_frames_grid of csrc/mr_normals.hip): curvatures, frames and cov bitwise those of the brute-force call on the same
points, lengths, K and flags, which test_gpu_normals.py holds to the float64 restatement of tests/normals_ref.py.

* the clouds of test_gpu_normals.py at every bucket and both sign rules, K = 2 .. 64;
* the covariance against the restatement itself (1e-4 trace(C_ref) per entry: it pins the neighbour set);
* clouds chosen against a grid: a large offset, a planar cloud, a far outlier, a lattice lying on the cell faces with
  every point twice, coincident and collinear points, more cells than the scan workgroup has threads, P = K + 1;
* the grid is really used (the counter of evaluated distances); determinism; padded rows;
* the public functions with a PointGrid in place of the cloud, HIP graph capture of build + frames, and
  iterative_closest_point_to_plane(X, grid, None), whose normals now come through the grid.
"""
import functools

import numpy as np
import pytest
import torch

from tests import normals_ref as NR
from tests.test_gpu_normals import cloud, ref  # the clouds and one cached reference per (cloud, K) for both modules
from torch_renderer_amd import kernels
from torch_renderer_amd.ops import (PointGrid, estimate_pointcloud_local_coord_frames, estimate_pointcloud_normals,
                                    iterative_closest_point_to_plane)
from torch_renderer_amd.structures import Pointclouds

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KS = (2, 5, 8, 9, 16, 32, 33, 50, 64)


def _rand(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def _both(pts, lengths, K, disambiguate, visited=None):
    """((cur, frm, cov) without a grid, the same through a grid built here), on the device."""
    pts = pts.to(DEV)
    l = None if lengths is None else lengths.to(DEV)
    plain = kernels.point_frames(pts, l, K, disambiguate, return_cov=True)
    grid = kernels.point_grid_build(pts, l)
    through = kernels.point_frames(pts, l, K, disambiguate, return_cov=True, grid=grid, visited=visited)
    torch.cuda.synchronize()
    return plain, through


def _assert_bitwise(tag, plain, through):
    for name, a, b in zip(("curvatures", "frames", "cov"), plain, through):
        assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape, (tag, name)
        diff = (a.view(torch.int32) != b.view(torch.int32))
        assert not diff.any(), (tag, name, int(diff.sum()))


# --------------------------------------------------------------------------- bitwise against the brute-force call
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", ["sphere300", "sphere1100", "cow", "batch70"])
def test_frames_grid_bitwise(name, K):
    pts, lengths = cloud(name)
    for dis in (True, False):
        plain, through = _both(pts, lengths, K, dis)
        _assert_bitwise((name, K, dis), plain, through)
        assert through[0].abs().sum() > 0


def test_the_70_point_clouds_at_the_ends_of_k():
    pts, _ = cloud("batch70")
    _assert_bitwise(("batch70", 2), *_both(pts, None, 2, True))
    grid = kernels.point_grid_build(pts.to(DEV))
    for g in (None, grid):  # above 64: exactly as without a grid
        with pytest.raises(NotImplementedError, match="64"):
            kernels.point_frames(pts.to(DEV), None, 69, grid=g)
    nine = pts[:, :9].contiguous().to(DEV)  # P <= K
    with pytest.raises(ValueError):
        kernels.point_frames(nine, None, 9, grid=kernels.point_grid_build(nine))


@pytest.mark.parametrize("name", ["sphere1100", "cow"])
def test_covariance_against_the_float64_restatement(name):
    K = 16
    pts, lengths = cloud(name)
    r = ref(name, K)
    ptsd = pts.to(DEV)
    l = None if lengths is None else lengths.to(DEV)
    _, _, cov = kernels.point_frames(ptsd, l, K, return_cov=True, grid=kernels.point_grid_build(ptsd, l))
    got = NR.cov33(cov.cpu().numpy())
    ok = r["valid"]
    tr = np.trace(r["cov"][ok], axis1=1, axis2=2)
    err = np.abs(got[ok] - r["cov"][ok]).reshape(-1, 9).max(1)
    print(f"[frames grid] {name} K = {K}: max |cov - ref| / trace {(err / tr).max():.2e}")
    assert (err <= 1e-4 * tr).all() and (got[~ok] == 0).all()


@functools.lru_cache(maxsize=None)
def against_a_grid(name):
    """(points (1,P,3) on the CPU, never modified; K)."""
    t = _rand(1, 3000, 3, seed=102)
    if name == "uniform":
        return t, 8
    if name == "offset":
        return t + 1000.0, 8
    if name == "planar":
        p = t.clone()
        p[..., 2] = 0.25
        return p, 8
    if name == "outlier":
        p = t.clone()
        p[0, 0] = torch.tensor([500.0, -300.0, 40.0])
        return p, 8
    if name == "lattice":  # the 12^3 lattice of spacing 1/8 twice over: exact ties on cell faces, every point twice
        r = torch.arange(12, dtype=torch.float32) / 8.0
        lat = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
        return torch.cat([lat, lat], 0)[None].contiguous(), 16
    if name == "coincident":
        return torch.tensor([0.3, 1.3, 2.3]).expand(1, 3000, 3).contiguous(), 8
    if name == "collinear":
        s = torch.linspace(-1.0, 1.0, 3000)[:, None]
        return (s * torch.tensor([[1.0, 2.0, 3.0]]) + 0.5)[None].contiguous(), 8
    if name == "20001":  # 18^3 cells, more than the 1,024 threads of the scan; P is no multiple of the wave
        return _rand(1, 20001, 3, seed=105), 8
    if name == "9":  # P = K + 1
        return _rand(1, 9, 3, seed=106), 8
    if name == "65":
        return _rand(1, 65, 3, seed=107), 8
    raise KeyError(name)


AGAINST = ("uniform", "offset", "planar", "outlier", "lattice", "coincident", "collinear", "20001", "9", "65")


@pytest.mark.parametrize("name", AGAINST)
def test_frames_grid_bitwise_on_clouds_chosen_against_a_grid(name):
    pts, K = against_a_grid(name)
    for dis in (True, False):
        plain, through = _both(pts, None, K, dis)
        _assert_bitwise((name, K, dis), plain, through)
        assert torch.isfinite(through[1]).all()
    if name == "65":  # the deepest list, one point to spare
        _assert_bitwise((name, 64), *_both(pts, None, 64, True))


# --------------------------------------------------------------------------- the grid is used; determinism; padding
def test_the_search_visits_a_fraction_of_the_cloud():
    pts, K = against_a_grid("20001")
    P = pts.shape[1]
    visited = torch.zeros(1, dtype=torch.int64, device=DEV)
    plain, through = _both(pts, None, K, True, visited)
    _assert_bitwise(("20001", "visited"), plain, through)
    print(f"[frames grid] 1 x {P}, K = {K}: {visited.item() / P:.1f} distances per query, {visited.item() / (P * P):.5f} "
          "of all pairs")
    assert 0 < visited.item() < P * P / 10
    with pytest.raises(ValueError, match="visited"):
        kernels.point_frames(pts.to(DEV), None, K, visited=visited)


def test_two_runs_are_bitwise_equal_and_padded_rows_are_zero():
    pts, lengths = cloud("cow")
    a = _both(pts, lengths, 16, True)[1]
    b = _both(pts, lengths, 16, True)[1]  # another build: the order inside a cell may differ
    _assert_bitwise("two runs", a, b)
    for t in a:
        assert (t[1, 257:] == 0).all() and (t[1, :257] != 0).any()
    # a cloud shorter than K inside a batch that is not: its rows are zeros, as without a grid
    short = torch.tensor([733, 12])
    plain, through = _both(pts, short, 16, True)
    _assert_bitwise("short", plain, through)
    assert all((t[1] == 0).all() for t in through)


# --------------------------------------------------------------------------- the public functions
def test_public_functions_take_a_grid_in_place_of_the_cloud():
    pts, lengths = cloud("cow")
    K = 16
    one = pts[:1].to(DEV)
    c, f = estimate_pointcloud_local_coord_frames(one, K)
    grid = PointGrid(one)
    cg, fg = estimate_pointcloud_local_coord_frames(grid, K, use_symeig_workaround=False)
    assert torch.equal(c, cg) and torch.equal(f, fg)
    assert torch.equal(estimate_pointcloud_normals(grid, K), f[..., 0])
    assert torch.equal(estimate_pointcloud_normals(grid, K, False), estimate_pointcloud_normals(one, K, False))
    # a tensor with lengths; a Pointclouds brings its own
    pd, ld = pts.to(DEV), lengths.to(DEV)
    cur, frm = kernels.point_frames(pd, ld, K)
    cl, fl = estimate_pointcloud_local_coord_frames(PointGrid(pd, ld), K)
    assert torch.equal(cl, cur) and torch.equal(fl, frm)
    pc = Pointclouds([pd[0], pd[1, :257]])
    cp, fp = estimate_pointcloud_local_coord_frames(PointGrid(pc), K)
    c0, f0 = estimate_pointcloud_local_coord_frames(pc, K)
    assert torch.equal(cp, c0) and torch.equal(fp, f0) and torch.equal(cp, cur)
    # float64 in, float64 out
    d64 = one.double()
    n64 = estimate_pointcloud_normals(PointGrid(d64), K)
    assert n64.dtype == torch.float64 and torch.equal(n64, estimate_pointcloud_normals(d64, K))
    # errors: a cloud with length <= K, a tensor modified in place since the build
    short = Pointclouds([pd[0], pd[1, :16]])  # kept alive: the grid holds its padded tensor by weak reference
    with pytest.raises(ValueError, match="smaller than the size"):
        estimate_pointcloud_normals(PointGrid(short), K)
    with pytest.raises(ValueError, match="smaller than the size"):
        estimate_pointcloud_normals(PointGrid(pd, torch.tensor([733, 16], device=DEV)), K)
    stale = PointGrid(one)
    one.mul_(2.0)
    with pytest.raises(ValueError, match="modified in place"):
        estimate_pointcloud_normals(stale, K)
    with pytest.raises(ValueError, match="modified in place"):
        estimate_pointcloud_local_coord_frames(stale, K)


def test_hip_graph_capture_of_build_and_frames_replays_with_changed_points():
    K = 16
    pts = _rand(2, 700, 3, seed=120).to(DEV)

    def step():
        return estimate_pointcloud_local_coord_frames(PointGrid(pts), neighborhood_size=K)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up on the side stream: workspace sizes cached, allocator primed
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for seed in (121, 122):  # replay twice, each time with other points in the captured tensor
        pts.copy_(_rand(2, 700, 3, seed=seed).to(DEV) * 3.0 - 1.0)
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        eager = estimate_pointcloud_local_coord_frames(pts, neighborhood_size=K)
        for u, w in zip(eager, captured):
            assert torch.equal(u, w)


# --------------------------------------------------------------------------- the plane loop's normals
def test_plane_icp_through_a_grid_estimates_its_normals_through_the_grid():
    g = torch.Generator().manual_seed(130)
    Y = torch.randn(2, 600, 3, generator=g)
    Y = (Y / Y.norm(dim=-1, keepdim=True) * torch.tensor([1.0, 0.7, 0.4])).to(DEV)
    a = 0.1
    R = torch.tensor([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    X = (Y[:, :500] @ R.to(DEV) + 0.02).contiguous()
    normals = estimate_pointcloud_normals(Y, 16)
    want = iterative_closest_point_to_plane(X, Y, normals, max_iterations=5)
    grid = PointGrid(Y)
    got = iterative_closest_point_to_plane(X, grid, None, max_iterations=5, neighborhood_size=16)
    also = iterative_closest_point_to_plane(X, grid, normals, max_iterations=5)
    for sol in (got, also):
        assert sol.converged == want.converged and len(sol.t_history) == len(want.t_history) >= 1
        assert torch.equal(sol.rmse, want.rmse) and torch.equal(sol.Xt, want.Xt)
        for u, w in zip(sol.RTs, want.RTs):
            assert torch.equal(u, w)
        for hu, hw in zip(sol.t_history, want.t_history):
            for u, w in zip(hu, hw):
                assert torch.equal(u, w)
    assert (want.rmse > 0).all()
