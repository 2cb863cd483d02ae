"""sample_farthest_points (csrc/mr_fps.hip) without a GPU: the import path, the Python layer's errors, the C ABI's
checks before any launch, the launch geometry, and a sanity test of the restatement of tests/fps_ref.py itself."""
import os

import pytest
import torch

from tests import fps_ref as FR
from torch_renderer_amd import _lib, kernels, ops
from torch_renderer_amd.structures import Pointclouds


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from torch_renderer_amd import _build

        _build.build()
    return _lib.load()


def test_upstream_import_path():
    from torch_renderer_amd.ops import sample_farthest_points

    assert sample_farthest_points is ops.sample_farthest_points
    for name in ("farthest_points", "farthest_geometry", "FarthestPoints"):
        assert hasattr(kernels, name), name
    for name in ("mr_farthest_points", "mr_farthest_points_geometry", "mr_farthest_points_workspace"):
        assert name in _lib.EXPORTED_SYMBOLS


def test_python_errors_come_before_any_device_use():
    g = torch.Generator().manual_seed(0)
    p = torch.randn(2, 9, 3, generator=g)
    f = ops.sample_farthest_points
    with pytest.raises(ValueError, match="points and lengths must have same batch dimension."):
        f(p, lengths=torch.tensor([9]))
    with pytest.raises(ValueError, match="points and lengths must have same batch dimension."):
        f(p, lengths=torch.tensor([[9, 9]]))
    with pytest.raises(ValueError, match="A value in lengths was too large."):
        f(p, lengths=torch.tensor([9, 10]))
    with pytest.raises(ValueError):
        f(p, lengths=torch.tensor([-1, 9]))
    with pytest.raises(ValueError, match="K and points must have the same batch dimension"):
        f(p, K=[3])
    with pytest.raises(ValueError, match="K and points must have the same batch dimension"):
        f(p, K=torch.tensor([3, 3, 3]))
    with pytest.raises(ValueError):
        f(p, K=[3, -1])
    with pytest.raises(ValueError):
        f(p, K=torch.tensor([-2, 3]))
    with pytest.raises(ValueError):
        f(p, K=-1)
    with pytest.raises(ValueError):
        f(p, K=torch.tensor([1.0, 2.0]))  # not integers
    with pytest.raises(ValueError):
        f(p[0])  # not (N, P, D)
    with pytest.raises(ValueError):
        f([p[0], p[1]])  # neither a tensor nor a Pointclouds
    with pytest.raises(NotImplementedError):
        f(p[..., :2])  # D = 2
    with pytest.raises(NotImplementedError):
        kernels.farthest_points(p[..., :2], K=3)
    with pytest.raises(ValueError):
        f(Pointclouds([p[0], p[1, :4]]), lengths=torch.tensor([9, 4]))  # a Pointclouds brings its own lengths
    with pytest.raises(ValueError):
        kernels.farthest_points(p, K=0)
    with pytest.raises(ValueError):
        kernels.farthest_points(p, K=3, start_idx=torch.tensor([0]))
    for call in (lambda: f(p), lambda: f(p, K=3, random_start_point=True), lambda: f(p, torch.tensor([9, 4]), [2, 5]),
                 lambda: f(Pointclouds([p[0], p[1, :4]]), K=3), lambda: kernels.farthest_points(p, K=3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_abi_rejects_bad_arguments_without_touching_the_gpu(lib):
    one = 1  # any non-NULL pointer value: the checks below return before anything is read
    f = lib.mr_farthest_points
    ws = lib.mr_farthest_points_workspace(2, 100, 8)
    assert ws > 0
    assert f(None, 2, 100, None, None, 8, None, one, one, one, ws, None) == 1 and b"NULL" in lib.mr_last_error()
    assert f(one, 2, 100, None, None, 8, None, None, one, one, ws, None) == 1
    assert f(one, 2, 100, None, None, 8, None, one, None, one, ws, None) == 1
    assert f(one, 2, 100, None, None, 8, None, one, one, None, ws, None) == 1
    for N, P, K in ((0, 100, 8), (2, 0, 8), (2, 100, 0), (-1, 100, 8), (2, 100, -3)):
        assert f(one, N, P, None, None, K, None, one, one, one, ws, None) == 1, (N, P, K)
        assert lib.mr_farthest_points_geometry(N, P, K, None, None, None) == 1
        assert lib.mr_farthest_points_workspace(N, P, K) == 0
    rc = f(one, 1, 1 << 31, None, None, 8, None, one, one, one, 1 << 40, None)  # too large for 32-bit point ids
    assert rc == 3 and b"32-bit" in lib.mr_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc)
    assert lib.mr_farthest_points_geometry(1, 1 << 31, 8, None, None, None) == 3
    assert lib.mr_farthest_points_workspace(1, 1 << 31, 8) == 0
    # a workspace one byte short, on the register path and on the streamed path (whose m values live there)
    big = FR.register_capacity(kernels.farthest_geometry) + 1
    assert kernels.farthest_geometry(2, big, 8)[2] and not kernels.farthest_geometry(2, big - 1, 8)[2]
    for P in (100, big):
        ws = lib.mr_farthest_points_workspace(2, P, 8)
        assert f(one, 2, P, None, None, 8, None, one, one, one, ws - 1, None) == 4
        assert b"workspace" in lib.mr_last_error()
    assert lib.mr_farthest_points_workspace(2, big, 8) >= 4 * 2 * big > lib.mr_farthest_points_workspace(2, 100, 8)


def test_geometry(lib):
    geo = kernels.farthest_geometry
    seen = set()
    for P in (1, 50, 64, 65, 256, 257, 300, 600, 1500, 2048, 2049, 5000, 10000, 20000, 32768):
        threads, per, streamed = geo(1, P, 4)
        seen.add((threads, per))
        assert not streamed and threads in (64, 256, 1024) and per in (1, 2, 4, 8, 16, 32), (P, threads, per)
        assert threads * per >= P, (P, threads, per)  # the cloud fits
        assert per == 1 or threads * (per // 2) < P, (P, threads, per)  # in the smallest bucket that holds it
    assert geo(1, 50, 4)[0] == 64 and geo(1, 300, 4)[0] == 256 and geo(1, 20000, 4) == (1024, 32, False)
    assert len(seen) == 10  # every (threads, points per thread) pair the library builds
    threads, per, streamed = geo(1, 32769, 4)
    assert streamed and threads == 1024 and per == 33
    assert geo(300, 2000, 500) == geo(1, 2000, 1)  # one workgroup per cloud: N and K do not enter
    with pytest.raises(NotImplementedError):
        geo(1, 1 << 31, 4)
    with pytest.raises(RuntimeError):
        geo(0, 10, 4)


def test_restatement_selects_a_farthest_point_every_round():
    """Distances recomputed in float64: every selected point's float64 min-distance to the points selected before it
    is >= (1 - 1e-6) x the float64 maximum over the cloud at that round. The float32 distance is a sum of three squares
    of float32 differences, about 6 roundings of 2^-24 (3.6e-7 relative), so 1e-6 is derived, not tuned."""
    pts = FR.cloud(1, 500, seed=77)
    K = 40
    idx, sel = FR.fps_ref(pts, K=K, start_idx=torch.tensor([17]))
    assert idx.dtype == torch.int32 and idx.shape == (1, K) and sel.shape == (1, K, 3)
    assert int(idx[0, 0]) == 17 and torch.equal(sel[0], pts[0][idx[0].long()])
    assert len(set(idx[0].tolist())) == K  # distinct points: nothing is selected twice
    c = pts[0].double()
    m = torch.full((500,), float("inf"), dtype=torch.float64)
    worst = 1.0
    for k in range(1, K):
        m = torch.minimum(m, ((c - c[idx[0, k - 1]]) ** 2).sum(-1))
        ratio = (m[idx[0, k]] / m.max()).item()
        worst = min(worst, ratio)
        assert ratio >= 1 - 1e-6, (k, ratio)
    print(f"[fps] restatement: worst selected / max float64 min-distance over {K - 1} rounds: {worst:.9f}")


def test_restatement_edge_cases():
    # exact ties go to the lowest index: on the lattice every distance is an integer, exact in float32 and float64
    pts, _, K, _ = FR.case("lattice")
    idx, _ = FR.fps_ref(pts, K=K)
    assert idx[0, :2].tolist() == [0, 63]  # from corner 0 the opposite corner
    c, m, tied = pts[0].double(), torch.full((64,), float("inf"), dtype=torch.float64), 0
    for k in range(1, K):
        m = torch.minimum(m, ((c - c[idx[0, k - 1]]) ** 2).sum(-1))
        best = (m == m.max()).nonzero()[:, 0]
        tied += int(len(best) > 1)
        assert int(idx[0, k]) == int(best[0]), (k, best.tolist())
    print(f"[fps] lattice: {tied} of {K - 1} rounds had more than one farthest point")
    assert tied >= 5
    # identical points: the start, then index 0 for ever
    pts, _, K, start = FR.case("same")
    idx, sel = FR.fps_ref(pts, K=K, start_idx=start)
    assert idx[0].tolist() == [3, 0, 0, 0, 0, 0] and torch.equal(sel[0], pts[0, :1].expand(6, 3))
    # padding: K per cloud above and below the lengths, an empty cloud, K = 0
    pts, lengths, K, _ = FR.case("klist")
    idx, sel = FR.fps_ref(pts, lengths, K)
    assert idx.shape == (4, 9) and (idx[0] == -1).all() and idx[1].tolist() == [0] + [-1] * 8
    assert (idx[2, :3] >= 0).all() and (idx[2, 3:] == -1).all() and (idx[3] == -1).all()
    assert (sel[idx < 0] == 0).all() and (idx[2, :3] < 7).all()
