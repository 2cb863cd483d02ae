"""The ICP loops through a PointGrid on the MI355X (k_icp_nn_grid of csrc/mr_points.hip): every call with
``Y = PointGrid(...)`` against the call with the points themselves, bit for bit. The points route is the unchanged code
that test_gpu_icp.py and test_gpu_icp_plane.py hold to the float64 restatements.

* every case of icp_ref.CASES and icp_plane_ref.CASES through the grid (lengths travel in Pointclouds on both sides);
* clouds chosen against a grid, 1 x 200 -> 3,000 built as test_gpu_knn_grid.adversarial builds them: queries outside
  the box, a far outlier, a planar target, coincident targets, a lattice on the cell faces, a large offset, a target
  cloud of one point, an empty source cloud;
* the distance cap of the plane estimator: bitwise at three distances, and it only removes ring visits;
* the grid is really used (the counter of evaluated distances), idle iterations add nothing;
* reproducible from build to build and independent of the status batch; a grid of other clouds returns.
"""
import functools
import math

import pytest
import torch

from tests import icp_plane_ref as PR
from tests import icp_ref as IR
from tests.test_gpu_knn_grid import adversarial
from torch_renderer_amd import Pointclouds, kernels
from torch_renderer_amd.ops import (PointGrid, SimilarityTransform, iterative_closest_point,
                                    iterative_closest_point_to_plane)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(t):
    return None if t is None else t.to(DEV)


def _as_pointclouds(t, lengths):
    n = [t.shape[1]] * t.shape[0] if lengths is None else [int(v) for v in lengths.tolist()]
    return Pointclouds([t[i, :n[i]].to(DEV) for i in range(t.shape[0])])


def _kw(kw):
    kw = dict(kw)
    init = kw.pop("init", None)
    if init is not None:
        kw["init_transform"] = SimilarityTransform(*(t.to(DEV) for t in init))
    return kw


def _padded(xt):
    return xt.points_padded() if isinstance(xt, Pointclouds) else xt


def _flat(sol):
    return [sol.rmse, _padded(sol.Xt), *sol.RTs] + [t for h in sol.t_history for t in h]


def _bits(t):
    assert t.dtype == torch.float32
    return t.contiguous().view(torch.int32)


def _assert_same_solution(tag, got, want):
    assert type(got.Xt) is type(want.Xt), tag
    assert got.converged == want.converged and len(got.t_history) == len(want.t_history), \
        (tag, got.converged, want.converged, len(got.t_history), len(want.t_history))
    a, b = _flat(got), _flat(want)
    assert len(a) == len(b)
    for k, (u, w) in enumerate(zip(a, b)):
        assert torch.equal(_bits(u), _bits(w)), (tag, k)


def _assert_same_tuple(tag, got, want):
    """The tuples of kernels.icp / kernels.icp_plane."""
    assert got[0] == want[0] and got[1] == want[1], (tag, got[:2], want[:2])
    for k, (u, w) in enumerate(zip(got[2:], want[2:])):
        assert torch.equal(_bits(u), _bits(w)), (tag, k)


def _pair(X, Y, xl, yl, pointclouds=False):
    """(X, Y as points, Y as a PointGrid of those points) on the device; lengths travel in Pointclouds."""
    if pointclouds or xl is not None or yl is not None:
        x, y = _as_pointclouds(X, xl), _as_pointclouds(Y, yl)
    else:
        x, y = X.to(DEV), Y.to(DEV)
    return x, y, PointGrid(y)


# --------------------------------------------------------------------------- the existing cases, through the grid
@pytest.mark.parametrize("name", list(IR.CASES))
def test_icp_cases_through_the_grid(name):
    X, Y, xl, yl, kw = IR.case(name)
    x, y, grid = _pair(X, Y, xl, yl)
    want = iterative_closest_point(x, y, **_kw(kw))
    got = iterative_closest_point(x, grid, **_kw(kw))
    print(f"[icp grid] {name}: {len(want.t_history)} iterations, converged {want.converged}")
    assert len(want.t_history) >= 1
    _assert_same_solution(name, got, want)


@pytest.mark.parametrize("name", list(PR.CASES))
def test_icp_plane_cases_through_the_grid(name):
    X, Y, Yn, xl, yl, kw = PR.case(name)
    x, y, grid = _pair(X, Y, xl, yl)
    want = iterative_closest_point_to_plane(x, y, Yn.to(DEV), **_kw(kw))
    got = iterative_closest_point_to_plane(x, grid, Yn.to(DEV), **_kw(kw))
    print(f"[icp plane grid] {name}: {len(want.t_history)} iterations, converged {want.converged}")
    assert len(want.t_history) >= 1
    _assert_same_solution(name, got, want)


def test_pointclouds_on_both_sides_of_full_clouds():
    """Full clouds as Pointclouds (no lengths reach the kernels), once per estimator; Xt comes back in X's type; the
    normals estimated from the grid's points are those estimated from the points."""
    X, Y, xl, yl, kw = IR.case("scale")
    x, y, grid = _pair(X, Y, xl, yl, pointclouds=True)
    assert grid.full
    got = iterative_closest_point(x, grid, **_kw(kw))
    assert isinstance(got.Xt, Pointclouds)
    _assert_same_solution("scale", got, iterative_closest_point(x, y, **_kw(kw)))
    X, Y, Yn, xl, yl, kw = PR.case("tiles")
    x, y, grid = _pair(X, Y, xl, yl, pointclouds=True)
    got = iterative_closest_point_to_plane(x, grid, Yn.to(DEV), **_kw(kw))
    assert isinstance(got.Xt, Pointclouds)
    _assert_same_solution("tiles", got, iterative_closest_point_to_plane(x, y, Yn.to(DEV), **_kw(kw)))
    X, Y, Yn, xl, yl, kw = PR.case("het")
    x, y, grid = _pair(X, Y, xl, yl)
    _assert_same_solution("het, estimated normals",
                          iterative_closest_point_to_plane(x, grid, neighborhood_size=16, **_kw(kw)),
                          iterative_closest_point_to_plane(x, y, neighborhood_size=16, **_kw(kw)))
    # a grid of a tensor with a lengths tensor: the kernels' call with those lengths
    yd, ld = Y.to(DEV), yl.to(DEV)  # the grid holds its tensor by weak reference
    g2 = PointGrid(yd, ld)
    a = iterative_closest_point(x, g2, **_kw(IR.case("het")[4]))
    b = iterative_closest_point(x, y, **_kw(IR.case("het")[4]))
    _assert_same_solution("het, tensor grid with lengths", a, b)


# --------------------------------------------------------------------------- shapes chosen against a grid
SHAPES = ("outside", "outlier", "planar", "coincident", "lattice", "offset", "one-target", "empty-source")


def _moved_subset(t, count=200, angle=0.05, shift=0.02, seed=7):
    """`count` of the targets t (P,3), evenly spaced in index, rotated by `angle` rad about their centroid and shifted."""
    sub = t[:: max(t.shape[0] // count, 1)][:count].double()
    g = torch.Generator().manual_seed(seed)
    R = IR.rotations(torch.randn(1, 3, generator=g), torch.tensor([angle]))[0]
    d = torch.randn(3, generator=g, dtype=torch.float64)
    c = sub.mean(0)
    return ((sub - c) @ R + c + shift * d / d.norm()).float()


@functools.lru_cache(maxsize=None)
def shape(name):
    """(X, Y, Yn, x_lengths, y_lengths, init) on the CPU (never modified): the targets of test_gpu_knn_grid.adversarial,
    the sources a rotated subset of them, unit normals drawn at random (the estimator takes them as given)."""
    src = {"outside": "uniform", "one-target": "uniform", "empty-source": "uniform"}.get(name, name)
    Y = adversarial(src)[1]
    if name == "lattice":  # 3,456 points; the sources start a quarter cell off the lattice
        X = _moved_subset(Y[0], angle=0.02, shift=1.0 / 32.0)[None]
    elif name == "coincident":  # nothing to subsample: the sources of the uniform cloud
        X = _moved_subset(adversarial("uniform")[1][0])[None]
    else:
        X = _moved_subset(Y[0])[None]
    xl = yl = init = None
    if name == "outside":  # three box sizes away: every query of the first iteration is outside the box
        init = IR.RTs(torch.eye(3)[None], torch.full((1, 3), 3.0), torch.ones(1))
    if name in ("one-target", "empty-source"):
        X = torch.cat([X, X.flip(1)], 0).contiguous()
        Y = torch.cat([Y, Y.flip(1)], 0).contiguous()
        if name == "one-target":
            yl = torch.tensor([Y.shape[1], 1])
        else:
            xl = torch.tensor([X.shape[1], 0])
    g = torch.Generator().manual_seed(11)
    Yn = torch.randn(Y.shape, generator=g)
    return X, Y, Yn / Yn.norm(dim=2, keepdim=True), xl, yl, init


@pytest.mark.parametrize("name", SHAPES)
def test_icp_shapes_chosen_against_a_grid(name):
    X, Y, _, xl, yl, init = shape(name)
    kw = _kw({"init": init, "max_iterations": 30})
    x, y, grid = _pair(X, Y, xl, yl)
    want = iterative_closest_point(x, y, **kw)
    got = iterative_closest_point(x, grid, **kw)
    print(f"[icp grid] {name}: {len(want.t_history)} iterations, converged {want.converged}, "
          f"grid dims {grid.describe()[0].tolist()}")
    _assert_same_solution(name, got, want)


@pytest.mark.parametrize("name", SHAPES)
def test_icp_plane_shapes_chosen_against_a_grid(name):
    X, Y, Yn, xl, yl, init = shape(name)
    kw = _kw({"init": init, "max_iterations": 30, "relative_rmse_thr": PR.THR})
    x, y, grid = _pair(X, Y, xl, yl)
    want = iterative_closest_point_to_plane(x, y, Yn.to(DEV), **kw)
    got = iterative_closest_point_to_plane(x, grid, Yn.to(DEV), **kw)
    print(f"[icp plane grid] {name}: {len(want.t_history)} iterations, converged {want.converged}")
    _assert_same_solution(name, got, want)
    capped = dict(kw, max_correspondence_distance=0.1)
    _assert_same_solution(name + ", capped", iterative_closest_point_to_plane(x, grid, Yn.to(DEV), **capped),
                          iterative_closest_point_to_plane(x, y, Yn.to(DEV), **capped))


# --------------------------------------------------------------------------- the distance cap, plane estimator
@functools.lru_cache(maxsize=None)
def cut_scan():
    """(X (1,500,3), Y (1,2000,3), Yn): the target is the ellipsoid of icp_plane_ref cut by the half-space x < 0.2,
    the source another sample of the whole surface moved by 5 degrees and 0.03: the sources over the missing part
    lie far from every target."""
    g = torch.Generator().manual_seed(21)
    pts, nrm = PR.ellipsoid(6000, g)
    keep = (pts[:, 0] < 0.2).nonzero()[:2000, 0]
    assert keep.numel() == 2000
    xs, _ = PR.ellipsoid(500, g)
    R = IR.rotations(torch.randn(1, 3, generator=g), torch.tensor([math.radians(5.0)]))[0]
    X = (xs.double() @ R + torch.tensor([0.03, 0.0, 0.0], dtype=torch.float64)).float()
    far = (torch.cdist(X.double(), pts[keep].double()).min(1).values > 0.3).sum().item()
    assert far >= 50, far
    return X[None].contiguous(), pts[keep][None].contiguous(), nrm[keep][None].contiguous()


def _cap_inputs(which):
    if which == "maxd":
        X, Y, Yn, _, _, kw = PR.case("maxd")
        return X, Y, Yn, {k: v for k, v in kw.items() if k != "max_correspondence_distance"}
    return (*cut_scan(), {"relative_rmse_thr": PR.THR})


@pytest.mark.parametrize("which", ["maxd", "cut"])
@pytest.mark.parametrize("d", [0.15, 0.02, 1e-6])
def test_the_cap_is_bitwise_the_points_route(which, d):
    X, Y, Yn, kw = _cap_inputs(which)
    x, y, yn = X.to(DEV), Y.to(DEV), Yn.to(DEV)
    want = iterative_closest_point_to_plane(x, y, yn, max_correspondence_distance=d, **kw)
    got = iterative_closest_point_to_plane(x, PointGrid(y), yn, max_correspondence_distance=d, **kw)
    print(f"[icp plane grid] {which}, d = {d}: {len(want.t_history)} iterations, rmse {want.rmse.tolist()}")
    _assert_same_solution((which, d), got, want)
    if d == 1e-6:  # every pair is rejected: the transform stays the identity, bit for bit
        assert got.converged and len(got.t_history) == 1 and got.rmse.item() == 0.0
        assert torch.equal(got.RTs.R.cpu(), torch.eye(3)[None]) and torch.equal(got.RTs.T.cpu(), torch.zeros(1, 3))
        assert torch.equal(_bits(got.Xt), _bits(x))


def test_the_cap_only_removes_ring_visits():
    """One iteration from the same start with and without the cap: a lane's capped walk is a prefix of its uncapped
    one, and the sources over the cut lie far from every target, so the capped count is strictly smaller."""
    X, Y, Yn = (t.to(DEV) for t in cut_scan())
    grid = kernels.point_grid_build(Y)
    counts = {}
    for d in (None, 0.15, 0.02):
        visited = torch.zeros(1, dtype=torch.int64, device=DEV)
        got = kernels.icp_plane(X, Y, Yn, max_iterations=1, max_correspondence_distance=d, grid=grid, visited=visited)
        want = kernels.icp_plane(X, Y, Yn, max_iterations=1, max_correspondence_distance=d)
        _assert_same_tuple(("cut", d), got, want)
        assert got[1] == 1
        counts[d] = visited.item()
    print(f"[icp plane grid] cut scan, distances per source point and iteration: "
          + ", ".join(f"d = {d}: {c / 500:.1f}" for d, c in counts.items()))
    assert 0 < counts[0.02] <= counts[0.15] < counts[None] <= 500 * 2000


# --------------------------------------------------------------------------- the grid is used
def test_the_search_visits_a_fraction_of_the_targets():
    Y = adversarial("uniform")[1]
    X = _moved_subset(Y[0])[None]  # within 0.05 rad and 0.02 of the truth
    x, y = X.to(DEV), Y.to(DEV)
    visited = torch.zeros(1, dtype=torch.int64, device=DEV)
    got = kernels.icp(x, y, grid=kernels.point_grid_build(y), visited=visited)
    _assert_same_tuple("uniform", got, kernels.icp(x, y))
    iters = got[1]
    share = visited.item() / (iters * 200 * 3000)
    print(f"[icp grid] uniform 200 x 3000: {iters} iterations, {share:.4f} of all pairs evaluated")
    assert iters >= 2 and 0 < share <= 0.25, share


def test_one_cell_visits_every_pair_and_idle_iterations_add_nothing():
    """The coincident cloud is one cell: every iteration that runs evaluates every pair. The loop converges before its
    first status batch of 8 ends, so the count is a multiple of the iterations run, not of those enqueued; a second
    call on the same counter adds its own iterations."""
    X, Y, _, _, _, _ = shape("coincident")
    x, y = X.to(DEV), Y.to(DEV)
    grid = kernels.point_grid_build(y)
    visited = torch.zeros(1, dtype=torch.int64, device=DEV)
    got = kernels.icp(x, y, grid=grid, visited=visited)
    iters = got[1]
    assert got[0] and 1 <= iters < kernels.ICP_STATUS_BATCH, got[:2]
    assert visited.item() == iters * 200 * 3000
    _assert_same_tuple("coincident", got, kernels.icp(x, y))
    again = kernels.icp(x, y, grid=grid, visited=visited, status_batch=3)
    assert again[1] == iters and visited.item() == 2 * iters * 200 * 3000
    with pytest.raises(ValueError, match="visited"):
        kernels.icp(x, y, visited=visited)
    with pytest.raises(ValueError, match="grid"):
        kernels.icp(x, y, grid=kernels.point_grid_build(y[:, :2000].contiguous()))


# --------------------------------------------------------------------------- reproducible, status batch, a stale grid
@pytest.mark.parametrize("plane", [False, True])
def test_reproducible_and_independent_of_the_status_batch(plane):
    """The order inside a cell varies from build to build and no result may depend on it: the grid is rebuilt for
    every run."""
    if plane:
        X, Y, Yn, xl, yl, _ = PR.case("chunks")
        args = (X.to(DEV), Y.to(DEV), Yn.to(DEV), _dev(xl), _dev(yl))
        fn = kernels.icp_plane
    else:
        X, Y, xl, yl, _ = IR.case("chunks")
        args = (X.to(DEV), Y.to(DEV), _dev(xl), _dev(yl))
        fn = kernels.icp
    y, l2 = args[1], args[-1]
    want = fn(*args)
    assert want[1] >= 2
    for batch in (None, None, 1, 3):
        _assert_same_tuple(("chunks", plane, batch), fn(*args, status_batch=batch, grid=kernels.point_grid_build(y, l2)),
                           want)


def test_a_grid_of_other_clouds_returns():
    """The grid of other clouds of the same shape: the walk clamps every address it forms into the buffers it was given
    (test_gpu_knn_grid.py observes the indices themselves: in [-1, P2)), and the moments kernels take an index at or
    past the target's length as "no target". So the call returns, with wrong and finite results of the right shape."""
    P2 = 3000
    g = torch.Generator().manual_seed(107)
    old = (torch.rand(2, P2, 3, generator=g) * 3.0 - 1.0).to(DEV)
    new = torch.rand(2, P2, 3, generator=g).to(DEV)
    x = torch.rand(2, 200, 3, generator=g).to(DEV)
    l2 = torch.tensor([P2, 1700], device=DEV)
    grid = kernels.point_grid_build(old)  # other points, other lengths
    conv, iters, rmse, xt, rts, hist = kernels.icp(x, new, None, l2, max_iterations=5, grid=grid)
    torch.cuda.synchronize()
    assert 1 <= iters <= 5 and xt.shape == x.shape and rts.shape == (2, 13) and hist.shape == (iters, 2, 13)
    assert torch.isfinite(xt).all() and torch.isfinite(rts).all() and torch.isfinite(rmse).all()
