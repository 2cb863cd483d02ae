"""iterative_closest_point_to_plane (csrc/mr_points.hip, k_icp_plane_*) on the GPU against the float64 restatement of
tests/icp_plane_ref.py run on the CPU.

* every case of icp_plane_ref.CASES (whose restatements with float32 and float64 moments make the same decisions:
  test_icp_plane_cpu.py::test_input_condition_of_the_gpu_cases): ``converged`` and the number of iterations equal the
  restatement's; every R and T of the history, the final RTs, rmse and Xt within 1e-4 * max(1, |ref|) of it; s is the
  initial scale bitwise; |R R^T - I| <= 1e-5;
* bitwise: run to run, and status batches of 1, 3 and 8 iterations;
* Y_normals=None against the explicit estimate, and every normal's sign flipped;
* Pointclouds inputs, max_iterations = 0, an empty source cloud;
* a planar target (rank-deficient normal equations), a cloud whose every pair is rejected, a cloud of four points;
* the reason for the estimator: fewer iterations than point-to-point on a smooth cloud.
"""
import math

import pytest
import torch

from tests import icp_plane_ref as PR
from tests.helpers import report
from tests.icp_ref import apply_ref, rotations
from torch_renderer_amd import Pointclouds, kernels
from torch_renderer_amd.ops import (SimilarityTransform, estimate_pointcloud_normals, iterative_closest_point,
                                    iterative_closest_point_to_plane)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(t):
    return None if t is None else t.to(DEV)


def _as_pointclouds(t, lengths):
    n = [t.shape[1]] * t.shape[0] if lengths is None else lengths.tolist()
    return Pointclouds([t[i, :n[i]].to(DEV) for i in range(t.shape[0])])


def _kw(kw):
    kw = dict(kw)
    init = kw.pop("init", None)
    if init is not None:
        kw["init_transform"] = SimilarityTransform(*(t.to(DEV) for t in init))
    return kw


def _run(name, pointclouds=False, **over):
    X, Y, Yn, xl, yl, kw = PR.case(name)
    kw = dict(_kw(kw), **over)
    if pointclouds or xl is not None or yl is not None:  # lengths travel in Pointclouds
        return iterative_closest_point_to_plane(_as_pointclouds(X, xl), _as_pointclouds(Y, yl), Yn.to(DEV), **kw)
    return iterative_closest_point_to_plane(X.to(DEV), Y.to(DEV), Yn.to(DEV), **kw)


def _padded(xt):
    return xt.points_padded() if isinstance(xt, Pointclouds) else xt


def _check(name, got, tag=""):
    r32, r64 = PR.restated(name, torch.float32), PR.restated(name, torch.float64)
    X, _, _, xl, _, kw = PR.case(name)
    N, P1 = X.shape[:2]
    assert got.converged == r64.converged
    assert len(got.t_history) == len(r64.t_history)
    for field in ("R", "T"):
        g = torch.stack([getattr(t, field) for t in got.t_history])
        ref = torch.stack([getattr(t, field) for t in r64.t_history])
        f32 = torch.stack([getattr(t, field) for t in r32.t_history])
        report(f"icp plane {name}{tag} history {field}", g, ref)
        report(f"icp plane {name}{tag} history {field} (float32 moments)", f32, ref)
        report(f"icp plane {name}{tag} final {field}", getattr(got.RTs, field), getattr(r64.RTs, field))
    s0 = kw["init"].s if "init" in kw else torch.ones(N)
    for t in [got.RTs, *got.t_history]:
        assert torch.equal(t.s.cpu(), s0)  # the scale: bitwise the initial one
    report(f"icp plane {name}{tag} rmse", got.rmse, r64.rmse)
    valid = (torch.arange(P1)[None] < (torch.full((N,), P1) if xl is None else xl)[:, None])
    report(f"icp plane {name}{tag} Xt", _padded(got.Xt).cpu() * valid[..., None], r64.Xt * valid[..., None])
    R = got.RTs.R.cpu().double()
    ortho = (torch.bmm(R, R.transpose(1, 2)) - torch.eye(3, dtype=torch.float64)).abs().max().item()
    print(f"[icp plane] {name}{tag}: {len(got.t_history)} iterations, |R R^T - I| = {ortho:.2e}")
    assert ortho <= 1e-5


@pytest.mark.parametrize("name", list(PR.CASES))
def test_matches_the_float64_restatement(name):
    got = _run(name)
    _check(name, got)
    kw = PR.case(name)[5]
    if "max_iterations" in kw:
        assert not got.converged and len(got.t_history) == kw["max_iterations"]


def _flat(sol):
    return [sol.rmse, _padded(sol.Xt), *sol.RTs] + [t for h in sol.t_history for t in h]


@pytest.mark.parametrize("name", ["chunks", "het"])
def test_bitwise_reproducible_and_independent_of_the_status_batch(name):
    X, Y, Yn, xl, yl, kw = PR.case(name)
    args = (X.to(DEV), Y.to(DEV), Yn.to(DEV), _dev(xl), _dev(yl))
    runs = [kernels.icp_plane(*args, status_batch=b) for b in (None, None, 1, 3, 8)]
    first = runs[0]  # the default threshold 1e-6: the runs are compared with each other, bit for bit
    assert 2 <= first[1] <= 15
    for r in runs[1:]:
        assert r[0] == first[0] and r[1] == first[1]
        for a, b in zip(first[2:], r[2:]):
            assert torch.equal(a, b)
    a, b = _run(name), _run(name)
    assert all(torch.equal(u, v) for u, v in zip(_flat(a), _flat(b)))


def test_estimated_normals_and_flipped_normals():
    """Y_normals=None is the call with estimate_pointcloud_normals(Y, 16) passed explicitly, and a normal's sign does
    not matter: J and r change sign together, so J J^T, J r and r^2 keep their bits."""
    X, Y, Yn, xl, yl, _ = PR.case("het")
    px, py = _as_pointclouds(X, xl), _as_pointclouds(Y, yl)
    est = estimate_pointcloud_normals(py, 16)
    assert est.shape == Y.shape
    a = iterative_closest_point_to_plane(px, py, neighborhood_size=16)
    b = iterative_closest_point_to_plane(px, py, est, neighborhood_size=50)  # ignored beside given normals
    assert len(a.t_history) >= 2 and all(torch.equal(u, v) for u, v in zip(_flat(a), _flat(b)))
    c = iterative_closest_point_to_plane(px, py, -est)
    assert all(torch.equal(u, v) for u, v in zip(_flat(a), _flat(c)))
    # the analytic normals flipped, and zero normals on rows past the lengths: the same again
    d, e = _run("het"), iterative_closest_point_to_plane(px, py, -Yn.to(DEV), relative_rmse_thr=PR.THR)
    assert all(torch.equal(u, v) for u, v in zip(_flat(d), _flat(e)))
    X1, Y1, _, _, _, _ = PR.case("maxd")
    full = iterative_closest_point_to_plane(X1.to(DEV), Y1.to(DEV), neighborhood_size=16, max_correspondence_distance=0.15)
    expl = iterative_closest_point_to_plane(X1.to(DEV), Y1.to(DEV), estimate_pointcloud_normals(Y1.to(DEV), 16),
                                            max_correspondence_distance=0.15)
    assert all(torch.equal(u, v) for u, v in zip(_flat(full), _flat(expl)))


def test_pointclouds_inputs_equal_the_tensor_call_with_lengths():
    X, Y, Yn, xl, yl, _ = PR.case("het")
    got = _run("het")
    assert isinstance(got.Xt, Pointclouds) and got.Xt.counts() == [300, 150, 64]
    assert got.rmse.shape == (3,) and got.RTs.R.shape == (3, 3, 3) and got.RTs.T.shape == (3, 3) and got.RTs.s.shape == (3,)
    raw = kernels.icp_plane(X.to(DEV), Y.to(DEV), Yn.to(DEV), xl.to(DEV), yl.to(DEV), relative_rmse_thr=PR.THR)
    assert raw[0] == got.converged and raw[1] == len(got.t_history)
    assert torch.equal(raw[2], got.rmse) and torch.equal(raw[3], got.Xt.points_padded())
    assert torch.equal(raw[4][:, :9].reshape(3, 3, 3), got.RTs.R) and torch.equal(raw[4][:, 9:12], got.RTs.T)
    # full clouds through Pointclouds against plain tensors
    X2, Y2, Yn2, _, _, _ = PR.case("maxd")
    a = iterative_closest_point_to_plane(Pointclouds(X2.to(DEV)), Pointclouds(Y2.to(DEV)), Yn2.to(DEV))
    b = iterative_closest_point_to_plane(X2.to(DEV), Y2.to(DEV), Yn2.to(DEV))
    assert isinstance(a.Xt, Pointclouds) and torch.is_tensor(b.Xt)
    assert all(torch.equal(u, v) for u, v in zip(_flat(a), _flat(b)))


def test_without_iterations_and_with_an_empty_source():
    X, Y, Yn, _, _, _ = PR.case("chunks")
    g = torch.Generator().manual_seed(5)
    init = SimilarityTransform(rotations(torch.randn(2, 3, generator=g), torch.tensor([0.3, 1.0])).float().to(DEV),
                               torch.randn(2, 3, generator=g).to(DEV), torch.tensor([0.5, 2.0]).to(DEV))
    got = iterative_closest_point_to_plane(X.to(DEV), Y.to(DEV), Yn.to(DEV), init_transform=init, max_iterations=0)
    assert got.converged is False and got.rmse is None and got.t_history == []
    report("icp plane max_iterations=0 Xt", got.Xt, apply_ref(X.double(), *(t.cpu().double() for t in init)))
    for a, b in zip(got.RTs, init):
        assert torch.equal(a, b)
    # an empty source cloud beside a full one: it keeps the identity with rmse 0; the full one as if alone
    Xh, Yh, Ynh, _, _, _ = PR.case("het")
    src = Pointclouds([Xh[0].to(DEV), Xh[1, :0].to(DEV)])
    tgt = Pointclouds([Yh[0].to(DEV), Yh[1, :257].to(DEV)])
    got = iterative_closest_point_to_plane(src, tgt, Ynh[:2].to(DEV), max_iterations=3)
    alone = iterative_closest_point_to_plane(Xh[:1].to(DEV), Yh[:1].to(DEV), Ynh[:1].to(DEV), max_iterations=3)
    assert torch.equal(got.RTs.R[1].cpu(), torch.eye(3)) and got.RTs.T[1].abs().max() == 0 and got.RTs.s[1] == 1
    assert got.rmse[1] == 0 and len(got.t_history) == len(alone.t_history) == 3
    assert got.converged == alone.converged  # a cloud without a pair counts as done
    assert torch.equal(got.RTs.R[0], alone.RTs.R[0]) and torch.equal(got.RTs.T[0], alone.RTs.T[0])
    assert torch.equal(got.rmse[0], alone.rmse[0])


def test_a_planar_target():
    """400 points on z = 0 with normals +z, a tilted and lifted source: A has three null directions (the rotation about
    the normal and the two in-plane shifts), which the damping leaves at zero. Every result is finite, the final rmse
    is <= 1e-6 and the source ends on the plane."""
    g = torch.Generator().manual_seed(11)
    Y = torch.cat([2.0 * torch.rand(400, 2, generator=g) - 1.0, torch.zeros(400, 1)], dim=1)[None]
    Yn = torch.tensor([0.0, 0.0, 1.0]).expand_as(Y).contiguous()
    flat = torch.cat([1.6 * torch.rand(300, 2, generator=g) - 0.8, torch.zeros(300, 1)], dim=1)[None]
    tilt = rotations(torch.tensor([[1.0, 0.5, 0.0]]), torch.tensor([math.radians(8.0)])).float()
    X = torch.bmm(flat, tilt) + torch.tensor([0.0, 0.0, 0.07])
    got = iterative_closest_point_to_plane(X.to(DEV), Y.to(DEV), Yn.to(DEV), max_iterations=20)
    for t in _flat(got):
        assert torch.isfinite(t).all()
    print(f"[icp plane] planar target: {len(got.t_history)} iterations, converged {got.converged}, rmse "
          f"{got.rmse.item():.2e}, max |z| {got.Xt[..., 2].abs().max().item():.2e}")
    assert got.rmse.item() <= 1e-6
    assert got.Xt[..., 2].abs().max().item() <= 1e-5
    ref = PR.icp_plane_ref(X, Y, Yn, max_iterations=20)
    assert ref.rmse.item() <= 1e-6 and ref.Xt[..., 2].abs().max().item() <= 1e-5


def test_a_cloud_whose_every_pair_is_rejected():
    """Cloud 1 lies 5 units away from its target and the maximum distance is 0.3: no pair, so it keeps its initial
    transform, reports rmse 0 and does not keep the batch from converging; cloud 0 registers as if alone."""
    X, Y, Yn, _, _, _ = PR.case("chunks")
    X = X.clone()
    X[1] += 5.0
    g = torch.Generator().manual_seed(6)
    init = SimilarityTransform(rotations(torch.randn(2, 3, generator=g), torch.tensor([0.0, 0.4])).float().to(DEV),
                               torch.tensor([[0.0, 0.0, 0.0], [0.1, -0.2, 0.3]]).to(DEV), torch.ones(2).to(DEV))
    kw = dict(init_transform=init, max_correspondence_distance=0.3)
    got = iterative_closest_point_to_plane(X.to(DEV), Y.to(DEV), Yn.to(DEV), **kw)
    alone = iterative_closest_point_to_plane(X[:1].to(DEV), Y[:1].to(DEV), Yn[:1].to(DEV),
                                             init_transform=SimilarityTransform(*(t[:1] for t in init)),
                                             max_correspondence_distance=0.3)
    assert got.converged and alone.converged and len(got.t_history) == len(alone.t_history) >= 2
    assert got.rmse[1] == 0
    for h in [got.RTs, *got.t_history]:
        assert torch.equal(h.R[1], init.R[1]) and torch.equal(h.T[1], init.T[1]) and torch.equal(h.s[1], init.s[1])
    assert torch.equal(got.RTs.R[0], alone.RTs.R[0]) and torch.equal(got.RTs.T[0], alone.RTs.T[0])
    assert torch.equal(got.rmse[0], alone.rmse[0])
    ref = PR.icp_plane_ref(X, Y, Yn, init=tuple(t.cpu() for t in init), max_correspondence_distance=0.3)
    assert ref.converged and not any(v[1].any() for v in ref.valid_history)  # the restatement rejects them all too
    assert torch.equal(ref.RTs.R[1], init.R[1].cpu()) and torch.equal(ref.RTs.T[1], init.T[1].cpu())
    # only rejected pairs at all: one iteration, converged, nothing moved
    lone = iterative_closest_point_to_plane(X[1:].to(DEV), Y[1:].to(DEV), Yn[1:].to(DEV), max_correspondence_distance=0.3)
    assert lone.converged and len(lone.t_history) == 1 and lone.rmse[0] == 0
    assert torch.equal(lone.RTs.R[0].cpu(), torch.eye(3)) and lone.RTs.T.abs().max() == 0
    assert torch.equal(lone.Xt, X[1:].to(DEV))


def test_a_cloud_of_four_points_is_finite():
    """Four pairs against six unknowns: under-determined, so no parity (the damping decides the step); shapes and
    finiteness only, beside a one-point cloud."""
    g = torch.Generator().manual_seed(3)
    x4, y4 = torch.randn(2, 4, 3, generator=g), torch.randn(2, 4, 3, generator=g)
    n4 = torch.nn.functional.normalize(torch.randn(2, 4, 3, generator=g), dim=2)
    got = iterative_closest_point_to_plane(Pointclouds([x4[0].to(DEV), x4[1, :1].to(DEV)]), Pointclouds(y4.to(DEV)),
                                           n4.to(DEV), max_iterations=3)
    assert 1 <= len(got.t_history) <= 3 and got.rmse.shape == (2,) and got.Xt.counts() == [4, 1]
    for t in _flat(got):
        assert torch.isfinite(t).all()
    assert torch.equal(got.RTs.s.cpu(), torch.ones(2))


def test_point_to_plane_needs_fewer_iterations_than_point_to_point():
    """The reason for the estimator: on the smooth "tiles" cloud it stops well before the point-to-point loop does."""
    X, Y, Yn, _, _, kw = PR.case("tiles")
    plane = iterative_closest_point_to_plane(X.to(DEV), Y.to(DEV), Yn.to(DEV), **_kw(kw))
    point = iterative_closest_point(X.to(DEV), Y.to(DEV), relative_rmse_thr=kw["relative_rmse_thr"])
    print(f"[icp plane] tiles: point-to-plane {len(plane.t_history)} iterations, point-to-point {len(point.t_history)}")
    assert plane.converged and len(plane.t_history) < len(point.t_history)
