"""iterative_closest_point and corresponding_points_alignment (csrc/mr_points.hip, k_icp_*) on the GPU against the
float64 restatement of tests/icp_ref.py run on the CPU.

* ICP, every case of icp_ref.CASES (whose float32 and float64 restatements make the same decisions:
  test_icp_cpu.py::test_input_condition_of_the_gpu_cases): ``converged`` and the number of iterations equal the float64
  restatement's; every R, T, s of the history, the final RTs, rmse and Xt within 1e-4 * max(1, |ref|) of it, the
  float32 restatement's own error printed beside;
* Pointclouds inputs, max_iterations = 0, an empty source cloud;
* corresponding_points_alignment alone: random weights with zeros, the mirrored cloud both ways, scale, lengths;
* bitwise: run to run, and the status read back after every iteration against once at the end;
* chamfer_distance on Pointclouds equals the tensor call with the same lengths.
"""
import pytest
import torch

from tests import icp_ref as I
from tests.helpers import report
from torch_renderer_amd import Pointclouds, kernels
from torch_renderer_amd.loss import chamfer_distance
from torch_renderer_amd.ops import SimilarityTransform, corresponding_points_alignment, iterative_closest_point

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(t):
    return None if t is None else t.to(DEV)


def _as_pointclouds(t, lengths):
    n = [t.shape[1]] * t.shape[0] if lengths is None else lengths.tolist()
    return Pointclouds([t[i, :n[i]].to(DEV) for i in range(t.shape[0])])


def _run(name, pointclouds=False, **over):
    X, Y, xl, yl, kw = I.case(name)
    kw = dict(kw, **over)
    init = kw.pop("init", None)
    if init is not None:
        kw["init_transform"] = SimilarityTransform(*(t.to(DEV) for t in init))
    if pointclouds or xl is not None or yl is not None:  # lengths travel in Pointclouds, as upstream
        return iterative_closest_point(_as_pointclouds(X, xl), _as_pointclouds(Y, yl), **kw)
    return iterative_closest_point(X.to(DEV), Y.to(DEV), **kw)


def _check(name, got, tag=""):
    r32, r64 = I.restated(name, torch.float32), I.restated(name, torch.float64)
    X, _, xl, _, _ = I.case(name)
    assert got.converged == r64.converged
    assert len(got.t_history) == len(r64.t_history)
    for field in ("R", "T", "s"):
        g = torch.stack([getattr(t, field) for t in got.t_history])
        ref = torch.stack([getattr(t, field) for t in r64.t_history])
        f32 = torch.stack([getattr(t, field) for t in r32.t_history])
        report(f"icp {name}{tag} history {field}", g, ref)
        report(f"icp {name}{tag} history {field} (float32 restatement)", f32, ref)
        report(f"icp {name}{tag} final {field}", getattr(got.RTs, field), getattr(r64.RTs, field))
    report(f"icp {name}{tag} rmse", got.rmse, r64.rmse)
    report(f"icp {name}{tag} rmse (float32 restatement)", r32.rmse, r64.rmse)
    xt = got.Xt.points_padded() if isinstance(got.Xt, Pointclouds) else got.Xt
    valid = (torch.arange(X.shape[1])[None] < (torch.full((X.shape[0],), X.shape[1]) if xl is None else xl)[:, None])
    report(f"icp {name}{tag} Xt", xt.cpu() * valid[..., None], r64.Xt * valid[..., None])
    report(f"icp {name}{tag} Xt (float32 restatement)", r32.Xt * valid[..., None], r64.Xt * valid[..., None])


@pytest.mark.parametrize("name", list(I.CASES))
def test_icp_matches_the_float64_restatement(name):
    got = _run(name)
    _check(name, got)
    if "max_iterations" in I.CASES[name][6]:
        assert not got.converged and len(got.t_history) == I.CASES[name][6]["max_iterations"]


def test_icp_pointclouds_inputs():
    """Full clouds through Pointclouds: Xt comes back as a Pointclouds of the source's sizes."""
    got = _run("many-64", pointclouds=True)
    assert isinstance(got.Xt, Pointclouds) and got.Xt.counts() == [64] * 70
    _check("many-64", got, " (Pointclouds)")
    het = _run("het")
    assert isinstance(het.Xt, Pointclouds) and het.Xt.counts() == [300, 150, 40]
    assert het.rmse.shape == (3,) and het.RTs.R.shape == (3, 3, 3) and het.RTs.T.shape == (3, 3) and het.RTs.s.shape == (3,)


def test_icp_without_iterations_and_with_an_empty_source():
    X, Y, _, _, _ = I.case("scale")
    g = torch.Generator().manual_seed(5)
    init = SimilarityTransform(I.rotations(torch.randn(2, 3, generator=g), torch.tensor([0.3, 1.0])).float().to(DEV),
                               torch.randn(2, 3, generator=g).to(DEV), torch.tensor([0.5, 2.0]).to(DEV))
    got = iterative_closest_point(X.to(DEV), Y.to(DEV), init_transform=init, max_iterations=0)
    assert got.converged is False and got.rmse is None and got.t_history == []
    ref = I.apply_ref(X.double(), *(t.cpu().double() for t in init))
    report("icp max_iterations=0 Xt", got.Xt, ref)
    for a, b in zip(got.RTs, init):
        assert torch.equal(a, b)
    # an empty source cloud beside a full one: identity, rmse 0; the full one as if alone
    Xh, Yh, _, _, _ = I.case("het")
    src = Pointclouds([Xh[0].to(DEV), Xh[1, :0].to(DEV)])
    tgt = Pointclouds([Yh[0].to(DEV), Yh[1, :64].to(DEV)])
    got = iterative_closest_point(src, tgt, max_iterations=3)
    alone = iterative_closest_point(Xh[:1].to(DEV), Yh[:1].to(DEV), max_iterations=3)
    assert torch.equal(got.RTs.R[1].cpu(), torch.eye(3)) and got.RTs.T[1].abs().max() == 0 and got.RTs.s[1] == 1
    assert got.rmse[1] == 0 and not got.converged  # 0 / 0 is a NaN drop: never converged, as upstream
    assert torch.equal(got.RTs.R[0], alone.RTs.R[0]) and torch.equal(got.rmse[0], alone.rmse[0])


def _align_inputs(seed=3, N=5, P=1500):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, P, 3, generator=g)
    R = I.rotations(torch.randn(N, 3, generator=g), 3.0 * torch.rand(N, generator=g)).float()
    T = torch.randn(N, 3, generator=g)
    s = 0.5 + torch.rand(N, generator=g)
    Y = I.apply_ref(X, R, T, s) + 0.05 * torch.randn(N, P, 3, generator=g)
    w = torch.rand(N, P, generator=g)
    w[torch.rand(N, P, generator=g) < 0.3] = 0.0
    return X, Y, w


@pytest.mark.parametrize("estimate_scale", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_alignment_matches_the_float64_restatement(weighted, estimate_scale):
    """1500 points: two tiles of partial sums a cloud; large rotations; weights with 30% zeros."""
    X, Y, w = _align_inputs()
    w = w if weighted else None
    got = corresponding_points_alignment(X.to(DEV), Y.to(DEV), weights=_dev(w), estimate_scale=estimate_scale)
    ref = I.align_ref(X, Y, w, estimate_scale=estimate_scale)
    f32 = I.align_ref(X, Y, w, estimate_scale=estimate_scale, dtype=torch.float32)
    for field in ("R", "T", "s"):
        report(f"alignment w={weighted} scale={estimate_scale} {field}", getattr(got, field), getattr(ref, field))
        report(f"alignment w={weighted} scale={estimate_scale} {field} (float32 restatement)", getattr(f32, field),
               getattr(ref, field))
    if not estimate_scale:
        assert torch.equal(got.s.cpu(), torch.ones(5))


def test_alignment_of_a_mirrored_cloud_and_of_pointclouds():
    g = torch.Generator().manual_seed(4)
    X = torch.randn(2, 257, 3, generator=g)
    M = torch.diag(torch.tensor([1.0, -1.0, 1.0]))
    Y = X @ M + torch.tensor([0.2, 0.0, -0.4])
    for reflect in (False, True):
        got = corresponding_points_alignment(X.to(DEV), Y.to(DEV), allow_reflection=reflect)
        ref = I.align_ref(X, Y, allow_reflection=reflect)
        for field in ("R", "T", "s"):
            report(f"alignment mirrored reflect={reflect} {field}", getattr(got, field), getattr(ref, field))
        det = torch.det(got.R.cpu().double())
        assert torch.allclose(det, torch.full((2,), -1.0 if reflect else 1.0, dtype=torch.float64), atol=1e-5)
    assert torch.allclose(got.R.cpu(), M[None].expand(2, 3, 3), atol=1e-5)  # reflections allowed: the mirror itself
    # Pointclouds: the lengths weigh the padding 0
    lengths = [257, 100]
    px = Pointclouds([X[i, :n].to(DEV) for i, n in enumerate(lengths)])
    py = Pointclouds([Y[i, :n].to(DEV) for i, n in enumerate(lengths)])
    got = corresponding_points_alignment(px, py, estimate_scale=True)
    mask = (torch.arange(257)[None] < torch.tensor(lengths)[:, None]).float()
    ref = I.align_ref(X, Y, mask, estimate_scale=True)
    for field in ("R", "T", "s"):
        report(f"alignment Pointclouds {field}", getattr(got, field), getattr(ref, field))


def _flat(sol):
    xt = sol.Xt.points_padded() if isinstance(sol.Xt, Pointclouds) else sol.Xt
    return [sol.rmse, xt, *sol.RTs] + [t for h in sol.t_history for t in h]


@pytest.mark.parametrize("name", ["chunks", "het"])
def test_icp_is_bitwise_reproducible_and_independent_of_the_status_batch(name):
    X, Y, xl, yl, kw = I.case(name)
    args = (X.to(DEV), Y.to(DEV), _dev(xl), _dev(yl))
    runs = [kernels.icp(*args, status_batch=b) for b in (None, None, 1, 100)]
    first = runs[0]
    assert first[1] == len(I.restated(name, torch.float64).t_history)
    for r in runs[1:]:
        assert r[0] == first[0] and r[1] == first[1]
        for a, b in zip(first[2:], r[2:]):
            assert torch.equal(a, b)
    a, b = _run(name), _run(name)
    assert all(torch.equal(u, v) for u, v in zip(_flat(a), _flat(b)))
    X5, Y5, w5 = _align_inputs()
    one = kernels.points_alignment(X5.to(DEV), Y5.to(DEV), None, w5.to(DEV), 1)
    assert torch.equal(one, kernels.points_alignment(X5.to(DEV), Y5.to(DEV), None, w5.to(DEV), 1))


def test_chamfer_on_pointclouds_equals_the_tensor_call():
    X, Y, xl, yl, _ = I.case("het")
    px, py = _as_pointclouds(X, xl), _as_pointclouds(Y, yl)
    for kw in ({}, {"batch_reduction": None}, {"point_reduction": "sum", "single_directional": True}):
        a, _ = chamfer_distance(px, py, **kw)
        b, _ = chamfer_distance(px.points_padded(), py.points_padded(), x_lengths=xl.to(DEV), y_lengths=yl.to(DEV), **kw)
        assert torch.equal(a, b)
    full, _ = chamfer_distance(Pointclouds(X.to(DEV)), Y.to(DEV))
    assert torch.equal(full, chamfer_distance(X.to(DEV), Y.to(DEV))[0])
    leaf = X.to(DEV).requires_grad_(True)
    chamfer_distance(Pointclouds(leaf), py)[0].backward()
    assert leaf.grad is not None and leaf.grad.abs().sum() > 0
