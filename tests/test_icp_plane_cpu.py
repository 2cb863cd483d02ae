"""iterative_closest_point_to_plane without a GPU: the import path, every argument error of the Python layer (and CPU
tensors refused), the C ABI's checks before any launch, the step (6x6 damped solve, Rodrigues, update) run on the host
by the code the kernel runs (mr_icp_plane_solve_host) against numpy.linalg.solve, the restatement of
tests/icp_plane_ref.py against a hand value, and the input condition of the GPU suite: on every case of
icp_plane_ref.CASES the restatement with float32 moments makes the decisions of the float64 one."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import icp_plane_ref as PR
from torch_renderer_amd import Pointclouds, _lib, kernels
from torch_renderer_amd.ops import ICPSolution, SimilarityTransform

MR_EINVAL, MR_EUNSUPPORTED, MR_EWORKSPACE = 1, 3, 4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from torch_renderer_amd import _build

        _build.build()
    return _lib.load()


def _p2plane():
    from torch_renderer_amd.ops import iterative_closest_point_to_plane

    return iterative_closest_point_to_plane


def _clouds(N=2, P1=5, P2=7, D=3):
    g = torch.Generator().manual_seed(0)
    return torch.randn(N, P1, D, generator=g), torch.randn(N, P2, D, generator=g), torch.randn(N, P2, D, generator=g)


def test_import_path_and_signature():
    import inspect

    from torch_renderer_amd import ops

    fn = _p2plane()
    assert ops.iterative_closest_point_to_plane is fn
    assert list(inspect.signature(fn).parameters) == [
        "X", "Y", "Y_normals", "init_transform", "max_iterations", "relative_rmse_thr", "max_correspondence_distance",
        "neighborhood_size"]
    d = {k: p.default for k, p in inspect.signature(fn).parameters.items()}
    assert d["Y_normals"] is None and d["init_transform"] is None and d["max_iterations"] == 100
    assert d["relative_rmse_thr"] == 1e-6 and d["max_correspondence_distance"] is None and d["neighborhood_size"] == 50
    assert "status_batch" in inspect.signature(kernels.icp_plane).parameters
    assert ICPSolution._fields == ("converged", "rmse", "Xt", "RTs", "t_history")


def test_cpu_tensors_are_refused():
    fn = _p2plane()
    x, y, n = _clouds()
    big = torch.randn(2, 70, 3, generator=torch.Generator().manual_seed(1))
    for call in (lambda: fn(x, y, n),
                 lambda: fn(Pointclouds([x[0], x[1, :3]]), Pointclouds(y), n),
                 lambda: fn(x, y, n, max_iterations=0),
                 lambda: fn(x, y, n, max_correspondence_distance=0.5),
                 lambda: fn(x, big, neighborhood_size=16),  # the normals' own refusal
                 lambda: kernels.icp_plane(x, y, n)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_argument_errors():
    fn = _p2plane()
    x, y, n = _clouds()
    with pytest.raises(ValueError, match="same number of batches and data dimensions"):
        fn(x, y[:1], n[:1])
    x2, y2, n2 = _clouds(D=2)
    with pytest.raises(ValueError, match="same number of batches and data dimensions"):
        fn(x, y2, n2)
    with pytest.raises(NotImplementedError, match="D = 3"):
        fn(x2, y2, n2)
    with pytest.raises(ValueError, match="Pointclouds objects or tensors"):
        fn([x[0]], y, n)
    good = SimilarityTransform(torch.eye(3)[None].repeat(2, 1, 1), torch.zeros(2, 3), torch.ones(2))
    for bad in (good[:2], (good.R[:1], good.T, good.s), (good.R, good.T[:, :2], good.s), (good.R, good.T, good.s[:, None]), 5):
        with pytest.raises(ValueError, match="The initial transformation init_transform has to be"):
            fn(x, y, n, init_transform=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan"), "far", True):
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            fn(x, y, n, max_correspondence_distance=bad)
    for bad in (n[:, :6], n[:1], n[..., :2], n[0], "normals"):
        with pytest.raises(ValueError, match="Y_normals"):
            fn(x, y, bad)
    with pytest.raises(ValueError, match="Y_normals"):  # the padded shape, also beside Pointclouds
        fn(x, Pointclouds([y[0], y[1, :4]]), n[:, :4])
    for leaf in ("x", "y", "n"):
        a = [t.clone().requires_grad_(True) if k == leaf else t for k, t in zip("xyn", (x, y, n))]
        with pytest.raises(NotImplementedError, match="requires grad"):
            fn(*a)
    with pytest.raises(NotImplementedError, match="requires grad"):
        fn(x, y, n, init_transform=(good.R.clone().requires_grad_(True), good.T, good.s))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):  # grad mode off: not refused for it
        fn(x.clone().requires_grad_(True), y, n)
    with pytest.raises(ValueError, match="target cloud is empty"):
        fn(Pointclouds([x[0], x[1, :2]]), Pointclouds([y[0], y[1, :0]]), n)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # an empty target under an empty source is allowed
        fn(Pointclouds([x[0], x[1, :0]]), Pointclouds([y[0], y[1, :0]]), n)
    with pytest.raises(ValueError, match="neighborhood_size"):  # the normals' own error: 7 points, K = 50
        fn(x, y)
    with pytest.raises(TypeError):
        fn(x, y, n, estimate_scale=True)
    with pytest.raises(TypeError):
        fn(x, y, n, allow_reflection=True)


def _it(lib, **k):
    buf = k.pop("_buf")
    p = ctypes.addressof(buf)
    return lib.mr_icp_plane_iterate(k.get("x", p), k.get("y", p), k.get("yn", p), k.get("N", 2), 4, k.get("P2", 4), None,
                                    None, k.get("r2", float("inf")), 1e-6, k.get("max_it", 10), k.get("its", 1),
                                    k.get("rts", p), k.get("hist", p), k.get("rmse", p), k.get("status", p),
                                    k.get("ws", p), k.get("wsb", 1 << 40), None)


def test_abi_rejects_bad_arguments_without_touching_the_gpu(lib):
    """The codes and texts of mr_icp_iterate's checks, before any launch (no GPU here). `p` is host memory that is
    never dereferenced."""
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)

    def it(**k):
        return _it(lib, _buf=buf, **k)

    def err():
        return lib.mr_last_error()

    for key in ("x", "y", "yn", "rts", "hist", "rmse", "status", "ws"):
        assert it(**{key: None}) == MR_EINVAL and b"NULL" in err(), key
    assert it(N=0) == MR_EINVAL and b">= 1" in err()
    assert it(P2=0) == MR_EINVAL and it(N=70000) == MR_EUNSUPPORTED and b"65535" in err()
    assert it(max_it=0) == MR_EINVAL and b"max_iterations" in err()
    assert it(its=-1) == MR_EINVAL and it(wsb=16) == MR_EWORKSPACE and b"too small" in err()
    for r2 in (0.0, -1.0, float("nan")):
        assert it(r2=r2) == MR_EINVAL and b"max_dist2" in err()
    assert it(its=0) == 0 and it(its=0, r2=0.25) == 0  # nothing to enqueue
    assert lib.mr_icp_plane_workspace(0, 4, 4) == 0 and lib.mr_icp_plane_workspace(2, 1 << 31, 4) == 0
    # mr_icp_init is shared: its layout comes first, the plane estimator's sums after it
    assert lib.mr_icp_plane_workspace(300, 2000, 400) >= lib.mr_icp_workspace(300, 2000, 400) + 300 * 2 * 28 * 8
    assert lib.mr_icp_init(p, 2, 4, 4, None, None, None, None, p, p, p, lib.mr_icp_workspace(2, 4, 4) - 1,
                           None) == MR_EWORKSPACE
    one = (ctypes.c_double * 21)()
    e = lib.mr_icp_plane_solve_host
    for k in range(5):
        args = [ctypes.addressof(one)] * 5
        args[k] = None
        assert e(*args) == MR_EINVAL and b"NULL" in err()
    assert lib.mr_version() == 5
    for name, nargs in (("mr_icp_plane_workspace", 3), ("mr_icp_plane_iterate", 19), ("mr_icp_plane_solve_host", 5)):
        assert name in _lib.EXPORTED_SYMBOLS and len(getattr(lib, name).argtypes) == nargs


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 300, 200), (2, 2049, 1100), (300, 2000, 400)])
def test_entry_point_enforces_its_workspace_query(lib, shape):
    """One byte less than the queried size is refused with MR_EWORKSPACE and a "too small" text before any device
    work; the query is a multiple of 256."""
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    N, P1, P2 = shape
    need = lib.mr_icp_plane_workspace(N, P1, P2)
    assert need > lib.mr_icp_workspace(N, P1, P2) > 0 and need % 256 == 0

    def call(b):
        return lib.mr_icp_plane_iterate(p, p, p, N, P1, P2, None, None, float("inf"), 1e-6, 10, 0, p, p, p, p, p, b, None)

    assert call(need - 1) == MR_EWORKSPACE
    assert b"too small" in lib.mr_last_error()
    assert call(need) == 0  # no iteration to enqueue: nothing touches the device


# ---------------------------------------------------------------------------------------------------------------------
# The step on the host
# ---------------------------------------------------------------------------------------------------------------------
def _host_step(lib, A, b, rts, c):
    iu = np.triu_indices(6)
    A21 = np.ascontiguousarray(A[iu], dtype=np.float64)
    b6 = np.ascontiguousarray(b, dtype=np.float64)
    rin = np.ascontiguousarray(rts, dtype=np.float32)
    c3 = np.ascontiguousarray(c, dtype=np.float64)
    out = np.full(13, np.nan, dtype=np.float32)
    assert lib.mr_icp_plane_solve_host(A21.ctypes.data, b6.ctypes.data, rin.ctypes.data, c3.ctypes.data,
                                       out.ctypes.data) == 0
    return out


def _numpy_step(A, b, rts, c):
    """numpy.linalg.solve plus the float64 update, before the rounding to float32."""
    R, T = rts[:9].astype(np.float64).reshape(3, 3), rts[9:12].astype(np.float64)
    lam = 1e-9 * np.trace(A) / 6.0
    xi = np.linalg.solve(A + lam * np.eye(6), -b)
    w, th = xi[:3], np.linalg.norm(xi[:3])
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    E = np.eye(3) + (np.sin(th) / th if th > 0 else 1.0) * K + ((1 - np.cos(th)) / th ** 2 if th > 1e-7 else 0.5) * K @ K
    return np.concatenate([(R @ E.T).reshape(-1), (T - c) @ E.T + c + xi[3:], [float(rts[12])]]), xi


def _system(rng, P=60, noise=0.05, planar=False):
    """The normal equations of P random valid pairs under a random transform: (A, b, rts float32, c)."""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    th = rng.uniform(0, 3.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    rts = np.concatenate([R.reshape(-1), rng.normal(size=3), [rng.uniform(0.5, 2.0)]]).astype(np.float32)
    x = rng.normal(size=(P, 3)).astype(np.float32)
    Rf, Tf, s = rts[:9].reshape(3, 3).astype(np.float64), rts[9:12].astype(np.float64), float(rts[12])
    p = (s * (x.astype(np.float64) @ Rf) + Tf).astype(np.float32).astype(np.float64)
    c = s * (x.astype(np.float64).mean(0) @ Rf) + Tf
    if planar:
        n = np.tile(np.array([0.0, 0.0, 1.0]), (P, 1))
        q = p.copy()
        q[:, 2] = 0.3
    else:
        n = rng.normal(size=(P, 3))
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        q = p + noise * rng.normal(size=(P, 3))
    r = ((p - q) * n).sum(1)
    J = np.concatenate([np.cross(p - c, n), n], axis=1)
    return J.T @ J, J.T @ r, rts, c


def test_host_step_against_numpy(lib):
    """300 systems of random valid pairs (steps of ~0.05 rad and of ~1e-6 rad, the Rodrigues series): finite, and
    within 1e-6 of numpy.linalg.solve plus the float64 update. A planar target (A has three null directions: w_z,
    t_x, t_y): finite, the in-plane motion stays ~0 and the step closes the gap along the normal."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for k in range(300):
        A, b, rts, c = _system(rng, noise=1e-6 if k % 10 == 9 else 0.05)
        assert np.linalg.cond(A) < 1e6
        got = _host_step(lib, A, b, rts, c)
        ref, _ = _numpy_step(A, b, rts, c)
        assert np.isfinite(got).all()
        worst = max(worst, np.abs(got.astype(np.float64) - ref).max())
        assert got[12] == rts[12]  # the scale, bitwise
    print(f"[icp plane host step] 300 systems: max |rts - numpy| = {worst:.2e}")
    assert worst <= 1e-6
    for k in range(20):
        A, b, rts, c = _system(rng, planar=True)
        assert np.linalg.matrix_rank(A, tol=1e-9 * np.trace(A)) == 3
        got = _host_step(lib, A, b, rts, c)
        assert np.isfinite(got).all()
        R0, R1 = rts[:9].reshape(3, 3).astype(np.float64), got[:9].reshape(3, 3).astype(np.float64)
        E = (R0.T @ R1).T  # R1 = R0 E^T
        assert abs(E[1, 0] - E[0, 1]) < 1e-5  # no rotation about the normal
        # the source's mean c lands on the plane z = 0.3 (c -> c + t), the in-plane shift is rounding
        moved = (rts[9:12].astype(np.float64) - c) @ E.T + c + 0  # (T - c) E^T + c
        t = got[9:12].astype(np.float64) - moved
        assert abs(t[0]) < 1e-5 and abs(t[1]) < 1e-5 and abs(c[2] + t[2] - 0.3) < 1e-5
    # no pair, or only zero normals: the transform is kept bit for bit
    A, b, rts, c = _system(rng)
    assert np.array_equal(_host_step(lib, 0 * A, 0 * b, rts, c), rts)
    # a non-finite system keeps the transform too
    assert np.array_equal(_host_step(lib, A * np.nan, b, rts, c), rts)


def test_restatement_step_is_the_host_step(lib):
    """The restatement's step (torch.linalg.solve) and the library's on the same systems, to 1e-6."""
    rng = np.random.default_rng(1)
    for _ in range(20):
        A, b, rts, c = _system(rng)
        R64, T64 = PR.plane_step_ref(torch.from_numpy(A), torch.from_numpy(b), torch.from_numpy(rts[:9].reshape(3, 3)),
                                     torch.from_numpy(rts[9:12]), torch.from_numpy(c))
        got = _host_step(lib, A, b, rts, c)
        assert np.abs(got[:9].astype(np.float64) - R64.numpy().reshape(-1)).max() <= 1e-6
        assert np.abs(got[9:12].astype(np.float64) - T64.numpy()).max() <= 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# The restatement
# ---------------------------------------------------------------------------------------------------------------------
def _grid_plane(k=10):
    u = torch.linspace(-1.0, 1.0, k)
    gx, gy = torch.meshgrid(u, u, indexing="ij")
    Y = torch.stack([gx.reshape(-1), gy.reshape(-1), torch.zeros(k * k)], dim=1)[None]
    return Y, torch.tensor([0.0, 0.0, 1.0]).expand_as(Y).contiguous()


def test_hand_value_a_shift_along_the_normal_is_fixed_in_one_step(lib):
    """The source is the target (a grid on z = 0, normals +z) lifted by 0.1: every point's neighbour is the one below
    it, r = 0.1 for all, and one step gives T = (0, 0, -0.1), R = I and an rmse of 0 (to rounding)."""
    Y, Yn = _grid_plane()
    X = Y + torch.tensor([0.0, 0.0, 0.1])
    sol = PR.icp_plane_ref(X, Y, Yn, max_iterations=1)
    assert sol.nn_history[0].tolist() == [list(range(100))]
    R1, T1, s1 = sol.t_history[0]
    assert torch.allclose(R1, torch.eye(3)[None], atol=1e-6) and torch.allclose(T1, torch.tensor([[0.0, 0.0, -0.1]]), atol=1e-6)
    assert s1.tolist() == [1.0]
    assert len(sol.t_history) == 1 and sol.rmse.item() <= 1e-6
    assert sol.Xt[..., 2].abs().max() <= 1e-6
    # the same single step through the library's host code, from the pairs' normal equations
    p, c = X[0].double().numpy(), X[0].double().mean(0).numpy()
    n = Yn[0].double().numpy()
    J = np.concatenate([np.cross(p - c, n), n], axis=1)
    r = ((p - Y[0].double().numpy()) * n).sum(1)
    rts = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=np.float32)
    got = _host_step(lib, J.T @ J, J.T @ r, rts, c)
    assert np.abs(got - np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, -0.1, 1])).max() <= 1e-6
    # a flipped normal, and a zero normal beside it, change nothing
    flipped = PR.icp_plane_ref(X, Y, -Yn, max_iterations=1)
    assert all(torch.equal(a, b) for ta, tb in zip(sol.t_history, flipped.t_history) for a, b in zip(ta, tb))
    Yz = Yn.clone()
    Yz[0, ::2] = 0.0
    half = PR.icp_plane_ref(X, Y, Yz, max_iterations=1)
    assert torch.allclose(half.t_history[0].T, torch.tensor([[0.0, 0.0, -0.1]]), atol=1e-6)


def test_restatement_edge_behaviour():
    """max_iterations = 0; every pair rejected; a 4-point cloud (under-determined: shape and finiteness only)."""
    X, Y, Yn, xl, yl, _ = PR.case("het")
    none = PR.icp_plane_ref(X, Y, Yn, xl, yl, max_iterations=0)
    assert not none.converged and none.rmse is None and none.t_history == [] and torch.equal(none.Xt, X)
    far = PR.icp_plane_ref(X[:1] + 5.0, Y[:1], Yn[:1], max_correspondence_distance=1e-3, max_iterations=4)
    assert far.converged and len(far.t_history) == 1 and far.rmse.tolist() == [0.0]
    assert torch.equal(far.RTs.R, torch.eye(3)[None]) and far.RTs.T.abs().max() == 0
    assert not far.valid_history[0].any()
    g = torch.Generator().manual_seed(3)
    x4, y4 = torch.randn(1, 4, 3, generator=g), torch.randn(1, 4, 3, generator=g)
    n4 = torch.nn.functional.normalize(torch.randn(1, 4, 3, generator=g), dim=2)
    tiny = PR.icp_plane_ref(x4, y4, n4, max_iterations=3)
    assert 1 <= len(tiny.t_history) <= 3 and tiny.Xt.shape == (1, 4, 3) and tiny.rmse.shape == (1,)
    assert all(torch.isfinite(t).all() for h in tiny.t_history for t in h) and torch.isfinite(tiny.Xt).all()


@pytest.mark.parametrize("name", list(PR.CASES))
def test_input_condition_of_the_gpu_cases(name):
    """What makes the GPU comparison against the float64 restatement meaningful: with float32 moments the restatement
    runs the same number of iterations, picks the same neighbour and the same validity for every point in every
    iteration, and its history is within 1e-5 of the float64 one. An input that fails this is replaced, not
    tolerated."""
    a, b = PR.restated(name, torch.float32), PR.restated(name, torch.float64)
    assert a.converged == b.converged and len(a.t_history) == len(b.t_history) >= 1
    differ = sum(int((p != q).sum()) for p, q in zip(a.nn_history, b.nn_history))
    differ += sum(int((p != q).sum()) for p, q in zip(a.valid_history, b.valid_history))
    worst = max((u.double() - v.double()).abs().max().item()
                for ta, tb in zip(a.t_history, b.t_history) for u, v in zip(ta, tb))
    print(f"[icp plane cases] {name}: {len(b.t_history)} iterations, converged {b.converged}, {differ} decisions differ, "
          f"history f32 vs f64 moments {worst:.2e}, rmse {b.rmse.tolist()}")
    assert differ == 0
    assert worst <= 1e-5
    X, Y, Yn, xl, yl, kw = PR.case(name)
    # no stopping decision is left to rounding: every relative drop is 5x above or below the threshold
    thr = kw["relative_rmse_thr"]
    rels = torch.stack(b.rel_history[1:]) if len(b.rel_history) > 1 else torch.ones(1, 1)
    assert bool(((rels >= 5 * thr) | (rels <= thr / 5)).all()), rels
    assert (X.shape[0], X.shape[1], Y.shape[1]) == PR.CASES[name][:3]
    if "max_iterations" in kw:  # the capped case stops before it converges
        assert not b.converged and len(b.t_history) == kw["max_iterations"]
    else:
        assert b.converged and 2 <= len(b.t_history) <= 15
    if "max_correspondence_distance" in kw:
        r2 = float(torch.tensor(kw["max_correspondence_distance"], dtype=torch.float32) ** 2)
        moved = PR.displaced(X[0])
        for d2, valid, nn in zip(b.d2_history, b.valid_history, b.nn_history):
            have = nn >= 0
            assert float(((d2[have] - r2).abs() / r2).min()) > 1e-4  # no pair sits on the threshold
            assert not valid[0, moved].any() and int((~valid[have]).sum()) >= PR.DISPLACED
            assert int(valid.sum()) >= 200  # the bulk of the cloud still registers
    if "init" in kw:
        assert all(torch.equal(h.s, kw["init"].s) for h in b.t_history)  # the scale stays what the call set
    if name == "scaled":
        assert b.RTs.s.tolist() == pytest.approx([0.9] * 3)
    assert math.isfinite(float(b.rmse.max())) and float(b.rmse.max()) < 0.02  # registered: the 1e-3 noise's scale
