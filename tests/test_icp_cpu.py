"""iterative_closest_point, corresponding_points_alignment and Pointclouds without a GPU: the upstream import paths,
every argument error of the Python layer (and CPU tensors refused), Pointclouds' behaviour, the C ABI's checks before
any launch, the restatement of tests/icp_ref.py against hand values, and the input condition of the GPU suite: on
every case of icp_ref.CASES the float32 and the float64 restatement make the same decisions."""
import ctypes
import os
import warnings

import pytest
import torch

from tests import icp_ref as I
from torch_renderer_amd import Pointclouds, _lib, kernels
from torch_renderer_amd.ops import (ICPSolution, SimilarityTransform, corresponding_points_alignment,
                                    iterative_closest_point)

MR_EINVAL, MR_EUNSUPPORTED, MR_EWORKSPACE = 1, 3, 4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from torch_renderer_amd import _build

        _build.build()
    return _lib.load()


def _clouds(N=2, P1=5, P2=7, D=3):
    g = torch.Generator().manual_seed(0)
    return torch.randn(N, P1, D, generator=g), torch.randn(N, P2, D, generator=g)


def test_upstream_import_paths():
    import torch_renderer_amd
    from torch_renderer_amd import ops, structures

    assert torch_renderer_amd.Pointclouds is structures.Pointclouds is Pointclouds
    assert ops.iterative_closest_point is iterative_closest_point
    assert ops.corresponding_points_alignment is corresponding_points_alignment
    assert SimilarityTransform._fields == ("R", "T", "s")
    assert ICPSolution._fields == ("converged", "rmse", "Xt", "RTs", "t_history")
    for name in ("icp", "points_alignment", "similarity_transform"):
        assert hasattr(kernels, name), name


def test_cpu_tensors_are_refused():
    from torch_renderer_amd.loss import chamfer_distance

    x, y = _clouds()
    pc = Pointclouds([x[0], x[1, :3]])
    for call in (lambda: iterative_closest_point(x, y),
                 lambda: iterative_closest_point(pc, Pointclouds(y)),
                 lambda: iterative_closest_point(x, y, max_iterations=0),
                 lambda: corresponding_points_alignment(x, x),
                 lambda: corresponding_points_alignment(pc, pc, estimate_scale=True),
                 lambda: chamfer_distance(pc, Pointclouds(y)),
                 lambda: kernels.similarity_transform(x, torch.zeros(2, 13))):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()


def test_icp_argument_errors():
    x, y = _clouds()
    with pytest.raises(NotImplementedError, match="verbose"):
        iterative_closest_point(x, y, verbose=True)
    with pytest.raises(ValueError, match="same number of batches and data dimensions"):
        iterative_closest_point(x, y[:1])
    x2, y2 = _clouds(D=2)
    with pytest.raises(ValueError, match="same number of batches and data dimensions"):
        iterative_closest_point(x, y2)
    with pytest.raises(NotImplementedError, match="D = 3"):
        iterative_closest_point(x2, y2)
    with pytest.raises(ValueError, match="Pointclouds objects or tensors"):
        iterative_closest_point([x[0]], y)
    good = SimilarityTransform(torch.eye(3)[None].repeat(2, 1, 1), torch.zeros(2, 3), torch.ones(2))
    for bad in (good[:2], (good.R[:1], good.T, good.s), (good.R, good.T[:, :2], good.s), (good.R, good.T, good.s[:, None]),
                (good.R[:, :2], good.T, good.s), 5):
        with pytest.raises(ValueError, match="The initial transformation init_transform has to be"):
            iterative_closest_point(x, y, init_transform=bad)
    with pytest.raises(NotImplementedError, match="requires grad"):
        iterative_closest_point(x.clone().requires_grad_(True), y)
    with pytest.raises(NotImplementedError, match="requires grad"):
        iterative_closest_point(x, y, init_transform=(good.R.clone().requires_grad_(True), good.T, good.s))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):  # grad mode off: not refused for it
        iterative_closest_point(x.clone().requires_grad_(True), y)
    src = Pointclouds([x[0], x[1, :2]])
    with pytest.raises(ValueError, match="target cloud is empty"):
        iterative_closest_point(src, Pointclouds([y[0], y[1, :0]]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # an empty target under an empty source is allowed
        iterative_closest_point(Pointclouds([x[0], x[1, :0]]), Pointclouds([y[0], y[1, :0]]))


def test_alignment_argument_errors():
    x, y = _clouds()
    with pytest.raises(ValueError, match="same number of batches, points and dimensions"):
        corresponding_points_alignment(x, y)
    with pytest.raises(ValueError, match="same number of batches, points and dimensions"):
        corresponding_points_alignment(Pointclouds([x[0], x[1, :3]]), Pointclouds([x[0], x[1, :4]]))
    with pytest.raises(ValueError, match="same number of batches, points and dimensions"):
        corresponding_points_alignment(Pointclouds([x[0], x[1, :3]]), x)
    for w in (torch.ones(2, 4), torch.ones(2), torch.ones(1, 5)):
        with pytest.raises(ValueError, match="weights should have the same first two dimensions"):
            corresponding_points_alignment(x, x, weights=w)
    x2, _ = _clouds(D=2)
    with pytest.raises(NotImplementedError, match="D = 3"):
        corresponding_points_alignment(x2, x2)
    with pytest.raises(NotImplementedError, match="requires grad"):
        corresponding_points_alignment(x.clone().requires_grad_(True), x)
    with pytest.raises(NotImplementedError, match="requires grad"):
        corresponding_points_alignment(x, x, weights=torch.ones(2, 5, requires_grad=True))
    with pytest.warns(UserWarning, match="cannot return a unique rotation"), pytest.raises(RuntimeError):
        corresponding_points_alignment(x[:, :3], x[:, :3])
    with pytest.warns(UserWarning, match="cannot return a unique rotation"), pytest.raises(RuntimeError):
        corresponding_points_alignment(Pointclouds([x[0], x[1, :3]]), Pointclouds([x[0], x[1, :3]]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # four points: no warning
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            corresponding_points_alignment(x[:, :4], x[:, :4])


def test_chamfer_takes_pointclouds_and_refuses_lengths_beside_them():
    from torch_renderer_amd.loss import chamfer_distance

    x, y = _clouds()
    px, py = Pointclouds([x[0], x[1, :3]]), Pointclouds(y)
    with pytest.raises(ValueError, match="x_lengths must be None"):
        chamfer_distance(px, py, x_lengths=torch.tensor([5, 3]))
    with pytest.raises(ValueError, match="y_lengths must be None"):
        chamfer_distance(x, py, y_lengths=torch.tensor([7, 7]))
    with pytest.raises(ValueError):
        chamfer_distance(px, Pointclouds(y[:1]))
    with pytest.raises(NotImplementedError):
        chamfer_distance([x[0]], y)


def test_pointclouds_behaviour():
    g = torch.Generator().manual_seed(1)
    pts = [torch.randn(5, 3, generator=g), torch.randn(0, 3), torch.randn(2, 3, generator=g)]
    pc = Pointclouds(pts)
    assert len(pc) == 3 and not pc.isempty() and pc.device == torch.device("cpu")
    assert pc.counts() == [5, 0, 2]
    n = pc.num_points_per_cloud()
    assert n.dtype == torch.int64 and n.tolist() == [5, 0, 2]
    pad = pc.points_padded()
    assert pad.shape == (3, 5, 3) and pc.points_padded() is pad  # cached
    assert torch.equal(pad[0], pts[0]) and pad[1].abs().max() == 0 and torch.equal(pad[2, :2], pts[2])
    assert pad[2, 2:].abs().max() == 0
    assert all(torch.equal(a, b) for a, b in zip(pc.points_list(), pts))
    assert torch.equal(pc.points_packed(), torch.cat(pts, 0))
    # padded -> list -> padded
    full = Pointclouds(pad)
    assert len(full) == 3 and full.counts() == [5, 5, 5] and full.points_padded() is pad
    assert all(torch.equal(a, pad[i]) for i, a in enumerate(full.points_list()))
    assert torch.equal(Pointclouds(full.points_list()).points_padded(), pad)
    # update_padded keeps the sizes
    new = pc.update_padded(pad + 1.0)
    assert new.counts() == [5, 0, 2] and torch.equal(new.points_list()[2], pts[2] + 1.0)
    assert new.points_list()[1].shape == (0, 3) and torch.equal(pc.points_padded(), pad)
    with pytest.raises(ValueError):
        pc.update_padded(pad[:, :4])
    # to / clone / detach
    moved = pc.to("cpu")
    assert moved.counts() == pc.counts() and torch.equal(moved.points_padded(), pad)
    leaf = torch.randn(4, 3, generator=g).requires_grad_(True)
    pg = Pointclouds([leaf * 2.0])
    assert pg.points_list()[0].requires_grad and not pg.detach().points_list()[0].requires_grad
    c = pc.clone()
    c.points_list()[0].add_(1.0)
    assert torch.equal(pc.points_list()[0], pts[0])
    # empties and refusals
    assert Pointclouds([]).isempty() and len(Pointclouds([])) == 0
    assert Pointclouds([torch.zeros(0, 3)]).isempty()
    with pytest.raises(NotImplementedError):
        Pointclouds(pts, normals=[torch.zeros_like(p) for p in pts])
    with pytest.raises(NotImplementedError):
        Pointclouds(pts, features=[torch.zeros_like(p) for p in pts])
    with pytest.raises(ValueError):
        Pointclouds([torch.zeros(4, 2)])
    with pytest.raises(ValueError):
        Pointclouds(torch.zeros(4, 3))
    with pytest.raises(ValueError):
        Pointclouds("clouds")


def test_abi_rejects_bad_arguments_without_touching_the_gpu(lib):
    """NULL pointers, N = 0, bad flags: a status and a message before any memset or launch (no GPU here). `p` is host
    memory that is never dereferenced."""
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    big = 1 << 40

    def err():
        return lib.mr_last_error()

    def init(**k):
        return lib.mr_icp_init(k.get("x", p), k.get("N", 2), k.get("P1", 4), 4, None, k.get("R0", None), None, None,
                               k.get("rts", p), k.get("status", p), k.get("ws", p), k.get("wsb", big), None)

    def it(**k):
        return lib.mr_icp_iterate(k.get("x", p), k.get("y", p), k.get("N", 2), 4, k.get("P2", 4), None, None,
                                  k.get("flags", 0), 1e-6, k.get("max_it", 10), k.get("its", 1), k.get("rts", p),
                                  k.get("hist", p), k.get("rmse", p), k.get("status", p), k.get("ws", p),
                                  k.get("wsb", big), None)

    def align(**k):
        return lib.mr_points_alignment(k.get("x", p), k.get("y", p), k.get("N", 2), k.get("P", 4), None, None,
                                       k.get("flags", 0), k.get("eps", 1e-9), k.get("rts", p), k.get("ws", p),
                                       k.get("wsb", big), None)

    assert init(x=None) == MR_EINVAL and b"NULL" in err()
    assert init(rts=None) == MR_EINVAL and init(status=None) == MR_EINVAL and init(ws=None) == MR_EINVAL
    assert init(N=0) == MR_EINVAL and b">= 1" in err()
    assert init(P1=0) == MR_EINVAL and init(N=70000) == MR_EUNSUPPORTED and b"65535" in err()
    assert init(R0=p) == MR_EINVAL and b"go together" in err()
    assert init(wsb=16) == MR_EWORKSPACE
    for key in ("x", "y", "rts", "hist", "rmse", "status", "ws"):
        assert it(**{key: None}) == MR_EINVAL and b"NULL" in err(), key
    assert it(N=0) == MR_EINVAL and it(P2=0) == MR_EINVAL and it(N=70000) == MR_EUNSUPPORTED
    assert it(flags=4) == MR_EINVAL and b"flags" in err()
    assert it(max_it=0) == MR_EINVAL and b"max_iterations" in err()
    assert it(its=-1) == MR_EINVAL and it(wsb=16) == MR_EWORKSPACE
    assert it(its=0) == 0  # nothing to enqueue
    for key in ("x", "y", "rts", "ws"):
        assert align(**{key: None}) == MR_EINVAL and b"NULL" in err(), key
    assert align(N=0) == MR_EINVAL and align(P=0) == MR_EINVAL and align(N=70000) == MR_EUNSUPPORTED
    assert align(flags=8) == MR_EINVAL and b"flags" in err()
    assert align(eps=-1.0) == MR_EINVAL and align(eps=float("nan")) == MR_EINVAL and b"eps" in err()
    assert align(wsb=16) == MR_EWORKSPACE
    assert lib.mr_icp_transform(None, 2, 4, p, p, None) == MR_EINVAL and b"NULL" in err()
    assert lib.mr_icp_transform(p, 2, 4, None, p, None) == MR_EINVAL
    assert lib.mr_icp_transform(p, 2, 4, p, None, None) == MR_EINVAL
    assert lib.mr_icp_transform(p, 0, 4, p, p, None) == MR_EINVAL
    assert lib.mr_icp_workspace(0, 4, 4) == 0 and lib.mr_icp_workspace(2, 1 << 31, 4) == 0
    assert lib.mr_points_alignment_workspace(2, 0) == 0
    assert lib.mr_icp_workspace(300, 2000, 400) >= 300 * 2000 * 12
    assert lib.mr_version() == 5
    for name in ("mr_icp_workspace", "mr_icp_init", "mr_icp_iterate", "mr_icp_transform",
                 "mr_points_alignment_workspace", "mr_points_alignment"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 300, 200), (2, 2049, 1100), (300, 2000, 400)])
@pytest.mark.parametrize("entry", ["mr_icp_init", "mr_icp_iterate", "mr_points_alignment"])
def test_entry_point_enforces_its_workspace_query(lib, entry, shape):
    """One byte less than the queried size is refused with MR_EWORKSPACE and a "too small" text before any device
    work, and the query is a multiple of 256 (tests/test_workspace_cpu.py's check, for the new entry points)."""
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    N, P1, P2 = shape
    if entry == "mr_points_alignment":
        need = lib.mr_points_alignment_workspace(N, P1)
        call = lambda b: lib.mr_points_alignment(p, p, N, P1, None, None, 0, 1e-9, p, p, b, None)  # noqa: E731
    elif entry == "mr_icp_init":
        need = lib.mr_icp_workspace(N, P1, P2)
        call = lambda b: lib.mr_icp_init(p, N, P1, P2, None, None, None, None, p, p, p, b, None)  # noqa: E731
    else:
        need = lib.mr_icp_workspace(N, P1, P2)
        call = lambda b: lib.mr_icp_iterate(p, p, N, P1, P2, None, None, 0, 1e-6, 10, 1, p, p, p, p, p, b,  # noqa: E731
                                            None)
    assert need > 0 and need % 256 == 0
    assert call(need - 1) == MR_EWORKSPACE
    assert b"too small" in lib.mr_last_error()


def _rot_z(deg):
    a = torch.tensor(deg * 3.141592653589793 / 180.0, dtype=torch.float64)
    return torch.stack([torch.stack([a.cos(), a.sin(), a * 0]), torch.stack([-a.sin(), a.cos(), a * 0]),
                        torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)])


def test_restatement_against_hand_values():
    """The yardstick itself: exact correspondences give the transform back; a mirrored cloud gives a proper rotation,
    or the mirror when reflections are allowed; a known scale; zero weights are ignored."""
    g = torch.Generator().manual_seed(2)
    X = torch.randn(1, 12, 3, generator=g, dtype=torch.float64)
    R, T = _rot_z(30.0)[None], torch.tensor([[0.5, -1.0, 2.0]], dtype=torch.float64)
    assert R[0, 0, 1].item() == pytest.approx(0.5)  # row vectors: x R turns the x axis towards +y
    Y = torch.bmm(X, R) + T[:, None]
    got = I.align_ref(X, Y)
    assert torch.allclose(got.R, R, atol=1e-12) and torch.allclose(got.T, T, atol=1e-12) and got.s.tolist() == [1.0]
    # a known scale
    got = I.align_ref(X, 2.5 * torch.bmm(X, R) + T[:, None], estimate_scale=True)
    assert torch.allclose(got.R, R, atol=1e-12) and torch.allclose(got.T, T, atol=1e-12)
    assert got.s.item() == pytest.approx(2.5, abs=1e-12)
    assert I.align_ref(X, 2.5 * torch.bmm(X, R) + T[:, None]).s.item() == 1.0  # not estimated: 1
    # a mirrored cloud
    M = torch.diag(torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64))[None]
    Ym = torch.bmm(X, M)
    proper = I.align_ref(X, Ym)
    assert torch.det(proper.R).item() == pytest.approx(1.0, abs=1e-12)
    assert torch.allclose(torch.bmm(proper.R, proper.R.transpose(1, 2)), torch.eye(3, dtype=torch.float64)[None], atol=1e-12)
    mirror = I.align_ref(X, Ym, allow_reflection=True)
    assert torch.allclose(mirror.R, M, atol=1e-12) and torch.det(mirror.R).item() == pytest.approx(-1.0, abs=1e-12)
    # zero weights are ignored: the last four targets are garbage
    w = torch.ones(1, 12, dtype=torch.float64)
    w[0, 8:] = 0.0
    Yg = Y.clone()
    Yg[0, 8:] = 100.0 * torch.randn(4, 3, generator=g, dtype=torch.float64)
    got = I.align_ref(X, Yg, weights=w)
    assert torch.allclose(got.R, R, atol=1e-12) and torch.allclose(got.T, T, atol=1e-12)
    assert not torch.allclose(I.align_ref(X, Yg).R, R, atol=1e-3)
    # no weight at all: the identity
    none = I.align_ref(X, Y, weights=torch.zeros(1, 12))
    assert torch.equal(none.R[0], torch.eye(3, dtype=torch.float64)) and none.T.abs().max() == 0 and none.s.item() == 1.0
    # ICP on exact correspondences of a small motion: one iteration finds it, the second confirms it
    Xs = torch.randn(1, 30, 3, generator=g)
    Rs = I.rotations(torch.tensor([[0.0, 0.0, 1.0]]), torch.tensor([0.05])).float()
    Ys = torch.bmm(Xs, Rs) + 0.01
    sol = I.icp_ref(Xs, Ys)
    assert sol.converged and len(sol.t_history) == len(sol.nn_history) == 2
    assert sol.nn_history[0].tolist() == [list(range(30))]
    assert torch.allclose(sol.RTs.R, Rs.double(), atol=1e-6) and torch.allclose(sol.RTs.T, torch.full((1, 3), 0.01).double(), atol=1e-6)
    assert sol.rmse.item() < 1e-6 and torch.allclose(sol.Xt, Ys.double(), atol=1e-6)
    capped = I.icp_ref(Xs, Ys, max_iterations=1)
    assert not capped.converged and len(capped.t_history) == 1
    none = I.icp_ref(Xs, Ys, max_iterations=0)
    assert not none.converged and none.rmse is None and none.t_history == [] and torch.equal(none.Xt, Xs.double())


@pytest.mark.parametrize("name", list(I.CASES))
def test_input_condition_of_the_gpu_cases(name):
    """What makes the GPU comparison against the float64 restatement meaningful: in float32 the restatement runs the
    same number of iterations and picks the same neighbour for every point in every iteration, and its history is
    within 1e-5 of the float64 one. An input that fails this is replaced, not tolerated."""
    a, b = I.restated(name, torch.float32), I.restated(name, torch.float64)
    assert a.converged == b.converged and len(a.t_history) == len(b.t_history) >= 1
    differ = sum(int((p != q).sum()) for p, q in zip(a.nn_history, b.nn_history))
    worst = max((u.double() - v).abs().max().item() for ta, tb in zip(a.t_history, b.t_history) for u, v in zip(ta, tb))
    print(f"[icp cases] {name}: {len(b.t_history)} iterations, converged {b.converged}, {differ} neighbours differ, "
          f"history f32 vs f64 {worst:.2e}")
    assert differ == 0
    assert worst <= 1e-5
    opts = I.CASES[name][6]
    if "max_iterations" in opts:  # the capped case stops before it converges
        assert not b.converged and len(b.t_history) == opts["max_iterations"]
    else:
        assert b.converged and 2 <= len(b.t_history) <= 13
