"""transforms.euler_angles_to_matrix, loss.posed_chamfer_distance and the entry points behind it
(mr_posed_chamfer, csrc/mr_points.hip) without a GPU: the rotation formula against the product of its axis matrices,
the import paths and argument checks of the Python layer, the C ABI's checks before any launch, and the restatement
of tests/pose_chamfer_ref.py against hand-computed values."""
import ctypes
import itertools
import math
import os

import pytest
import torch

from tests import pose_chamfer_ref as PR
from torch_renderer_amd import _lib, kernels
from torch_renderer_amd.transforms import euler_angles_to_matrix

CONVENTIONS = ["".join(p) for p in itertools.product("XYZ", repeat=3) if p[0] != p[1] and p[1] != p[2]]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from torch_renderer_amd import _build

        _build.build()
    return _lib.load()


def _axis(letter, a):
    c, s = math.cos(a), math.sin(a)
    return torch.tensor({"X": [[1, 0, 0], [0, c, -s], [0, s, c]], "Y": [[c, 0, s], [0, 1, 0], [-s, 0, c]],
                         "Z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[letter], dtype=torch.float64)


# --------------------------------------------------------------------------- euler_angles_to_matrix
def test_euler_quarter_turn_about_x():
    R = euler_angles_to_matrix(torch.tensor([math.pi / 2, 0.0, 0.0], dtype=torch.float64), "XYZ")
    assert R.shape == (3, 3)
    assert torch.allclose(R, torch.tensor([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=torch.float64), atol=1e-15)


def test_there_are_twelve_conventions():
    assert len(CONVENTIONS) == 12 and "XYZ" in CONVENTIONS and "ZXZ" in CONVENTIONS


@pytest.mark.parametrize("convention", CONVENTIONS)
def test_euler_convention_is_the_product_of_its_axis_matrices(convention):
    g = torch.Generator().manual_seed(3)
    ang = (torch.rand(6, 3, generator=g, dtype=torch.float64) - 0.5) * 6.0
    R = euler_angles_to_matrix(ang, convention)
    for k in range(ang.shape[0]):
        a, b, c = (_axis(l, float(v)) for l, v in zip(convention, ang[k]))
        assert (R[k] - a @ b @ c).abs().max() < 1e-12
    eye = torch.eye(3, dtype=torch.float64)
    assert (R @ R.transpose(1, 2) - eye).abs().max() < 1e-12
    assert (torch.linalg.det(R) - 1.0).abs().max() < 1e-12


def test_euler_batch_shapes_and_dtype():
    for shape in ((3,), (5, 3), (2, 4, 3)):
        a = torch.zeros(shape)
        R = euler_angles_to_matrix(a, "ZYX")
        assert R.shape == shape[:-1] + (3, 3) and R.dtype == torch.float32
        assert torch.equal(R, torch.eye(3).expand(R.shape))


def test_euler_error_messages():
    a = torch.zeros(2, 3)
    with pytest.raises(ValueError, match="Invalid input euler angles."):
        euler_angles_to_matrix(torch.zeros(2, 4), "XYZ")
    with pytest.raises(ValueError, match="Convention must have 3 letters."):
        euler_angles_to_matrix(a, "XY")
    with pytest.raises(ValueError, match="Invalid convention XXY."):
        euler_angles_to_matrix(a, "XXY")
    with pytest.raises(ValueError, match="Invalid convention ZYY."):
        euler_angles_to_matrix(a, "ZYY")
    with pytest.raises(ValueError, match="Invalid letter W in convention string."):
        euler_angles_to_matrix(a, "XYW")


def test_euler_gradcheck():
    g = torch.Generator().manual_seed(4)
    ang = (torch.rand(3, 3, generator=g, dtype=torch.float64) - 0.5).requires_grad_(True)
    for convention in ("XYZ", "ZXZ"):
        assert torch.autograd.gradcheck(lambda a: euler_angles_to_matrix(a, convention), (ang,))


# --------------------------------------------------------------------------- the Python layer
def _inputs(S=3, P1=5, P2=7, D=3):
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(P1, D, generator=g), torch.randn(P2, D, generator=g)
    R = euler_angles_to_matrix(torch.randn(S, 3, generator=g), "XYZ")
    return x, y, R, torch.randn(S, 3, generator=g), torch.rand(S, generator=g) + 0.5


def test_import_paths_and_all_is_unchanged():
    from torch_renderer_amd import loss, losses

    assert loss.posed_chamfer_distance is losses.posed_chamfer_distance
    assert loss.__all__ == ["mesh_edge_loss", "mesh_laplacian_smoothing", "mesh_normal_consistency",
                            "mesh_shape_priors"]
    for name in ("posed_chamfer", "PosedChamfer"):
        assert hasattr(kernels, name), name


def test_cpu_tensors_are_refused():
    from torch_renderer_amd.loss import posed_chamfer_distance

    x, y, R, T, s = _inputs()
    for call in (lambda: posed_chamfer_distance(x, y, R, T),
                 lambda: posed_chamfer_distance(x[None], y[None], R, T[:, None], s, norm=1),
                 lambda: posed_chamfer_distance(x, y, (R, T, s), point_reduction="sum", single_directional=True),
                 lambda: posed_chamfer_distance(x, y, R.transpose(1, 2), T),
                 lambda: kernels.posed_chamfer(x, y, R, T, s, return_idx=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_argument_errors():
    from torch_renderer_amd.loss import posed_chamfer_distance as pcd

    x, y, R, T, s = _inputs()
    x2, y2, _, _, _ = _inputs(D=2)
    with pytest.raises(NotImplementedError):
        pcd(x2, y, R, T)
    with pytest.raises(NotImplementedError):
        pcd(x, y2, R, T)
    for bad in (lambda: pcd(x[:0], y, R, T), lambda: pcd(x, y[:0], R, T),        # an empty cloud
                lambda: pcd(x, y, R, T, norm=3), lambda: pcd(x, y, R, T, norm=0),
                lambda: pcd(x, y, R, T, point_reduction="max"), lambda: pcd(x, y, R, T, point_reduction=None),
                lambda: pcd(x, y, R, T[:2]), lambda: pcd(x, y, R, T, s[:2]),      # mismatched S
                lambda: pcd(x, y, R[:, :2], T), lambda: pcd(x, y, R[0], T),       # R not (S,3,3)
                lambda: pcd(x, y, R.reshape(-1, 9), T),
                lambda: pcd(torch.stack((x, x)), y, R, T),                        # more than one source cloud
                lambda: pcd(x, y, (R, T)), lambda: pcd(x, y, (R, T, s), T),       # a malformed / doubled triple
                lambda: pcd(x, y, R),                                             # no T
                lambda: kernels.posed_chamfer(x, y, R, T, norm=3)):
        with pytest.raises(ValueError):
            bad()


def test_a_cloud_that_requires_grad_is_refused_only_with_grad_mode_on():
    from torch_renderer_amd.loss import posed_chamfer_distance as pcd

    x, y, R, T, s = _inputs()
    xg = x.clone().requires_grad_(True)
    yg = y.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="requires grad"):
        pcd(xg, y, R, T)
    with pytest.raises(NotImplementedError, match="requires grad"):
        pcd(x, yg, R, T, s)
    with torch.no_grad():  # past that check: the next refusal is the CPU tensor
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pcd(xg, yg, R, T)


# --------------------------------------------------------------------------- the C ABI
def test_abi_rejects_bad_arguments_without_touching_the_gpu(lib):
    """A status and a message before any launch (no GPU here). `p` is host memory that is never dereferenced."""
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    big = 1 << 40

    def call(**k):
        return lib.mr_posed_chamfer(k.get("x", p), k.get("y", p), k.get("P1", 4), k.get("P2", 5), k.get("rts", p),
                                    k.get("S", 3), k.get("norm", 2), k.get("flags", 1), k.get("out", p), p, p,
                                    k.get("pg", p), k.get("ws", p), k.get("wsb", big), None)

    def err():
        return lib.mr_last_error()

    for name in ("x", "y", "rts", "out", "ws"):
        assert call(**{name: None}) == 1 and b"NULL" in err(), name
    assert call(S=0) == 1 and b">= 1" in err()
    assert call(P1=0) == 1 and call(P2=0) == 1 and call(P2=-3) == 1
    assert call(norm=0) == 1 and b"norm" in err()
    assert call(norm=3) == 1
    for flags in (2, 4, 16, 1 | 2):  # the batch reductions are not this entry point's
        assert call(flags=flags) == 1 and b"flags" in err(), flags
    assert call(wsb=8) == 4
    rc = call(S=70000)
    assert rc == 3 and b"65535" in err()
    with pytest.raises(NotImplementedError):
        _lib.check(rc)
    assert call(P1=1 << 31) == 3
    need = lib.mr_posed_chamfer_workspace(1000, 1000, 500)
    assert need >= 8 * 14 * 2 * 1000 * 2  # 14 doubles per (direction, pose, tile), two tiles
    assert call(S=1000, P1=1000, P2=500, wsb=need - 1) == 4
    assert lib.mr_posed_chamfer_workspace(0, 10, 10) == 0 and lib.mr_posed_chamfer_workspace(70000, 10, 10) == 0
    assert lib.mr_posed_chamfer_workspace(1, 0, 10) == 0 and lib.mr_posed_chamfer_workspace(1, 1 << 31, 1) == 0


def test_abi_version_and_symbols(lib):
    assert lib.mr_version() == 5
    for name in ("mr_posed_chamfer", "mr_posed_chamfer_workspace"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


# --------------------------------------------------------------------------- the restatement
X = torch.tensor([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
Y = torch.tensor([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 1.0, 0.0]])
# pose 0: the identity. pose 1: x R = (-x1, x0, x2) (a quarter turn about z for row vectors), s = 2, T = (1, 0, 0)
RS = torch.stack((torch.eye(3), torch.tensor([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])))
TS = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
SS = torch.tensor([1.0, 2.0])


def test_restatement_against_hand_values():
    for dtype in (torch.float32, torch.float64):
        xt = PR.posed_points(X, RS, TS, SS, dtype)
        assert xt.dtype == dtype and xt[0].tolist() == X.tolist()
        assert xt[1].tolist() == [[1.0, 0.0, 0.0], [1.0, 4.0, 0.0], [-1.0, 0.0, 0.0]]
        dx, ix, dy, iy = PR.posed_nearest_ref(X, Y, RS, TS, SS, dtype=dtype)
        # pose 0: x0 ties y0, y1, y2 and x2 ties y0, y1, y2: the first; y0 and y2 tie x0, x1: the first
        assert ix.tolist() == [[0, 0, 0], [0, 3, 1]] and dx.tolist() == [[1.0, 1.0, 2.0], [0.0, 10.0, 0.0]]
        assert iy.tolist() == [[0, 0, 0, 1], [0, 2, 0, 0]] and dy.tolist() == [[1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 2.0]]
        d1 = PR.posed_nearest_ref(X, Y, RS, TS, SS, norm=1, dtype=dtype)
        # L1, pose 1: x'1 = (1, 4, 0) is 4 from y0, y2 and y3 alike: the first
        assert d1[0].tolist() == [[1.0, 1.0, 2.0], [0.0, 4.0, 0.0]] and d1[1].tolist() == [[0, 0, 0], [0, 0, 1]]
        assert d1[2].tolist() == [[1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 2.0]]
        R, T, s = RS.to(dtype), TS.to(dtype), SS.to(dtype)
        tot = PR.posed_chamfer_from_idx(X, Y, R, T, s, ix, iy, point_reduction="sum")
        assert tot.tolist() == [8.0, 12.0]
        mean = PR.posed_chamfer_from_idx(X, Y, R, T, s, ix, iy)
        assert mean.tolist() == pytest.approx([4.0 / 3 + 1.0, 10.0 / 3 + 0.5])
        one = PR.posed_chamfer_from_idx(X, Y, R, T, s, ix, None, point_reduction="sum", single_directional=True)
        assert one.tolist() == [4.0, 10.0]


def test_moment_gradient_against_hand_values_and_autograd():
    _, ix, _, iy = PR.posed_nearest_ref(X, Y, RS, TS, SS)
    # pose 1, norm 2, sums: the pairs with a non-zero g are (x1, y3): g = (-1, 3, 0), x R = (0, 2, 0), and
    # (x0, y3) of direction 1: g = (-1, -1, 0), x R = 0. dT = 2 sum g, ds = 2 sum (x R).g, dR = 2 s sum x^T g
    mom = PR.pose_moments(X, Y, RS, TS, SS, ix, iy)
    assert mom[0, 1, 0:3].tolist() == [-1.0, 3.0, 0.0] and mom[1, 1, 0:3].tolist() == [-1.0, -1.0, 0.0]
    assert mom[0, 1, 12].item() == 6.0 and mom[1, 1, 12].item() == 0.0
    pg = PR.pose_grad_from_moments(mom, SS, 3, 4, point_reduction="sum")
    assert pg[1, 9:12].tolist() == [-4.0, 4.0, 0.0] and pg[1, 12].item() == 12.0
    assert pg[1, 0:9].tolist() == [-8.0, 24.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]  # 2 * 2 * x1^T g, x1 = (2, 0, 0)
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(9, 3, generator=g), torch.randn(11, 3, generator=g)
    R = euler_angles_to_matrix(torch.randn(4, 3, generator=g), "XYZ")
    T, s = 0.3 * torch.randn(4, 3, generator=g), torch.rand(4, generator=g) + 0.5
    for norm in (2, 1):
        _, jx, _, jy = PR.posed_nearest_ref(x, y, R, T, s, norm=norm)
        for pr, single in (("mean", False), ("sum", False), ("mean", True)):
            kw = dict(norm=norm, point_reduction=pr, single_directional=single)
            _, gR, gT, gs = PR.posed_chamfer_ref(x, y, R, T, s, idx=(jx, None if single else jy), **kw)
            mom = PR.pose_moments(x, y, R, T, s, jx, None if single else jy, norm=norm)
            pg = PR.pose_grad_from_moments(mom, s, 9, 11, **kw)
            auto = torch.cat((gR.reshape(4, 9), gT, gs[:, None]), 1)
            assert (pg - auto).abs().max() < 1e-12, (norm, pr, single)
