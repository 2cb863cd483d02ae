"""chamfer_distance, sample_points_from_meshes and the kernels behind them (csrc/mr_points.hip) without a GPU: the
upstream import paths, the argument checks of the Python layer (every ValueError / NotImplementedError, and CPU
tensors refused), the C ABI's checks before any launch, and the restatement of tests/points_ref.py against
hand-computed values."""
import ctypes
import os

import pytest
import torch

from tests import points_ref as R
from torch_renderer_amd import Meshes, _lib, kernels


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from torch_renderer_amd import _build

        _build.build()
    return _lib.load()


def _clouds(N=2, P1=5, P2=7, D=3):
    g = torch.Generator().manual_seed(0)
    return torch.randn(N, P1, D, generator=g), torch.randn(N, P2, D, generator=g)


def _tri_mesh():
    return Meshes([torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])], [torch.tensor([[0, 1, 2]])])


def test_upstream_import_paths():
    from torch_renderer_amd import losses, ops
    from torch_renderer_amd.loss import chamfer_distance
    from torch_renderer_amd.ops import sample_points_from_meshes

    assert chamfer_distance is losses.chamfer_distance
    assert sample_points_from_meshes is ops.sample_points_from_meshes
    for name in ("nearest_points", "face_areas", "ChamferDistance", "SamplePoints"):
        assert hasattr(kernels, name), name


def test_cpu_tensors_are_refused():
    from torch_renderer_amd.loss import chamfer_distance
    from torch_renderer_amd.ops import sample_points_from_meshes

    x, y = _clouds()
    m = _tri_mesh()
    v, f = m.verts_list()[0], m.faces_list()[0]
    for call in (lambda: chamfer_distance(x, y),
                 lambda: chamfer_distance(x, y, x_lengths=torch.tensor([5, 2]), weights=torch.ones(2)),
                 lambda: kernels.nearest_points(x, y),
                 lambda: kernels.face_areas(v, f),
                 lambda: kernels.SamplePoints.apply(v, f, torch.zeros(1, 4, dtype=torch.int64), torch.rand(2, 1, 4)),
                 lambda: sample_points_from_meshes(m, 10)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_chamfer_argument_errors():
    from torch_renderer_amd.loss import chamfer_distance

    x, y = _clouds()
    nrm = torch.zeros_like(x)
    with pytest.raises(NotImplementedError):
        chamfer_distance(x, y, x_normals=nrm)
    with pytest.raises(NotImplementedError):
        chamfer_distance(x, y, y_normals=torch.zeros_like(y))
    with pytest.raises(NotImplementedError):
        chamfer_distance(x, y, point_reduction=None)
    x2, y2 = _clouds(D=2)
    with pytest.raises(NotImplementedError):
        chamfer_distance(x2, y2)
    for norm in (0, 3, 2.5):
        with pytest.raises(ValueError):
            chamfer_distance(x, y, norm=norm)
    with pytest.raises(ValueError):
        chamfer_distance(x, y, batch_reduction="max")
    with pytest.raises(ValueError):
        chamfer_distance(x, y, point_reduction="max")
    with pytest.raises(ValueError):
        chamfer_distance(x, y[:1])
    for w in (torch.ones(3), torch.ones(2, 1)):
        with pytest.raises(ValueError):
            chamfer_distance(x, y, weights=w)
    for kw in ({"x_lengths": torch.tensor([5, 6])}, {"x_lengths": torch.tensor([-1, 5])},
               {"y_lengths": torch.tensor([7, 8])}, {"y_lengths": torch.tensor([7])},
               {"x_lengths": torch.tensor([[5, 5]])}):
        with pytest.raises(ValueError):
            chamfer_distance(x, y, **kw)
    with pytest.raises(ValueError):
        kernels.nearest_points(x, y, norm=3)
    with pytest.raises(NotImplementedError):
        kernels.nearest_points(x2, y2)


def test_sample_points_argument_errors():
    from torch_renderer_amd.ops import sample_points_from_meshes

    m = _tri_mesh()
    with pytest.raises(NotImplementedError):
        sample_points_from_meshes(m, 10, return_normals=True)
    with pytest.raises(NotImplementedError):
        sample_points_from_meshes(m, 10, return_textures=True)
    empty = Meshes([torch.zeros(3, 3)], [torch.zeros(0, 3, dtype=torch.int64)])
    with pytest.raises(ValueError, match="Meshes are empty."):
        sample_points_from_meshes(empty, 10)
    bad = Meshes([torch.zeros(3, 3)], [torch.tensor([[0, 1, 3]])])
    with pytest.raises(ValueError, match="outside the mesh"):
        sample_points_from_meshes(bad, 10)


def test_abi_rejects_bad_arguments_without_touching_the_gpu(lib):
    """NULL pointers and bad sizes: a status and a message before any memset or launch (no GPU here). `p` is host
    memory that is never dereferenced."""
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    big = 1 << 40

    def err():
        return lib.mr_last_error()

    # nearest points
    assert lib.mr_nearest_points(None, p, 1, 4, 4, None, None, 2, p, p, p, p, p, big, None) == 1 and b"NULL" in err()
    assert lib.mr_nearest_points(p, p, 1, 4, 4, None, None, 2, p, None, p, p, p, big, None) == 1 and b"NULL" in err()
    assert lib.mr_nearest_points(p, p, 0, 4, 4, None, None, 2, p, p, p, p, p, big, None) == 1 and b">= 1" in err()
    assert lib.mr_nearest_points(p, p, 1, 0, 4, None, None, 2, p, p, p, p, p, big, None) == 1
    assert lib.mr_nearest_points(p, p, 1, 4, 4, None, None, 3, p, p, p, p, p, big, None) == 1 and b"norm" in err()
    assert lib.mr_nearest_points(p, p, 1, 4, 4, None, None, 2, p, p, p, p, p, 0, None) == 4  # MR_EWORKSPACE
    rc = lib.mr_nearest_points(p, p, 70000, 4, 4, None, None, 2, p, p, p, p, p, big, None)
    assert rc == 3 and b"65535" in err()
    with pytest.raises(NotImplementedError):
        _lib.check(rc)
    rc = lib.mr_nearest_points(p, p, 1, 2 * 10 ** 9, 2 * 10 ** 9, None, None, 2, p, p, p, p, p, big, None)
    assert rc == 3 and b"too large for one launch" in err()  # more workgroups than a grid holds
    assert lib.mr_nearest_points_workspace(1, 1000, 1000) >= 2 * 8 * 1000
    assert lib.mr_nearest_points_workspace(0, 10, 10) == 0 and lib.mr_nearest_points_workspace(1, 1 << 31, 1) == 0
    # chamfer
    def fwd(**k):
        return lib.mr_chamfer_forward(k.get("x", p), p, k.get("N", 2), 4, k.get("P2", 4), None, None, None,
                                      k.get("norm", 2), k.get("flags", 3), p, p, p, k.get("out", p), p,
                                      k.get("ws", big), None)

    def bwd(**k):
        return lib.mr_chamfer_backward(p, p, k.get("N", 2), 4, 4, k.get("norm", 2), k.get("flags", 3),
                                       k.get("idx_x", p), k.get("idx_y", p), k.get("coef", p), k.get("g", p),
                                       k.get("gx", p), p, p, k.get("ws", big), None)

    assert fwd(x=None) == 1 and b"NULL" in err()
    assert fwd(out=None) == 1 and b"out" in err()
    assert fwd(N=0) == 1 and fwd(P2=0) == 1 and fwd(P2=-1) == 1
    assert fwd(norm=0) == 1 and b"norm" in err()
    assert fwd(flags=16) == 1 and b"flags" in err()
    assert fwd(flags=6) == 1 and b"flags" in err()  # batch mean and batch sum together
    assert fwd(ws=16) == 4
    assert lib.mr_chamfer_workspace(2, 1000, 500) > 0 and lib.mr_chamfer_workspace(2, 0, 500) == 0
    for k in ("idx_x", "idx_y", "coef", "g", "gx"):
        assert bwd(**{k: None}) == 1 and b"NULL" in err(), k
    assert bwd(N=0) == 1 and bwd(norm=5) == 1 and bwd(flags=32) == 1 and bwd(ws=8) == 4
    assert lib.mr_chamfer_backward_workspace(1, 10, 20) >= 12 * 3 * 30
    # sampling and areas
    assert lib.mr_sample_points_forward(p, 3, p, 1, None, p, 8, p, None) == 1 and b"NULL" in err()
    assert lib.mr_sample_points_forward(p, 3, None, 1, p, p, 8, p, None) == 1
    assert lib.mr_sample_points_forward(p, -1, p, 1, p, p, 8, p, None) == 1 and b"out of range" in err()
    assert lib.mr_sample_points_forward(p, 3, p, 1, p, p, -8, p, None) == 1
    assert lib.mr_sample_points_forward(p, 3, p, 1, p, p, 0, p, None) == 0  # nothing to do
    assert lib.mr_sample_points_backward(3, p, 1, p, p, 8, None, p, p, big, None) == 1 and b"NULL" in err()
    assert lib.mr_sample_points_backward(3, p, 1, p, p, 8, p, p, None, big, None) == 1
    assert lib.mr_sample_points_backward(3, p, 1, p, p, 8, p, p, p, 4, None) == 4
    assert lib.mr_sample_points_backward(1 << 31, p, 1, p, p, 8, p, p, p, big, None) == 1
    assert lib.mr_sample_points_backward_workspace(100) >= 12 * 300
    assert lib.mr_face_areas(None, 3, p, 1, p, None) == 1 and b"NULL" in err()
    assert lib.mr_face_areas(p, 3, p, -1, p, None) == 1 and b"out of range" in err()
    assert lib.mr_face_areas(p, 3, p, 0, p, None) == 0


def test_abi_version_and_structs_are_unchanged(lib):
    assert lib.mr_version() == 5 and lib.mr_struct_size(9) == -1
    for name in ("mr_nearest_points", "mr_chamfer_forward", "mr_chamfer_backward", "mr_sample_points_forward",
                 "mr_sample_points_backward", "mr_face_areas"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_restatement_against_hand_values():
    """The yardstick itself: ties take the first index, lengths mask, upstream's reductions."""
    x = torch.tensor([[[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [9.0, 9.0, 9.0]]])
    y = torch.tensor([[[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 1.0, 0.0]]])
    dx, ix, dy, iy = R.nearest_ref(x, y, torch.tensor([2]), None)
    assert ix.tolist() == [[0, 0, -1]] and dx.tolist() == [[1.0, 1.0, 0.0]]  # x0 ties y0, y1, y2: the first
    assert iy.tolist() == [[0, 0, 0, 1]] and dy.tolist() == [[1.0, 1.0, 1.0, 1.0]]  # y0 ties x0, x1
    d1 = R.nearest_ref(x, y, torch.tensor([2]), None, norm=1)
    assert d1[0].tolist() == [[1.0, 1.0, 0.0]] and d1[2].tolist() == [[1.0, 1.0, 1.0, 1.0]]
    kw = dict(x_lengths=torch.tensor([2]))
    mean, _, _ = R.chamfer_ref(x, y, **kw)
    assert mean.item() == pytest.approx(2.0 / 2 + 4.0 / 4)
    tot, gx, gy = R.chamfer_ref(x, y, point_reduction="sum", batch_reduction=None, **kw)
    assert tot.tolist() == [6.0] and gx[0, 2].abs().max() == 0  # the padded point takes no gradient
    # y0 = (1,0,0): own term 2 (y0 - x0) = (2,0,0), plus x0's and x1's terms 2 (y0 - x0) + 2 (y0 - x1) = (0,0,0)
    assert gy[0, 0].tolist() == [2.0, 0.0, 0.0]
    one, _, _ = R.chamfer_ref(x, y, single_directional=True, weights=torch.tensor([3.0]), **kw)
    assert one.item() == pytest.approx(3.0 * 1.0 / 3.0)
    empty = R.nearest_ref(x, y, torch.tensor([0]), None)
    assert empty[1].max() == -1 and empty[3].max() == -1 and empty[2].abs().max() == 0
    v = torch.tensor([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.0]], dtype=torch.float64)
    f = torch.tensor([[0, 1, 2]])
    assert R.face_areas_ref(v, f).tolist() == [2.0]
    p = R.sample_ref(v, f, torch.tensor([[0, 0, -1]]), torch.tensor([[[0.0, 0.25, 0.5]], [[0.3, 0.5, 0.5]]],
                                                                    dtype=torch.float64))
    assert p[0, 0].tolist() == [0.0, 0.0, 0.0] and p[0, 2].tolist() == [0.0, 0.0, 0.0]
    assert torch.allclose(p[0, 1], torch.tensor([0.5, 0.5, 0.0], dtype=torch.float64))  # s = .5: w = .5, .25, .25
