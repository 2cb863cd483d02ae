"""estimate_pointcloud_normals / estimate_pointcloud_local_coord_frames (csrc/mr_normals.hip) without a GPU: the names
and the exported symbols, the Python layer's errors, the C ABI's checks before any launch, the launch geometry of the
shapes test_gpu_normals.py relies on, the eigen solver run on the host (mr_symmetric_eig3_host, the same code the
kernels run) against numpy.linalg.eigh, and the float64 reference itself on a sphere."""
import os

import numpy as np
import pytest
import torch

from tests import normals_ref as NR
from torch_renderer_amd import _lib, kernels, ops
from torch_renderer_amd.structures import Pointclouds


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from torch_renderer_amd import _build

        _build.build()
    return _lib.load()


def test_upstream_import_paths():
    from torch_renderer_amd.ops import estimate_pointcloud_local_coord_frames, estimate_pointcloud_normals

    assert estimate_pointcloud_normals is ops.estimate_pointcloud_normals
    assert estimate_pointcloud_local_coord_frames is ops.estimate_pointcloud_local_coord_frames
    for name in ("point_frames", "frames_geometry", "symmetric_eig3_host"):
        assert hasattr(kernels, name), name
    assert (kernels.FRAMES_MIN_K, kernels.FRAMES_MAX_K) == (2, 64) and kernels.KNN_MAX_K == 32


def test_symbols_are_exported_with_argtypes(lib):
    for name, nargs in (("mr_point_frames", 12), ("mr_point_frames_workspace", 3), ("mr_point_frames_geometry", 7),
                        ("mr_symmetric_eig3_host", 4)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert _lib.MR_FRAMES_DISAMBIGUATE == 1


def test_python_errors_come_before_any_device_use():
    g = torch.Generator().manual_seed(0)
    p = torch.randn(2, 70, 3, generator=g)
    for fn in (ops.estimate_pointcloud_normals, ops.estimate_pointcloud_local_coord_frames):
        with pytest.raises(ValueError):
            fn(p[:, :40], neighborhood_size=40)  # L <= K
        with pytest.raises(ValueError):
            fn(p[:, :50])  # the default 50 on clouds of 50
        with pytest.raises(ValueError):
            fn(p[..., :2], neighborhood_size=8)  # D != 3
        with pytest.raises(ValueError):
            fn(p[0], neighborhood_size=8)  # not (N, P, 3)
        with pytest.raises(ValueError):
            fn(p, neighborhood_size=1)
        with pytest.raises(ValueError):
            fn([p], neighborhood_size=8)  # neither a tensor nor a Pointclouds
        with pytest.raises(ValueError):
            fn(Pointclouds([p[0], p[1, :8]]), neighborhood_size=8)  # one cloud of the batch has L <= K
        with pytest.raises(NotImplementedError):
            fn(torch.randn(1, 100, 3, generator=g), neighborhood_size=65)
        with pytest.raises(NotImplementedError, match="not differentiable"):
            fn(p.clone().requires_grad_(True), neighborhood_size=8)
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(p.clone().requires_grad_(True), neighborhood_size=8)  # grad mode off: refused only for the device
        for call in (lambda: fn(p, neighborhood_size=8), lambda: fn(p, 8, False, use_symeig_workaround=False),
                     lambda: fn(Pointclouds([p[0], p[1, :40]]), neighborhood_size=8)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
    with pytest.raises(ValueError):
        kernels.point_frames(p[:, :40], K=40)
    with pytest.raises(ValueError):
        kernels.point_frames(p, K=1)
    with pytest.raises(ValueError):
        kernels.point_frames(p[..., :2], K=8)
    with pytest.raises(ValueError):
        kernels.point_frames(p, lengths=torch.tensor([70]), K=8)
    with pytest.raises(NotImplementedError):
        kernels.point_frames(torch.randn(1, 100, 3, generator=g), K=65)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.point_frames(p, K=8, return_cov=True)


def test_abi_rejects_bad_arguments_without_touching_the_gpu(lib):
    one = 1  # any non-NULL pointer value: the checks below return before anything is read
    f = lib.mr_point_frames
    big = 1 << 30
    assert f(None, 1, 100, None, 8, 1, one, one, None, one, big, None) == 1 and b"NULL" in lib.mr_last_error()
    assert f(one, 1, 100, None, 8, 1, None, one, None, one, big, None) == 1
    assert f(one, 1, 100, None, 8, 1, one, None, None, one, big, None) == 1
    assert f(one, 1, 100, None, 8, 1, one, one, None, None, big, None) == 1
    assert f(one, 0, 100, None, 8, 1, one, one, None, one, big, None) == 1
    assert f(one, 1, 0, None, 8, 1, one, one, None, one, big, None) == 1
    assert f(one, 70000, 100, None, 8, 1, one, one, None, one, big, None) == 3
    assert f(one, 1, 100, None, 1, 1, one, one, None, one, big, None) == 1 and b"K" in lib.mr_last_error()
    rc = f(one, 1, 100, None, 65, 1, one, one, None, one, big, None)
    assert rc == 3 and b"K" in lib.mr_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc)
    assert f(one, 1, 50, None, 50, 1, one, one, None, one, big, None) == 1 and b"more than K" in lib.mr_last_error()
    assert f(one, 1, 100, None, 8, 2, one, one, None, one, big, None) == 1 and b"flags" in lib.mr_last_error()
    assert f(one, 1, 100, None, 8, 1, one, one, None, one, 8, None) == 4 and b"workspace" in lib.mr_last_error()
    assert lib.mr_point_frames_workspace(1, 100, 1) == 0 and lib.mr_point_frames_workspace(1, 100, 65) == 0
    assert lib.mr_point_frames_workspace(1, 50, 50) == 0 and lib.mr_point_frames_workspace(70000, 100, 8) == 0
    for N, P, K in ((1, 300, 16), (256, 70, 50), (1, 20000, 50)):
        ws = lib.mr_point_frames_workspace(N, P, K)
        assert 0 < ws <= N * P * 8 * K * 16 + 512, (N, P, K, ws)
    g = lib.mr_point_frames_geometry
    assert g(1, 100, 65, None, None, None, None) == 3 and g(1, 100, 1, None, None, None, None) == 1
    assert g(1, 50, 50, None, None, None, None) == 1 and g(1, 100, 50, None, None, None, None) == 0
    e = lib.mr_symmetric_eig3_host
    assert e(None, 1, one, one) == 1 and e(one, -1, one, one) == 1 and e(None, 0, None, None) == 0


def test_geometry_of_the_gpu_cases(lib):
    assert [kernels.frames_geometry(1, 5000, K)[0] for K in (2, 9, 32, 50)] == [8, 16, 32, 64]
    assert [kernels.frames_geometry(1, 5000, K)[1] for K in (8, 16, 32, 33, 64)] == [512, 256, 128, 128, 128]
    for K in (5, 16, 32, 33, 50):
        bucket, _, splits, chunk = kernels.frames_geometry(1, 300, K)
        assert 1 < splits <= 16 and chunk < 1024, (K, splits, chunk)
        assert kernels.frames_geometry(256, 70, K)[2] == 1, K  # N * query tiles >= 256: one launch
        assert kernels.frames_geometry(2, 733, K)[2] > 1, K
    # one cloud of 1,100 points is split into ranges shorter than the 1,024-target LDS chunk; as a member of a batch
    # of 256 it is scanned whole, across the chunk boundary (test_gpu_normals.py runs it both ways)
    assert kernels.frames_geometry(1, 1100, 16)[2] > 1 and kernels.frames_geometry(1, 1100, 16)[3] < 1024
    assert kernels.frames_geometry(256, 1100, 16)[2:] == (1, 1024)
    # the scan's geometry is knn_points' wherever both exist
    for N, P, K in ((1, 300, 16), (3, 5000, 32), (300, 2000, 8)):
        assert kernels.frames_geometry(N, P, K)[1:] == kernels.knn_geometry(N, P, P, K)


def _covariances():
    """(M,6) float32: random SPD, rank 2, rank 1 and zero, each at scales 1e-6, 1 and 1e6."""
    g = torch.Generator().manual_seed(7)
    sets = []
    for rank in (3, 2, 1, 0):
        a = torch.randn(400, 3, 3, generator=g, dtype=torch.float64)
        a[:, :, rank:] = 0.0
        # some nearly isotropic and some strongly anisotropic members
        a[:100] = a[:100] * torch.tensor([1.0, 1e-2, 1e-4], dtype=torch.float64)
        q, _ = torch.linalg.qr(torch.randn(400, 3, 3, generator=g, dtype=torch.float64))
        a = q @ a
        sets.append(a @ a.transpose(1, 2))
    c = torch.cat(sets)
    c = torch.cat([c * s for s in (1e-6, 1.0, 1e6)])
    return torch.from_numpy(NR.cov6(c.numpy())).float()


def test_host_eigen_solver_against_numpy(lib):
    c6 = _covariances()
    assert c6.shape[0] == 4800
    lam, vec = kernels.symmetric_eig3_host(c6)
    lam, vec = lam.double().numpy(), vec.double().numpy()
    assert np.isfinite(lam).all() and np.isfinite(vec).all()
    C = NR.cov33(c6.numpy())
    w = np.linalg.eigvalsh(C)
    tr = np.trace(C, axis1=1, axis2=2)
    assert (tr >= 0).all()
    err = np.abs(lam - w).max(1)
    res = np.linalg.norm(C @ vec - vec * lam[:, None, :], axis=1).max(1)
    orth = np.abs(np.swapaxes(vec, 1, 2) @ vec - np.eye(3)).reshape(-1, 9).max(1)
    nz = tr > 0
    print(f"[normals] host solver over {len(tr)} covariances: max eigenvalue error / trace "
          f"{(err[nz] / tr[nz]).max():.2e}, max residual / trace {(res[nz] / tr[nz]).max():.2e}, "
          f"max |V^T V - I| {orth.max():.2e}")
    assert (err <= 1e-4 * tr).all() and (res <= 1e-4 * tr).all() and (orth <= 1e-5).all()
    assert (np.diff(lam, axis=1) >= 0).all()  # ascending
    zero = ~nz
    assert zero.sum() == 1200 and (lam[zero] == 0).all() and (vec[zero] == np.eye(3)).all()
    # every column's component of largest magnitude is positive
    assert (np.take_along_axis(vec, np.argmax(np.abs(vec), axis=1)[:, None, :], axis=1) > 0).all()
    # scale-free: a power-of-two multiple of a matrix has the same eigenvectors bit for bit, eigenvalues times it
    lam2, vec2 = kernels.symmetric_eig3_host(c6 * 1024.0)
    assert np.array_equal(vec2.numpy(), vec.astype(np.float32)) and np.array_equal(lam2.numpy(), (lam * 1024).astype(np.float32))


def test_reference_on_a_sphere():
    """The reference itself: on a noise-free unit sphere all neighbours lie on the inner side of the tangent plane, so
    every disambiguated normal points inwards."""
    p = NR.sphere(300)
    r = NR.frames_ref(p[None], K=16)
    n = r["frames"][0, :, :, 0]
    inward = -(n * p.double().numpy()).sum(1) / np.linalg.norm(p.double().numpy(), axis=1)
    print(f"[normals] reference, sphere 300, K = 16: min n . (-p) = {inward.min():.3f}")
    assert (inward >= 0.9).all()
    f = r["frames"][0]
    assert np.abs(np.swapaxes(f, 1, 2) @ f - np.eye(3)).max() < 1e-12
    assert np.abs(np.cross(f[:, :, 0], f[:, :, 2]) - f[:, :, 1]).max() == 0
    assert (np.diff(r["cur"][0], axis=1) >= 0).all() and r["valid"].all()
    assert (r["idx"][0, :, 0] == np.arange(300)).all()  # the point itself is its nearest neighbour
    # without the disambiguation: the largest component of every column is positive; the same axes
    u = NR.frames_ref(p[None], K=16, disambiguate=False)["frames"][0]
    assert (np.take_along_axis(u, np.argmax(np.abs(u), axis=1)[:, None, :], axis=1) > 0).all()
    assert np.abs(np.abs((u * f).sum(1)) - 1).max() < 1e-9
    # padded rows and a cloud shorter than K are zeros
    pts, lengths = NR.cow_clouds()
    assert pts.shape == (2, 733, 3) and lengths.tolist() == [733, 257]
    c = NR.frames_ref(pts, lengths, K=50)
    assert c["valid"][1, :257].all() and not c["valid"][1, 257:].any() and (c["frames"][1, 257:] == 0).all()
