"""knn_points / knn_gather (csrc/mr_knn.hip) without a GPU: the preconditions of the GPU cases (the ties case really
has ties at the K-th / (K+1)-th boundary, the named shapes really exercise each launch regime), the workspace sizes,
the Python layer's errors, the C ABI's checks before any launch, and knn_gather against an explicit loop."""
import os

import pytest
import torch

from tests import knn_ref as KR
from tests.points_ref import pair_dist
from torch_renderer_amd import _lib, kernels, ops


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from torch_renderer_amd import _build

        _build.build()
    return _lib.load()


def test_upstream_import_paths():
    from torch_renderer_amd.ops import knn_gather, knn_points

    assert knn_points is ops.knn_points and knn_gather is ops.knn_gather
    for name in ("knn_points", "knn_geometry", "KnnPoints"):
        assert hasattr(kernels, name), name


def test_ties_case_has_ties_at_the_boundary():
    """For each K of the ties case: the queries whose K-th and (K+1)-th reference distances are equal. There must be
    some, and there the reference keeps the lowest indices among the boundary distance."""
    p1, p2, _, _ = KR.case("ties")
    counts = {}
    for norm in (1, 2):
        d = pair_dist(p1[0], p2[0], norm)
        v, _ = KR.sorted_dists(p1[0], p2[0], norm)
        for K in KR.CASES["ties"]:
            tied = v[:, K - 1] == v[:, K]
            counts[(norm, K)] = int(tied.sum())
            _, idx = KR.knn_ref(p1, p2, K=K, norm=norm)
            for q in tied.nonzero()[:, 0].tolist():
                edge = v[q, K - 1]
                kept = idx[0, q][(d[q][idx[0, q].long()] == edge)].tolist()
                lowest = (d[q] == edge).nonzero()[:, 0][:len(kept)].tolist()
                assert kept == lowest, (norm, K, q)
    print(f"[knn] queries tied at the K-th boundary, (norm, K): {counts}")
    assert any(c > 0 for c in counts.values())
    for norm in (1, 2):
        assert any(counts[(norm, K)] > 0 for K in KR.CASES["ties"])


def test_named_cases_cover_the_launch_regimes(lib):
    def geom(name, K):
        p1, p2, _, _ = KR.case(name)
        return kernels.knn_geometry(p1.shape[0], p1.shape[1], p2.shape[1], K)

    # splits == 1, one LDS chunk
    for name, K in (("1x1", 1), ("1x3", 8), ("dup", 8)):
        qpg, splits, chunk = geom(name, K)
        assert splits == 1 and KR.case(name)[1].shape[1] <= chunk <= 1024, (name, qpg, splits, chunk)
    # 256 clouds are never split: the buckets 2, 16 and 32 on the path where the scan writes dists / idx itself
    for K in KR.CASES["256x1x40"]:
        qpg, splits, chunk = geom("256x1x40", K)
        assert splits == 1 and chunk == 40, (K, qpg, splits, chunk)
    # splits == 1, several LDS chunks and a partial last one
    qpg, splits, chunk = geom("600x1x1100", 4)
    assert splits == 1 and chunk == 1024 and 1100 % chunk != 0 and 1100 > chunk
    # splits > 1 with a partial last split
    for name, K, P2 in (("1x1000x1000", 16, 1000), ("63x65", 8, 65), ("het", 8, 1000)):
        qpg, splits, chunk = geom(name, K)
        assert 1 < splits <= 16 and chunk < 1024, (name, splits, chunk)  # below 1024 the chunk is the whole split
        assert (splits - 1) * chunk < P2 < splits * chunk, (name, splits, chunk)
    # splits > 1 and longer than one chunk: several chunks inside a split. A split is a multiple of 64 targets and
    # 20,000 is not a multiple of 64, so the last split is shorter than the others.
    _, splits, chunk = geom("8x100x20000", 8)
    assert 1 < splits <= 16 and chunk == 1024 and -(-20000 // splits) > chunk and 20000 % 64 != 0
    # the bucket of K sets the query tile
    assert [kernels.knn_geometry(1, 5000, 5000, K)[0] for K in (1, 8, 9, 16, 17, 32)] == [512, 512, 256, 256, 128, 128]
    # many clouds or many query tiles: never split
    assert kernels.knn_geometry(300, 2000, 400, 4)[1] == 1 and kernels.knn_geometry(1, 200000, 20000, 8)[1] == 1


def test_workspace_sizes(lib):
    for N, P1, P2, K in ((1, 1, 1, 1), (1, 1000, 1000, 16), (8, 100, 20000, 8), (600, 1, 1100, 4), (1, 63, 65, 32)):
        ws = lib.mr_knn_points_workspace(N, P1, P2, K)
        assert 0 < ws <= P1 * N * (8 * K * 16) + 512, (N, P1, P2, K, ws)
        assert lib.mr_knn_points_backward_workspace(N, P1, P2, K) >= 3 * N * P2 * 12
    assert lib.mr_knn_points_workspace(1, 10, 10, 0) == 0 and lib.mr_knn_points_workspace(1, 10, 10, 33) == 0
    assert lib.mr_knn_points_workspace(70000, 10, 10, 1) == 0


def test_abi_rejects_bad_arguments_without_touching_the_gpu(lib):
    one = 1  # any non-NULL pointer value: the checks below return before anything is read
    f = lib.mr_knn_points
    assert f(None, one, 1, 4, 4, None, None, 2, 1, one, one, one, 256, None) == 1 and b"NULL" in lib.mr_last_error()
    assert f(one, one, 1, 4, 4, None, None, 2, 0, one, one, one, 256, None) == 1 and b"K" in lib.mr_last_error()
    rc = f(one, one, 1, 4, 4, None, None, 2, 33, one, one, one, 256, None)
    assert rc == 3 and b"K" in lib.mr_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc)
    assert f(one, one, 1, 4, 4, None, None, 3, 1, one, one, one, 256, None) == 1 and b"norm" in lib.mr_last_error()
    assert f(one, one, 0, 4, 4, None, None, 2, 1, one, one, one, 256, None) == 1
    assert f(one, one, 70000, 4, 4, None, None, 2, 1, one, one, one, 256, None) == 3
    assert f(one, one, 1, 4, 4, None, None, 2, 1, None, one, one, 256, None) == 1
    assert f(one, one, 1, 4, 4, None, None, 2, 1, one, one, one, 8, None) == 4 and b"workspace" in lib.mr_last_error()
    b = lib.mr_knn_points_backward
    assert b(one, one, 1, 4, 4, None, None, 2, 33, one, one, one, one, one, 1 << 20, None) == 3
    assert b(one, one, 1, 4, 4, None, None, 5, 1, one, one, one, one, one, 1 << 20, None) == 1
    assert b(one, one, 1, 4, 4, None, None, 2, 1, None, one, one, one, one, 1 << 20, None) == 1
    assert b(one, one, 1, 4, 4, None, None, 2, 1, one, one, one, one, one, 8, None) == 4
    assert lib.mr_knn_geometry(1, 4, 4, 33, None, None, None) == 3 and lib.mr_knn_geometry(1, 4, 4, 0, None, None, None) == 1
    assert lib.mr_knn_geometry(1, 4, 4, 4, None, None, None) == 0


def test_python_errors_come_before_any_device_use():
    g = torch.Generator().manual_seed(0)
    p1, p2 = torch.randn(2, 5, 3, generator=g), torch.randn(2, 7, 3, generator=g)
    with pytest.raises(ValueError):
        ops.knn_points(p1, p2[:1])  # batch
    with pytest.raises(ValueError):
        ops.knn_points(p1, p2[..., :2])  # D differs
    with pytest.raises(ValueError):
        ops.knn_points(p1[0], p2[0])  # not (N, P, D)
    with pytest.raises(ValueError):
        ops.knn_points(p1, p2, norm=3)
    with pytest.raises(ValueError):
        ops.knn_points(p1, p2, lengths1=torch.tensor([5]))
    with pytest.raises(ValueError):
        ops.knn_points(p1, p2, lengths2=torch.tensor([[7, 7]]))
    with pytest.raises(ValueError):
        ops.knn_points(p1, p2, K=0)
    with pytest.raises(NotImplementedError):
        ops.knn_points(p1, p2, K=33)
    with pytest.raises(NotImplementedError):
        ops.knn_points(p1[..., :2], p2[..., :2])  # D = 2
    with pytest.raises(NotImplementedError):
        kernels.knn_points(p1, p2, K=33)
    with pytest.raises(ValueError):
        kernels.knn_points(p1, p2, K=0)
    for call in (lambda: ops.knn_points(p1, p2, K=2), lambda: kernels.knn_points(p1, p2, K=2),
                 lambda: ops.knn_points(p1, p2, K=2, version=3, return_nn=True, return_sorted=False)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError):
        ops.knn_gather(p2, torch.zeros(3, 5, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.knn_gather(p2, torch.zeros(2, 5, 2, dtype=torch.int64), torch.tensor([7]))


def test_knn_gather_against_a_loop():
    g = torch.Generator().manual_seed(1)
    N, M, U, L, K = 3, 6, 5, 4, 4
    x = torch.randn(N, M, U, generator=g, dtype=torch.float64, requires_grad=True)
    idx = torch.randint(0, M, (N, L, K), generator=g)
    for lengths in (None, torch.tensor([6, 2, 0])):
        want = torch.zeros(N, L, K, U, dtype=x.dtype)
        for n in range(N):
            for l in range(L):
                for k in range(K):
                    if lengths is None or k < int(lengths[n]):
                        want[n, l, k] = x[n, idx[n, l, k]].detach()
        got = ops.knn_gather(x, idx, lengths)
        assert got.shape == (N, L, K, U) and torch.equal(got.detach(), want)
        w = torch.randn(N, L, K, U, generator=g, dtype=x.dtype)
        gx, = torch.autograd.grad((got * w).sum(), x)
        ref = torch.zeros_like(gx)
        for n in range(N):
            for l in range(L):
                for k in range(K):
                    if lengths is None or k < int(lengths[n]):
                        ref[n, idx[n, l, k]] += w[n, l, k]
        assert torch.allclose(gx, ref, rtol=0, atol=1e-12)
    # K > M without lengths: the slots past M are zero
    few = ops.knn_gather(x[:, :2], torch.zeros(N, L, K, dtype=torch.int64))
    assert torch.equal(few[:, :, 2:], torch.zeros(N, L, 2, U, dtype=x.dtype)) and torch.equal(few[:, 0, 0], x[:, 0])
