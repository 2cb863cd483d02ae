"""ball_query / masked_gather (csrc/mr_ballquery.hip) without a GPU: the restatement against a plain double loop, the
preconditions of the GPU cases (the radii really give the hit counts the cases claim, the named shapes really reach
each launch regime), the Python layer's errors, the C ABI's checks before any launch, and masked_gather against an
explicit loop."""
import math
import os

import pytest
import torch

from tests import ball_query_ref as BR
from torch_renderer_amd import _lib, kernels, ops


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from torch_renderer_amd import _build

        _build.build()
    return _lib.load()


def test_upstream_import_paths():
    from torch_renderer_amd.ops import ball_query, masked_gather

    assert ball_query is ops.ball_query and masked_gather is ops.masked_gather
    for name in ("ball_query", "ball_query_geometry", "BallQuery"):
        assert hasattr(kernels, name), name
    import inspect

    sig = inspect.signature(ball_query)
    assert list(sig.parameters) == ["p1", "p2", "lengths1", "lengths2", "K", "radius", "return_nn"]
    assert sig.parameters["K"].default == 500 and sig.parameters["radius"].default == 0.2
    assert sig.parameters["return_nn"].default is True


def _loop_ref(p1, p2, l1, l2, K, radius):
    """The rule as a double loop over Python floats rounded to float32 after every operation."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    r = f(float(radius))
    r2 = r * r
    N, P1, _ = p1.shape
    dists = torch.zeros(N, P1, K)
    idx = torch.full((N, P1, K), -1, dtype=torch.int32)
    for n in range(N):
        for i in range(l1[n]):
            c = 0
            for j in range(l2[n]):
                dx, dy, dz = (p1[n, i, a] - p2[n, j, a] for a in range(3))
                d = (dx * dx + dy * dy) + dz * dz
                if d < r2 and c < K:
                    dists[n, i, c], idx[n, i, c] = d, j
                    c += 1
    return dists, idx


def test_restatement_against_a_double_loop():
    g = torch.Generator().manual_seed(3)
    p1, p2 = torch.randn(3, 6, 3, generator=g), torch.randn(3, 9, 3, generator=g)
    p2[0, 4, 1] = float("nan")  # never hits
    l1, l2 = [6, 2, 0], [9, 5, 9]
    for K, radius in ((1, 1.0), (3, 1.5), (12, 2.0), (4, 0.0)):
        rd, ri = BR.ball_query_ref(p1, p2, torch.tensor(l1), torch.tensor(l2), K, radius)
        ld, li = _loop_ref(p1, p2, l1, l2, K, radius)
        assert torch.equal(ri, li), (K, radius)
        assert torch.equal(rd.view(torch.int32), ld.view(torch.int32)), (K, radius)
        assert not (ri[0] == 4).any()
        if radius == 0.0:
            assert (ri == -1).all() and (rd == 0).all()
    rd, ri = BR.ball_query_ref(p1, p2, None, None, 12, 2.0)
    assert (ri[..., 9:] == -1).all() and (ri >= 0).any()
    # unsorted by distance, ascending by index
    filled = ri[1, 0][ri[1, 0] >= 0]
    assert torch.equal(filled, filled.sort().values)


def test_cases_have_the_hit_counts_they_claim():
    # strictness: only the second target of "strict" hits; the float32 and float64 squares of 0.7 disagree on the
    # first target of "round0.7" (d == r2 in float32: no hit; d < 0.7 ** 2 in float64: a hit)
    radius, _ = BR.CASES["strict"]
    assert BR.ball_query_ref(*BR.case("strict"), K=2, radius=radius)[1].tolist() == [[[1, -1]]]
    for name in ("round0.7", "round0.1"):
        radius, _ = BR.CASES[name]
        p1, p2, _, _ = BR.case(name)
        d, i = BR.ball_query_ref(p1, p2, K=2, radius=radius)
        assert i.tolist() == [[[1, -1]]], name
        d0 = float(p2[0, 0, 0]) ** 2  # exact in float64
        assert torch.tensor(d0, dtype=torch.float32).double().item() == float(BR.radius2(radius)), name
    p2 = BR.case("round0.7")[1]
    assert float(BR.radius2(0.7)) < 0.7 ** 2 and float(p2[0, 0, 0]) ** 2 < 0.7 ** 2
    # first-K: every query has all 600 targets in reach
    radius, _ = BR.CASES["first"]
    assert all((c == 600).all() for c in BR.hit_counts(*BR.case("first"), radius))
    # wave: the first 64 queries reach exactly targets 0..7, the others exactly target 1024
    radius, _ = BR.CASES["wave"]
    p1, p2, _, _ = BR.case("wave")
    _, idx = BR.ball_query_ref(p1, p2, K=16, radius=radius)
    assert p1.shape[1] == 128 and p2.shape[1] == 1025
    assert (idx[0, :64, :8] == torch.arange(8, dtype=torch.int32)).all() and (idx[0, :64, 8:] == -1).all()
    assert (idx[0, 64:, 0] == 1024).all() and (idx[0, 64:, 1:] == -1).all()
    # chunk and tile boundaries: counts from 0 to above the largest K (63x65: above 7; its K = 64 never fills)
    for name, top in (("63x65", 7), ("513x2049", 64)):
        radius, Ks = BR.CASES[name]
        c = BR.hit_counts(*BR.case(name), radius)[0]
        assert c.min() == 0 and c.max() > top and max(Ks) == 64, (name, c.min(), c.max())
    # het: full, one-point and empty clouds on both sides, with hits where both sides have points
    radius, _ = BR.CASES["het"]
    c = BR.hit_counts(*BR.case("het"), radius)
    assert [len(v) for v in c] == [257, 1, 128, 0] and c[0].max() > 8 and c[2].sum() == 0
    # split: a typical query has more than K hits, some have fewer, and the K-th hit lies past the first split
    radius, (K,) = BR.CASES["100x20000"]
    p1, p2, _, _ = BR.case("100x20000")
    c = BR.hit_counts(p1, p2, None, None, radius)[0]
    _, idx = BR.ball_query_ref(p1, p2, K=K, radius=radius)
    assert c.median() > K and (c < K).sum() >= 5 and (c == 0).any(), (c.median(), (c < K).sum())
    full = idx[0][c >= K]
    assert (full[:, K - 1] >= 3 * 1280).float().mean() > 0.5  # the cut falls in the 4th split or later, inside it
    print(f"[ball] split case: hits per query min {c.min()} median {c.median()} max {c.max()}; "
          f"K-th hit index median {full[:, K - 1].median()}")


def test_named_cases_cover_the_launch_regimes(lib):
    def geom(name, K, N=None):
        p1, p2, _, _ = BR.case(name)
        return kernels.ball_query_geometry(N or p1.shape[0], p1.shape[1], p2.shape[1], K)

    # one launch, one chunk, one tile
    for name in ("1x3", "strict", "first", "63x65"):
        qpg, splits, chunk = geom(name, 4)
        assert splits == 1 and BR.case(name)[1].shape[1] <= chunk <= 1024 and BR.case(name)[0].shape[1] <= qpg
    # one launch, two chunks, one workgroup of two waves
    assert geom("wave", 4) == (128, 1, 1024)
    # more than one query tile and splits > 1 (each split one chunk, the last one partial)
    qpg, splits, chunk = geom("513x2049", 7)
    assert qpg == 128 and 513 > 4 * qpg and splits == 3 and chunk == 1024
    # splits > 1 and more than one chunk inside a split
    qpg, splits, chunk = geom("100x20000", 16)
    assert splits == 16 and chunk == 1024 and -(-20000 // splits) > chunk
    # the same clouds as 300 copies: one launch
    assert geom("100x20000", 16, N=300)[1] == 1
    # het: several clouds, one launch
    assert geom("het", 8)[1] == 1 and geom("257x1000", 8)[1] == 1
    # the geometry does not depend on K, and the query tile grows once the chip is full
    assert kernels.ball_query_geometry(1, 20000, 20000, 1) == kernels.ball_query_geometry(1, 20000, 20000, 500)
    assert kernels.ball_query_geometry(300, 2000, 400, 16) == (512, 1, 400)
    assert kernels.ball_query_geometry(32, 512, 4096, 32)[1] > 1


def test_workspace_sizes(lib):
    for N, P1, P2, K in ((1, 1, 1, 1), (1, 100, 20000, 16), (1, 100, 20000, 500), (300, 2000, 400, 16)):
        ws = lib.mr_ball_query_workspace(N, P1, P2, K)
        splits = kernels.ball_query_geometry(N, P1, P2, K)[1]
        assert 0 < ws <= 4 * N * P1 * splits + 512, (N, P1, P2, K, ws)  # no (N, P1, splits, K) lists
        assert lib.mr_ball_query_backward_workspace(N, P1, P2, K) >= 3 * N * P2 * 12
    assert lib.mr_ball_query_workspace(1, 10, 10, 0) == 0 and lib.mr_ball_query_workspace(70000, 10, 10, 1) == 0
    assert lib.mr_ball_query_backward_workspace(1, 10, 10, 0) == 0


def test_abi_rejects_bad_arguments_without_touching_the_gpu(lib):
    one = 1  # any non-NULL pointer value: the checks below return before anything is read
    f = lib.mr_ball_query
    assert f(None, one, 1, 4, 4, None, None, 0.5, 1, one, one, one, 256, None) == 1 and b"NULL" in lib.mr_last_error()
    assert f(one, None, 1, 4, 4, None, None, 0.5, 1, one, one, one, 256, None) == 1
    assert f(one, one, 1, 4, 4, None, None, 0.5, 1, None, one, one, 256, None) == 1
    assert f(one, one, 1, 4, 4, None, None, 0.5, 1, one, None, one, 256, None) == 1
    assert f(one, one, 1, 4, 4, None, None, 0.5, 1, one, one, None, 256, None) == 1
    assert f(one, one, 0, 4, 4, None, None, 0.5, 1, one, one, one, 256, None) == 1
    assert f(one, one, 1, 4, 4, None, None, 0.5, 0, one, one, one, 256, None) == 1 and b"K" in lib.mr_last_error()
    for bad in (-0.5, float("nan"), float("inf")):
        assert f(one, one, 1, 4, 4, None, None, bad, 1, one, one, one, 256, None) == 1
        assert b"radius" in lib.mr_last_error()
    assert f(one, one, 70000, 4, 4, None, None, 0.5, 1, one, one, one, 256, None) == 3
    for N, P1, P2, K in ((1, 4, 4, 500), (1, 100, 20000, 16)):
        ws = lib.mr_ball_query_workspace(N, P1, P2, K)
        assert f(one, one, N, P1, P2, None, None, 0.5, K, one, one, one, ws - 1, None) == 4
        assert b"too small" in lib.mr_last_error()
    b = lib.mr_ball_query_backward
    ws = lib.mr_ball_query_backward_workspace(1, 4, 4, 500)
    assert ws > 0 and ws == lib.mr_knn_points_backward_workspace(1, 4, 4, 32)
    assert lib.mr_knn_points_backward_workspace(1, 4, 4, 33) == 0  # the knn entry points keep their cap
    assert b(one, one, 1, 4, 4, None, None, 500, one, one, one, one, one, ws - 1, None) == 4  # K = 500 passes the checks
    assert b"too small" in lib.mr_last_error()
    assert b(one, one, 1, 4, 4, None, None, 0, one, one, one, one, one, ws, None) == 1
    assert b(one, one, 0, 4, 4, None, None, 4, one, one, one, one, one, ws, None) == 1
    for hole in range(5):
        args = [one] * 5
        args[hole] = None
        assert b(one, one, 1, 4, 4, None, None, 4, *args, ws, None) == 1 and b"NULL" in lib.mr_last_error()
    assert b(None, one, 1, 4, 4, None, None, 4, one, one, one, one, one, ws, None) == 1
    g = lib.mr_ball_query_geometry
    assert g(1, 4, 4, 0, None, None, None) == 1 and g(0, 4, 4, 1, None, None, None) == 1
    assert g(70000, 4, 4, 1, None, None, None) == 3 and g(1, 4, 4, 100000, None, None, None) == 0


def test_python_errors_come_before_any_device_use():
    g = torch.Generator().manual_seed(0)
    p1, p2 = torch.randn(2, 5, 3, generator=g), torch.randn(2, 7, 3, generator=g)
    with pytest.raises(ValueError):
        ops.ball_query(p1, p2[:1])  # batch
    with pytest.raises(ValueError):
        ops.ball_query(p1, p2[..., :2])  # D differs
    with pytest.raises(ValueError):
        ops.ball_query(p1[0], p2[0])  # not (N, P, D)
    with pytest.raises(ValueError):
        ops.ball_query(p1, p2, lengths1=torch.tensor([5]))
    with pytest.raises(ValueError):
        ops.ball_query(p1, p2, lengths2=torch.tensor([[7, 7]]))
    with pytest.raises(NotImplementedError):
        ops.ball_query(p1[..., :2], p2[..., :2])  # D = 2
    for K in (0, -3):
        with pytest.raises(ValueError):
            ops.ball_query(p1, p2, K=K)
        with pytest.raises(ValueError):
            kernels.ball_query(p1, p2, K=K)
    for radius in (-0.1, float("nan"), float("inf"), -math.inf):
        with pytest.raises(ValueError):
            ops.ball_query(p1, p2, radius=radius)
        with pytest.raises(ValueError):
            kernels.ball_query(p1, p2, radius=radius)
    for call in (lambda: ops.ball_query(p1, p2), lambda: kernels.ball_query(p1, p2, K=2, radius=0.0),
                 lambda: ops.ball_query(p1, p2, K=1000, radius=1.0, return_nn=False),
                 lambda: kernels.BallQuery.apply(p1, p2, None, None, 4, 0.5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError):
        ops.masked_gather(p2, torch.zeros(3, 5, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.masked_gather(p2, torch.zeros(2, dtype=torch.int64))


def test_masked_gather_against_a_loop():
    g = torch.Generator().manual_seed(1)
    N, P, U, L, K = 3, 6, 5, 4, 4
    x = torch.randn(N, P, U, generator=g, dtype=torch.float64, requires_grad=True)
    idx = torch.randint(-1, P, (N, L, K), generator=g)
    idx[1] = -1  # a cloud without a single neighbour
    assert (idx == -1).any() and (idx >= 0).any()
    want = torch.zeros(N, L, K, U, dtype=x.dtype)
    for n in range(N):
        for l in range(L):
            for k in range(K):
                if idx[n, l, k] >= 0:
                    want[n, l, k] = x[n, idx[n, l, k]].detach()
    got = ops.masked_gather(x, idx)
    assert got.shape == (N, L, K, U) and torch.equal(got.detach(), want)
    assert torch.equal(ops.masked_gather(x, idx.to(torch.int32)).detach(), want)
    w = torch.randn(N, L, K, U, generator=g, dtype=x.dtype)
    gx, = torch.autograd.grad((got * w).sum(), x)
    ref = torch.zeros_like(gx)
    for n in range(N):
        for l in range(L):
            for k in range(K):
                if idx[n, l, k] >= 0:
                    ref[n, idx[n, l, k]] += w[n, l, k]
    assert torch.allclose(gx, ref, rtol=0, atol=1e-12) and (gx[1] == 0).all()
    # (N, L) indices, as upstream
    two = ops.masked_gather(x, idx[..., 0])
    assert two.shape == (N, L, U) and torch.equal(two.detach(), want[:, :, 0])
