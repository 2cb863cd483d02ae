"""iterative_closest_point_to_mesh without a GPU: the import path, every argument error of the Python layer (and CPU
tensors refused), the C ABI's checks before any launch, the scan's launch geometry of the GPU cases, the restatement of
tests/icp_mesh_ref.py against hand values, and the input condition of the GPU suite: on every case of
icp_mesh_ref.CASES the restatement with float32 moments makes the decisions of the float64 one."""
import ctypes
import math
import os

import pytest
import torch

from tests import icp_mesh_ref as MR
from torch_renderer_amd import Meshes, Pointclouds, _lib, kernels
from torch_renderer_amd.ops import ICPSolution, SimilarityTransform

MR_EINVAL, MR_EUNSUPPORTED, MR_EWORKSPACE = 1, 3, 4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from torch_renderer_amd import _build

        _build.build()
    return _lib.load()


def _p2mesh():
    from torch_renderer_amd.ops import iterative_closest_point_to_mesh

    return iterative_closest_point_to_mesh


def _inputs(N=2, P=5):
    g = torch.Generator().manual_seed(0)
    v, f = MR.bumped_ico(0)
    return torch.randn(N, P, 3, generator=g), Meshes([v] * N, [f] * N)


def test_import_path_and_signature():
    import inspect

    from torch_renderer_amd import ops

    fn = _p2mesh()
    assert ops.iterative_closest_point_to_mesh is fn
    assert list(inspect.signature(fn).parameters)[:7] == [
        "X", "meshes", "init_transform", "max_iterations", "relative_rmse_thr", "max_correspondence_distance",
        "min_triangle_area"]
    d = {k: p.default for k, p in inspect.signature(fn).parameters.items()}
    assert d["init_transform"] is None and d["max_iterations"] == 100 and d["relative_rmse_thr"] == 1e-6
    assert d["max_correspondence_distance"] is None and d["min_triangle_area"] == 0.0
    assert "status_batch" in inspect.signature(kernels.icp_mesh).parameters
    assert list(inspect.signature(kernels.mesh_closest_points).parameters) == ["x", "verts", "batch", "rts",
                                                                               "min_triangle_area"]
    assert ICPSolution._fields == ("converged", "rmse", "Xt", "RTs", "t_history")
    assert "true surface" in fn.__doc__ and "5e-3" in fn.__doc__  # the default area is said to differ from upstream's


def test_cpu_tensors_are_refused():
    fn = _p2mesh()
    x, meshes = _inputs()
    v, f = MR.bumped_ico(0)
    batch = kernels.PointMeshBatch(None, None, 5, f.int(), torch.zeros(2, dtype=torch.int64),
                                   torch.full((2,), 20, dtype=torch.int64), 20)
    for call in (lambda: fn(x, meshes),
                 lambda: fn(Pointclouds([x[0], x[1, :3]]), meshes),
                 lambda: fn(x, Meshes([v], [f]).extend(2)),
                 lambda: fn(x, meshes, max_iterations=0),
                 lambda: fn(x, meshes, max_correspondence_distance=0.5, min_triangle_area=5e-3),
                 lambda: kernels.icp_mesh(x, v, batch),
                 lambda: kernels.mesh_closest_points(x, v, batch)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_argument_errors():
    fn = _p2mesh()
    x, meshes = _inputs()
    v, f = MR.bumped_ico(0)
    with pytest.raises(ValueError, match="equal sized batches"):
        fn(x, Meshes([v], [f]))
    with pytest.raises(ValueError, match="equal sized batches"):
        fn(x[:1], meshes)
    with pytest.raises(ValueError, match="equal sized batches"):
        fn(x, Meshes([v], [f]).extend(3))
    with pytest.raises(ValueError, match="must be a Meshes"):
        fn(x, x)
    with pytest.raises(ValueError, match="Pointclouds objects or tensors"):
        fn([x[0]], meshes)
    with pytest.raises(NotImplementedError, match="D = 3"):
        fn(x[..., :2], meshes)
    with pytest.raises(NotImplementedError, match="verbose"):
        fn(x, meshes, verbose=True)
    good = SimilarityTransform(torch.eye(3)[None].repeat(2, 1, 1), torch.zeros(2, 3), torch.ones(2))
    for bad in (good[:2], (good.R[:1], good.T, good.s), (good.R, good.T[:, :2], good.s), (good.R, good.T, good.s[:, None]), 5):
        with pytest.raises(ValueError, match="The initial transformation init_transform has to be"):
            fn(x, meshes, init_transform=bad)
    for bad in (-1.0, -1e-9, float("nan"), "far", True):
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            fn(x, meshes, max_correspondence_distance=bad)
        with pytest.raises(ValueError, match="min_triangle_area"):
            fn(x, meshes, min_triangle_area=bad)
    with pytest.raises(NotImplementedError, match="requires grad"):
        fn(x.clone().requires_grad_(True), meshes)
    with pytest.raises(NotImplementedError, match="requires grad"):
        fn(x, Meshes([v.clone().requires_grad_(True), v], [f, f]))
    with pytest.raises(NotImplementedError, match="requires grad"):
        fn(x, meshes, init_transform=(good.R.clone().requires_grad_(True), good.T, good.s))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):  # grad mode off: not refused for it
        fn(x.clone().requires_grad_(True), meshes)
    with pytest.raises(TypeError):
        fn(x, meshes, estimate_scale=True)
    # the kernels layer's own checks
    batch = kernels.PointMeshBatch(None, None, 5, f.int(), torch.zeros(2, dtype=torch.int64),
                                   torch.full((2,), 20, dtype=torch.int64), 20)
    with pytest.raises(ValueError, match="min_triangle_area"):
        kernels.icp_mesh(x, v, batch, min_triangle_area=-1.0)
    with pytest.raises(ValueError, match="max_correspondence_distance"):
        kernels.icp_mesh(x, v, batch, max_correspondence_distance=float("nan"))
    with pytest.raises(ValueError, match="shape \\(N,\\)"):
        kernels.icp_mesh(x[:1], v, batch)
    with pytest.raises(NotImplementedError, match="D = 3"):
        kernels.mesh_closest_points(x[..., :2], v, batch)


def test_abi_rejects_bad_arguments_without_touching_the_gpu(lib):
    """The codes and texts of the mr_icp_mesh_* checks, before any launch (no GPU here). `p` is host memory that is
    never dereferenced."""
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    big = 1 << 40

    def it(**k):
        return lib.mr_icp_mesh_iterate(k.get("x", p), k.get("N", 2), k.get("P1", 4), None, k.get("T", 20), k.get("ff", p),
                                       k.get("fc", p), k.get("mf", 20), k.get("r2", float("inf")), 1e-6,
                                       k.get("max_it", 10), k.get("its", 0), k.get("rts", p), k.get("hist", p),
                                       k.get("rmse", p), k.get("status", p), k.get("ws", p), k.get("wsb", big), None)

    def prep(**k):
        return lib.mr_icp_mesh_prepare(k.get("verts", p), k.get("V", 12), k.get("faces", p), k.get("T", 20),
                                       k.get("ff", p), k.get("fc", p), k.get("mf", 20), k.get("N", 2), 4,
                                       k.get("area", 0.0), k.get("ws", p), k.get("wsb", big), None)

    def close(**k):
        return lib.mr_icp_mesh_closest(k.get("x", p), k.get("N", 2), 4, None, None, k.get("T", 20), k.get("ff", p),
                                       k.get("fc", p), k.get("mf", 20), None, None, k.get("q", p), k.get("n", p),
                                       k.get("ws", p), k.get("wsb", big), None)

    def err():
        return lib.mr_last_error()

    assert it() == 0  # no iteration to enqueue: nothing touches the device
    for key in ("x", "rts", "hist", "rmse", "status", "ws"):
        assert it(**{key: None}) == MR_EINVAL and b"NULL" in err(), key
    for fn in (it, prep, close):
        for key in ("ff", "fc"):
            assert fn(**{key: None}) == MR_EINVAL and b"NULL" in err(), key
        assert fn(N=0) == MR_EINVAL and b">= 1" in err()
        assert fn(N=70000) == MR_EUNSUPPORTED and b"65535" in err()
        assert fn(T=-1) == MR_EINVAL and fn(mf=21) == MR_EINVAL and b"max_faces" in err()
        assert fn(mf=-1) == MR_EINVAL
        assert fn(T=1 << 30, mf=0) == MR_EUNSUPPORTED and b"32-bit" in err()
        assert fn(wsb=16) == MR_EWORKSPACE and b"too small" in err()
    assert it(max_it=0) == MR_EINVAL and b"max_iterations" in err()
    assert it(its=-1) == MR_EINVAL
    for r2 in (-1.0, float("nan")):
        assert it(r2=r2) == MR_EINVAL and b"max_dist2" in err()
    assert it(r2=0.0) == 0 and it(r2=0.25) == 0
    for key in ("verts", "faces", "ws"):
        assert prep(**{key: None}) == MR_EINVAL and b"NULL" in err(), key
    for area in (-1.0, float("nan")):
        assert prep(area=area) == MR_EINVAL and b"min_triangle_area" in err()
    assert prep(V=-1) == MR_EINVAL
    assert prep(T=0, mf=0, verts=None, faces=None) == 0  # meshes without faces: nothing to prepare
    for key in ("x", "q", "n", "ws"):
        assert close(**{key: None}) == MR_EINVAL and b"NULL" in err(), key
    assert lib.mr_icp_mesh_workspace(0, 4, 4) == 0 and lib.mr_icp_mesh_workspace(2, 1 << 31, 4) == 0
    assert lib.mr_icp_mesh_workspace(2, 4, -1) == 0 and lib.mr_icp_mesh_workspace(2, 4, 1 << 30) == 0
    # mr_icp_init is shared: the plane estimator's layout comes first, then 7 float4 per face and q, n per point
    for N, P1, T in ((1, 1, 0), (3, 300, 320), (300, 800, 5856)):
        need = lib.mr_icp_mesh_workspace(N, P1, T)
        assert need % 256 == 0 and need >= lib.mr_icp_plane_workspace(N, P1, 1) + T * 112 + 2 * N * P1 * 12
        assert lib.mr_icp_mesh_iterate(p, N, P1, None, T, p, p, T, float("inf"), 1e-6, 10, 0, p, p, p, p, p, need - 1,
                                       None) == MR_EWORKSPACE
        assert lib.mr_icp_mesh_iterate(p, N, P1, None, T, p, p, T, float("inf"), 1e-6, 10, 0, p, p, p, p, p, need,
                                       None) == 0
    assert lib.mr_version() == 5
    for name, nargs in (("mr_icp_mesh_workspace", 3), ("mr_icp_mesh_geometry", 7), ("mr_icp_mesh_prepare", 13),
                        ("mr_icp_mesh_iterate", 19), ("mr_icp_mesh_closest", 16)):
        assert name in _lib.EXPORTED_SYMBOLS and len(getattr(lib, name).argtypes) == nargs


def _geometry(lib, N, P1, max_faces):
    c, lo, hi = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    g = ctypes.c_int64()
    assert lib.mr_icp_mesh_geometry(N, P1, max_faces, ctypes.byref(c), ctypes.byref(lo), ctypes.byref(hi),
                                    ctypes.byref(g)) == 0
    return c.value, lo.value, hi.value, g.value


def test_the_cases_cover_the_scan_geometry(lib):
    """The scan stages between min_chunk and max_chunk faces per workgroup. "many" runs at the largest chunk, "small"
    and "badfaces" at the smallest with a partly filled last chunk, "tiles" crosses a query tile, and the chunk never
    leaves its range."""
    seen = {}
    for name in MR.CASES:
        X, _, _, fl, _, _ = MR.case(name)
        T = max(f.shape[0] for f in fl)
        seen[name] = (*_geometry(lib, X.shape[0], X.shape[1], T), T)
        c, lo, hi, groups, _ = seen[name]
        assert lo <= c <= hi and c % lo == 0 and groups == -(-X.shape[1] // 512) * -(-T // c)
    print(f"[icp mesh geometry] {seen}")
    c, lo, hi, _, T = seen["many"]
    assert c == hi and T > c
    for name in ("small", "badfaces"):
        c, lo, hi, _, T = seen[name]
        assert c == lo and T % c != 0
    assert seen["tiles"][3] == 2 * -(-320 // seen["tiles"][0])
    assert lib.mr_icp_mesh_geometry(0, 4, 4, None, None, None, None) == MR_EINVAL
    assert _geometry(lib, 1, 1, 0)[3] == 0  # no faces: no scan


# ---------------------------------------------------------------------------------------------------------------------
# The restatement
# ---------------------------------------------------------------------------------------------------------------------
def _square():
    """Two triangles that tile the square [-1, 1]^2 on z = 0, sharing the diagonal from (-1,-1) to (1,1)."""
    v = torch.tensor([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [-1.0, 1.0, 0.0]])
    return v, torch.tensor([[0, 1, 2], [0, 2, 3]])


def test_hand_values_of_the_closest_point_and_normal():
    v, f = _square()
    mesh = MR.mesh_tris(v, f, 0.0)
    p = torch.tensor([[0.5, -0.5, 0.25],    # above face 0: the plane branch, n = the face normal
                      [-0.5, 0.5, -0.5],    # below face 1
                      [2.0, 0.0, 0.0],      # in the plane, beyond the edge x = 1: n = +x
                      [2.0, 2.0, 1.0],      # beyond the corner (1, 1): n along (1, 1, 1)
                      [0.25, 0.25, 0.0]])   # on the surface: still the plane branch, the face normal
    d, face, q, n = MR.closest_ref(p, mesh, 0.0)
    assert torch.allclose(d, torch.tensor([0.0625, 0.25, 1.0, 3.0, 0.0]), atol=1e-6)
    assert face[:3].tolist() == [0, 1, 0]
    assert torch.allclose(q, torch.tensor([[0.5, -0.5, 0.0], [-0.5, 0.5, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0],
                                           [0.25, 0.25, 0.0]]), atol=1e-6)
    s3 = 1.0 / math.sqrt(3.0)
    assert torch.allclose(n.abs(), torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [s3, s3, s3],
                                                 [0.0, 0.0, 1.0]]), atol=1e-6)
    # the gradient does not depend on which of the tied faces wins: swap the faces' order
    d2, face2, q2, n2 = MR.closest_ref(p, MR.mesh_tris(v, f.flip(0), 0.0), 0.0)
    assert torch.allclose(q, q2, atol=1e-6) and torch.allclose(n[2:4], n2[2:4], atol=1e-6) and torch.allclose(d, d2, atol=1e-6)
    # every face as its edges (the area threshold above both faces): above the interior the closest point moves to
    # an edge and the normal follows it
    de, _, qe, ne = MR.closest_ref(p[:1], MR.mesh_tris(v, f, 5.0), 5.0)
    assert float(de) > 0.0625 and abs(float(qe[0, 2])) == 0 and abs(float(ne.norm()) - 1) < 1e-6 and abs(float(ne[0, 2])) < 1
    # on a vertex of faces that count as their edges there is no direction: the zero normal
    dz, _, qz, nz = MR.closest_ref(torch.tensor([[1.0, 1.0, 0.0]]), MR.mesh_tris(v, f, 5.0), 5.0)
    assert float(dz) == 0 and qz.tolist() == [[1.0, 1.0, 0.0]] and nz.abs().max() == 0
    # a face with a vertex id out of range is skipped; without a usable face: no pair
    d3, face3, _, _ = MR.closest_ref(p, MR.mesh_tris(v, torch.tensor([[0, 1, 4], [0, 2, 3]]), 0.0), 0.0)
    assert face3.tolist() == [1] * 5
    d4, face4, q4, n4 = MR.closest_ref(p, MR.mesh_tris(v, torch.tensor([[0, 1, 4]]), 0.0), 0.0)
    assert face4.tolist() == [-1] * 5 and d4.abs().max() == 0 and q4.abs().max() == 0 and n4.abs().max() == 0


def test_hand_value_a_lift_off_a_flat_mesh_is_fixed_in_one_step():
    """100 points over the square's interior, lifted by 0.1: every pair is the plane branch with r = 0.1, and one step
    gives T = (0, 0, -0.1), R = I and an rmse of 0 (to rounding). The in-plane motion is left to the damping: 0."""
    v, f = _square()
    u = torch.linspace(-0.8, 0.8, 10)
    gx, gy = torch.meshgrid(u, u, indexing="ij")
    X = torch.stack([gx.reshape(-1), gy.reshape(-1), torch.full((100,), 0.1)], dim=1)[None]
    sol = MR.icp_mesh_ref(X, [v], [f], max_iterations=1)
    assert sol.valid_history[0].all() and (sol.n_history[0][..., 2].abs() == 1).all()
    R1, T1, s1 = sol.t_history[0]
    assert torch.allclose(R1, torch.eye(3)[None], atol=1e-6) and torch.allclose(T1, torch.tensor([[0.0, 0.0, -0.1]]), atol=1e-6)
    assert s1.tolist() == [1.0] and sol.rmse.item() <= 1e-6 and sol.Xt[..., 2].abs().max() <= 1e-6


def test_restatement_edge_behaviour():
    """max_iterations = 0; every pair rejected; an empty cloud and a mesh without faces."""
    X, xl, vl, fl, kw, _ = MR.case("het")
    none = MR.icp_mesh_ref(X, vl, fl, xl, max_iterations=0)
    assert not none.converged and none.rmse is None and none.t_history == [] and torch.equal(none.Xt, X)
    far = MR.icp_mesh_ref(X[:1] + 5.0, vl[:1], fl[:1], max_correspondence_distance=1e-3, max_iterations=4)
    assert far.converged and len(far.t_history) == 1 and far.rmse.tolist() == [0.0]
    assert torch.equal(far.RTs.R, torch.eye(3)[None]) and far.RTs.T.abs().max() == 0 and not far.valid_history[0].any()
    gone = MR.icp_mesh_ref(X, vl, [fl[0], fl[1][:0], fl[2]], torch.tensor([300, 150, 0]), max_iterations=2)
    assert torch.equal(gone.RTs.R[1:], torch.eye(3)[None].repeat(2, 1, 1)) and gone.RTs.T[1:].abs().max() == 0
    assert gone.rmse[1:].tolist() == [0.0, 0.0] and gone.rmse[0] > 0 and (gone.face_history[0][1:] == -1).all()


@pytest.mark.parametrize("name", list(MR.CASES))
def test_input_condition_of_the_gpu_cases(name):
    """What makes the GPU comparison against the float64 restatement meaningful: with float32 moments the restatement
    runs the same number of iterations with the same ``converged``, the same validity for every point in every
    iteration, and its history is within 1e-5 of the float64 one. Face indices may differ where the closest point
    lies on a shared edge or vertex; q and n may not: q within 1e-5, and n within what the inputs' own difference
    explains. n is a unit vector u / |u| with u = p - q (or a face normal, which does not move), and
    |a/|a| - b/|b|| <= 2 |a - b| / max(|a|, |b|): so |n32 - n64| <= 2 (|p32 - p64| + |q32 - q64|) / l + 1e-6 with l
    the pair's distance. An input that fails this is replaced, not tolerated."""
    a, b = MR.restated(name, torch.float32), MR.restated(name, torch.float64)
    X, xl, vl, fl, kw, truth = MR.case(name)
    assert a.converged == b.converged and len(a.t_history) == len(b.t_history) >= 1
    differ = sum(int((p != q).sum()) for p, q in zip(a.valid_history, b.valid_history))
    faces = sum(int((p != q).sum()) for p, q in zip(a.face_history, b.face_history))
    worst = max((u.double() - v.double()).abs().max().item()
                for ta, tb in zip(a.t_history, b.t_history) for u, v in zip(ta, tb))
    wq = wn = 0.0
    start = kw.get("init") or MR.RTs(torch.eye(3)[None].repeat(X.shape[0], 1, 1), torch.zeros(X.shape[0], 3),
                                     torch.ones(X.shape[0]))
    for k in range(len(b.t_history)):
        ta, tb = (start, start) if k == 0 else (a.t_history[k - 1], b.t_history[k - 1])
        pa, pb = MR.sim_apply_ref(X, *ta), MR.sim_apply_ref(X, *tb)
        dq = (a.q_history[k] - b.q_history[k]).norm(dim=2)
        dn = (a.n_history[k] - b.n_history[k]).norm(dim=2)
        l = torch.maximum((pa - a.q_history[k]).norm(dim=2), (pb - b.q_history[k]).norm(dim=2))
        allowed = 2 * ((pa - pb).norm(dim=2) + dq) / l.clamp(min=1e-12) + 1e-6
        v = b.valid_history[k]
        wq = max(wq, float(dq[v].max()) if v.any() else 0.0)
        wn = max(wn, float((dn / allowed)[v].max()) if v.any() else 0.0)
    print(f"[icp mesh cases] {name}: {len(b.t_history)} iterations, converged {b.converged}, {differ} validity decisions "
          f"and {faces} faces differ, history f32 vs f64 moments {worst:.2e}, q {wq:.2e}, n / allowed {wn:.2f}, rmse "
          f"{[round(r, 6) for r in b.rmse.tolist()[:4]]}")
    assert differ == 0
    assert worst <= 1e-5
    assert wq <= 1e-5
    assert wn <= 1.0
    # no stopping decision is left to rounding. The loop stops when every cloud is done in the same iteration, so an
    # iteration's decision is safe when some cloud's drop is 5x above the threshold or every cloud's is 5x below it
    thr = kw["relative_rmse_thr"]
    for rel in b.rel_history[1:]:
        assert bool((rel >= 5 * thr).any()) or bool((rel <= thr / 5).all()), b.rel_history
    if "max_iterations" in kw:  # the capped cases stop before they converge
        assert not b.converged and len(b.t_history) == kw["max_iterations"]
    else:
        assert b.converged and 2 <= len(b.t_history) <= 13
        ang, shift = MR.pose_error(b.RTs.R, b.RTs.T, truth)
        assert float(ang.max()) < 0.5 and float(shift.max()) < 5e-3  # registered, to the 1e-3 noise
        assert float(b.rmse.max()) < 2e-3
    if "max_correspondence_distance" in kw:
        moved = torch.topk(X[0].double().sum(1), MR.DISPLACED).indices
        for valid in b.valid_history:
            assert not valid[0, moved].any() and int(valid.sum()) >= 200  # the bulk of the cloud still registers
    if "init" in kw:
        assert all(torch.equal(h.s, kw["init"].s) for h in b.t_history)
    if name == "edges":  # every face of the case lies below the area: no pair takes the plane branch
        assert not any(bool((n.norm(dim=2) - 1).abs().lt(1e-5).logical_not().logical_and(v).any())
                       for n, v in zip(b.n_history, b.valid_history))  # unit normals along p - q all the same
        areas = torch.cat([0.5 * torch.linalg.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).norm(dim=1)
                           for v, f in zip(vl, fl)])
        assert float(areas.max()) < kw["min_triangle_area"]
    if name == "badfaces":  # the collapsed face 0 and the out-of-range face 1 lead every mesh
        assert all(f[0].tolist() == [3, 3, 3] and int(f[1].max()) == MR.BAD_ID for v, f in zip(vl, fl))
        assert all(int((h == 1).sum()) == 0 for h in b.face_history)
    if name == "shared":
        assert vl[0] is vl[1] and fl[0] is fl[1]
