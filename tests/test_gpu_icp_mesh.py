"""iterative_closest_point_to_mesh (csrc/mr_icpmesh.hip) on the GPU against the float64 restatement of
tests/icp_mesh_ref.py run on the CPU.

* every case of icp_mesh_ref.CASES (whose restatements with float32 and float64 moments make the same decisions:
  test_icp_mesh_cpu.py::test_input_condition_of_the_gpu_cases): ``converged`` and the number of iterations equal the
  restatement's; every R and T of the history, the final RTs, rmse and Xt within 1e-4 * max(1, |ref|) of it, with the
  float32 restatement's own error printed beside; s is the initial scale bitwise;
* mesh_closest_points under a non-trivial transform: dist and idx bitwise point_face_nearest's on the transformed
  points, q and n within the bar of the restatement, |n| 1 or 0;
* bitwise: run to run, and with the status read after every iteration, every 3 or 8, or once at the end;
* Pointclouds in gives Pointclouds out, max_iterations = 0;
* an empty cloud and a mesh without faces beside full ones; a cloud of four points.
"""
import pytest
import torch

from tests import icp_mesh_ref as MR
from tests.helpers import report
from tests.icp_ref import apply_ref, rotations
from torch_renderer_amd import Meshes, Pointclouds, kernels
from torch_renderer_amd.ops import ICPSolution, SimilarityTransform, _split_rts, iterative_closest_point_to_mesh

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _as_pointclouds(t, lengths):
    n = [t.shape[1]] * t.shape[0] if lengths is None else lengths.tolist()
    return Pointclouds([t[i, :n[i]].to(DEV) for i in range(t.shape[0])])


def _meshes(vl, fl):
    if len(vl) > 1 and all(v is vl[0] for v in vl) and all(f is fl[0] for f in fl):  # a shared batch: one copy
        return Meshes([vl[0].to(DEV)], [fl[0].to(DEV)]).extend(len(vl))
    return Meshes([v.to(DEV) for v in vl], [f.to(DEV) for f in fl])


def _kw(kw):
    kw = dict(kw)
    init = kw.pop("init", None)
    if init is not None:
        kw["init_transform"] = SimilarityTransform(*(t.to(DEV) for t in init))
    return kw


def _run_padded(X, xl, vl, fl, kw):
    """A tensor padded beyond its longest cloud, against one shared mesh: the kernels layer's call, with the shared
    batch laid out as ops.iterative_closest_point_to_mesh lays it out (every cloud's range is the whole table)."""
    N = X.shape[0]
    assert all(v is vl[0] for v in vl) and all(f is fl[0] for f in fl)
    verts, f = vl[0].to(DEV), fl[0].to(DEV)
    faces, first, count, max_faces = kernels.mesh_face_table([f], (verts.shape[0],))
    batch = kernels.PointMeshBatch(None, xl.to(DEV), X.shape[1], faces, first.expand(N).contiguous(),
                                   count.expand(N).contiguous(), max_faces)
    conv, iters, rmse, xt, rts, hist = kernels.icp_mesh(X.to(DEV), verts, batch, xl.to(DEV), kw.get("init_transform"),
                                                        kw.get("max_iterations", 100), kw["relative_rmse_thr"],
                                                        kw.get("max_correspondence_distance"),
                                                        kw.get("min_triangle_area", 0.0))
    return ICPSolution(conv, rmse, xt, _split_rts(rts), [_split_rts(hist[i]) for i in range(iters)])


def _run(name, **over):
    X, xl, vl, fl, kw, _ = MR.case(name)
    kw = dict(_kw(kw), **over)
    if xl is not None and int(xl.max()) < X.shape[1]:
        return _run_padded(X, xl, vl, fl, kw)
    src = _as_pointclouds(X, xl) if xl is not None else X.to(DEV)  # lengths travel in Pointclouds
    return iterative_closest_point_to_mesh(src, _meshes(vl, fl), **kw)


def _padded(xt):
    return xt.points_padded() if isinstance(xt, Pointclouds) else xt


def _check(name, got):
    r32, r64 = MR.restated(name, torch.float32), MR.restated(name, torch.float64)
    X, xl, _, _, kw, _ = MR.case(name)
    N, P1 = X.shape[:2]
    assert got.converged == r64.converged
    assert len(got.t_history) == len(r64.t_history)
    for field in ("R", "T"):
        g = torch.stack([getattr(t, field) for t in got.t_history])
        ref = torch.stack([getattr(t, field) for t in r64.t_history])
        f32 = torch.stack([getattr(t, field) for t in r32.t_history])
        report(f"icp mesh {name} history {field} (float32 moments)", f32, ref)
        report(f"icp mesh {name} history {field}", g, ref)
        report(f"icp mesh {name} final {field}", getattr(got.RTs, field), getattr(r64.RTs, field))
    s0 = kw["init"].s if "init" in kw else torch.ones(N)
    for t in [got.RTs, *got.t_history]:
        assert torch.equal(t.s.cpu(), s0)  # the scale: bitwise the initial one
    report(f"icp mesh {name} rmse (float32 moments)", r32.rmse, r64.rmse)
    report(f"icp mesh {name} rmse", got.rmse, r64.rmse)
    valid = (torch.arange(P1)[None] < (torch.full((N,), P1) if xl is None else xl)[:, None])
    report(f"icp mesh {name} Xt (float32 moments)", r32.Xt * valid[..., None], r64.Xt * valid[..., None])
    report(f"icp mesh {name} Xt", _padded(got.Xt).cpu() * valid[..., None], r64.Xt * valid[..., None])
    R = got.RTs.R.cpu().double()
    ortho = (torch.bmm(R, R.transpose(1, 2)) - torch.eye(3, dtype=torch.float64)).abs().max().item()
    print(f"[icp mesh] {name}: {len(got.t_history)} iterations, |R R^T - I| = {ortho:.2e}")
    assert ortho <= 1e-5


@pytest.mark.parametrize("name", list(MR.CASES))
def test_matches_the_float64_restatement(name):
    got = _run(name)
    _check(name, got)
    kw = MR.case(name)[4]
    if "max_iterations" in kw:
        assert not got.converged and len(got.t_history) == kw["max_iterations"]


def _batch(X, xl, vl, fl):
    """(x, packed verts, PointMeshBatch) on the device, every mesh with its own copy of the vertices."""
    faces, first, count, max_faces = kernels.mesh_face_table([f.to(DEV) for f in fl], [v.shape[0] for v in vl])
    return X.to(DEV), torch.cat(vl).to(DEV), kernels.PointMeshBatch(None, None if xl is None else xl.to(DEV),
                                                                   X.shape[1], faces, first, count, max_faces)


@pytest.mark.parametrize("name", ["tiny", "het", "badfaces", "edges", "many"])
def test_closest_points_under_a_transform(name):
    """mesh_closest_points with a rotation, a shift and a scale per cloud: dist and idx are bitwise what
    point_face_nearest gives for the points similarity_transform wrote; q and n are the restatement's within the bar;
    |n| is 1 or 0; rows past a length are 0 / -1 / 0 / 0."""
    if name == "tiny":
        X, v, f = MR.tiny()
        xl, vl, fl, area = None, [v], [f], 0.0
    else:
        X, xl, vl, fl, kw, _ = MR.case(name)
        area = kw.get("min_triangle_area", 0.0)
    N, P1 = X.shape[:2]
    g = torch.Generator().manual_seed(21)
    R = rotations(torch.randn(N, 3, generator=g), 0.2 + 0.5 * torch.rand(N, generator=g)).float()
    rts = torch.cat([R.reshape(N, 9), 0.1 * torch.randn(N, 3, generator=g), 0.9 + 0.2 * torch.rand(N, 1, generator=g)], 1)
    x, verts, batch = _batch(X, xl, vl, fl)
    dist, idx, q, n = kernels.mesh_closest_points(x, verts, batch, rts.to(DEV), area)
    assert dist.shape == (N, P1) and idx.dtype == torch.int32 and q.shape == n.shape == (N, P1, 3)
    moved = kernels.similarity_transform(x, rts.to(DEV))
    lens = [P1] * N if xl is None else xl.tolist()
    first = torch.tensor([0] + lens[:-1]).cumsum(0).to(DEV)
    packed = torch.cat([moved[i, :lens[i]] for i in range(N)])
    dp, ip, _, _ = kernels.point_face_nearest(packed, first, torch.tensor(lens).to(DEV), verts, batch.faces,
                                              batch.faces_first, batch.faces_count, area, max(lens), batch.max_faces)
    off = 0
    meshes = {}
    for i in range(N):
        L = lens[i]
        assert torch.equal(dist[i, :L], dp[off:off + L]) and torch.equal(idx[i, :L], ip[off:off + L])
        assert dist[i, L:].abs().sum() == 0 and (idx[i, L:] == -1).all() and q[i, L:].abs().sum() == 0 and n[i, L:].abs().sum() == 0
        if i < 3:  # the restatement on the very points the kernels searched from
            key = (id(vl[i]), id(fl[i]))
            meshes[key] = meshes.get(key) or MR.mesh_tris(vl[i], fl[i], area)
            d_ref, f_ref, q_ref, n_ref = MR.closest_ref(moved[i, :L].cpu(), meshes[key], area)
            assert torch.equal(dist[i, :L].cpu(), d_ref) and torch.equal(idx[i, :L].cpu().long(), f_ref)
            report(f"mesh closest {name}[{i}] q", q[i, :L], q_ref)
            report(f"mesh closest {name}[{i}] n", n[i, :L], n_ref)
        off += L
    norm = n.norm(dim=2)
    assert bool(((norm - 1).abs() <= 1e-5).logical_or(norm == 0).all())
    assert bool((norm[idx >= 0] > 0).all())  # noisy scans: no point lies on the surface to 1e-8
    # without a transform: the points as they are
    d0, i0, _, _ = kernels.mesh_closest_points(x, verts, batch, None, area)
    p0 = torch.cat([x[i, :lens[i]] for i in range(N)])
    dp0, ip0, _, _ = kernels.point_face_nearest(p0, first, torch.tensor(lens).to(DEV), verts, batch.faces,
                                                batch.faces_first, batch.faces_count, area, max(lens), batch.max_faces)
    assert torch.equal(torch.cat([d0[i, :lens[i]] for i in range(N)]), dp0)
    assert torch.equal(torch.cat([i0[i, :lens[i]] for i in range(N)]), ip0)


def _flat(sol):
    return [sol.rmse, _padded(sol.Xt), *sol.RTs] + [t for h in sol.t_history for t in h]


@pytest.mark.parametrize("name", ["tiles", "het"])
def test_bitwise_reproducible_and_independent_of_the_status_batch(name):
    X, xl, vl, fl, _, _ = MR.case(name)
    x, verts, batch = _batch(X, xl, vl, fl)
    runs = [kernels.icp_mesh(x, verts, batch, batch.points_count, status_batch=b) for b in (None, None, 1, 3, 8, 100)]
    first = runs[0]  # the default threshold 1e-6: the runs are compared with each other, bit for bit
    assert 2 <= first[1] <= 100
    for r in runs[1:]:
        assert r[0] == first[0] and r[1] == first[1]
        for a, b in zip(first[2:], r[2:]):
            assert torch.equal(a, b)
    a, b = _run(name), _run(name)
    assert all(torch.equal(u, v) for u, v in zip(_flat(a), _flat(b)))


def test_a_shared_batch_equals_separate_copies():
    """Meshes.extend(N) is read in place (one copy of vertices and faces, every cloud's range the whole table) and
    gives bitwise what N separate copies of the mesh give."""
    X, xl, vl, fl, kw, _ = MR.case("shared")
    a = _run("shared")
    copies = Meshes([v.clone().to(DEV) for v in vl], [f.clone().to(DEV) for f in fl])
    b = iterative_closest_point_to_mesh(_as_pointclouds(X, xl), copies, **_kw(kw))
    assert a.converged == b.converged and all(torch.equal(u, v) for u, v in zip(_flat(a), _flat(b)))


def test_pointclouds_in_pointclouds_out_and_the_kernels_call():
    X, xl, vl, fl, kw, _ = MR.case("het")
    got = _run("het")
    assert isinstance(got.Xt, Pointclouds) and got.Xt.counts() == [300, 150, 40]
    assert got.rmse.shape == (3,) and got.RTs.R.shape == (3, 3, 3) and got.RTs.T.shape == (3, 3) and got.RTs.s.shape == (3,)
    x, verts, batch = _batch(X, xl, vl, fl)
    raw = kernels.icp_mesh(x, verts, batch, xl.to(DEV), relative_rmse_thr=MR.THR)
    assert raw[0] == got.converged and raw[1] == len(got.t_history)
    assert torch.equal(raw[2], got.rmse) and torch.equal(raw[3], got.Xt.points_padded())
    assert torch.equal(raw[4][:, :9].reshape(3, 3, 3), got.RTs.R) and torch.equal(raw[4][:, 9:12], got.RTs.T)
    X2, _, vl2, fl2, kw2, _ = MR.case("fine")
    a = iterative_closest_point_to_mesh(Pointclouds(X2.to(DEV)), _meshes(vl2, fl2), **_kw(kw2))
    b = iterative_closest_point_to_mesh(X2.to(DEV), _meshes(vl2, fl2), **_kw(kw2))
    assert isinstance(a.Xt, Pointclouds) and torch.is_tensor(b.Xt)
    assert all(torch.equal(u, v) for u, v in zip(_flat(a), _flat(b)))


def test_without_iterations():
    X, _, vl, fl, _, _ = MR.case("tiles")
    g = torch.Generator().manual_seed(5)
    init = SimilarityTransform(rotations(torch.randn(2, 3, generator=g), torch.tensor([0.3, 1.0])).float().to(DEV),
                               torch.randn(2, 3, generator=g).to(DEV), torch.tensor([0.5, 2.0]).to(DEV))
    got = iterative_closest_point_to_mesh(X.to(DEV), _meshes(vl, fl), init_transform=init, max_iterations=0)
    assert got.converged is False and got.rmse is None and got.t_history == []
    report("icp mesh max_iterations=0 Xt", got.Xt, apply_ref(X.double(), *(t.cpu().double() for t in init)))
    for a, b in zip(got.RTs, init):
        assert torch.equal(a, b)


def test_an_empty_cloud_and_a_mesh_without_faces():
    """Four pairs: a full one, an empty cloud against a mesh, a cloud against a mesh without faces, a cloud whose every
    pair lies beyond the distance. The last three keep their (given) transform bit for bit in every iteration and
    report rmse 0; the first is bitwise what it is when run alone; they do not keep the batch from converging."""
    X, xl, vl, fl, kw, _ = MR.case("het")
    far = X[0] + 5.0
    src = Pointclouds([X[0].to(DEV), X[1, :0].to(DEV), X[2, :40].to(DEV), far.to(DEV)])
    verts = [vl[0], vl[1], vl[2], vl[0]]
    faces = [fl[0], fl[1], fl[2][:0], fl[0]]
    g = torch.Generator().manual_seed(6)
    init = SimilarityTransform(rotations(torch.randn(4, 3, generator=g), torch.tensor([0.0, 0.4, 0.2, 0.0])).float().to(DEV),
                               torch.tensor([[0.0, 0.0, 0.0], [0.1, -0.2, 0.3], [0.3, 0.0, -0.1], [0.0, 0.0, 0.0]]).to(DEV),
                               torch.ones(4).to(DEV))
    opts = dict(relative_rmse_thr=MR.THR, max_correspondence_distance=0.5)
    got = iterative_closest_point_to_mesh(src, _meshes(verts, faces), init_transform=init, **opts)
    alone = iterative_closest_point_to_mesh(X[:1].to(DEV), _meshes(vl[:1], fl[:1]),
                                            init_transform=SimilarityTransform(*(t[:1] for t in init)), **opts)
    assert got.converged and alone.converged and len(got.t_history) == len(alone.t_history) >= 2
    assert got.Xt.counts() == [300, 0, 40, 300]
    for k in (1, 2, 3):
        assert got.rmse[k] == 0
        for h in [got.RTs, *got.t_history]:
            assert torch.equal(h.R[k], init.R[k]) and torch.equal(h.T[k], init.T[k]) and torch.equal(h.s[k], init.s[k])
    assert torch.equal(got.RTs.R[0], alone.RTs.R[0]) and torch.equal(got.RTs.T[0], alone.RTs.T[0])
    assert torch.equal(got.rmse[0], alone.rmse[0])
    assert all(torch.equal(a.R[0], b.R[0]) and torch.equal(a.T[0], b.T[0]) for a, b in zip(got.t_history, alone.t_history))
    # nothing but such pairs: one iteration, converged, nothing moved
    lone = iterative_closest_point_to_mesh(far[None].to(DEV), _meshes(vl[:1], fl[:1]), max_correspondence_distance=0.5)
    assert lone.converged and len(lone.t_history) == 1 and lone.rmse[0] == 0
    assert torch.equal(lone.RTs.R[0].cpu(), torch.eye(3)) and lone.RTs.T.abs().max() == 0
    assert torch.equal(lone.Xt, far[None].to(DEV))


def test_a_cloud_of_four_points_is_finite():
    """1 cloud x 4 points x T = 20: four pairs against six unknowns, so no parity (the damping decides the step);
    shapes and finiteness only."""
    X, v, f = MR.tiny()
    got = iterative_closest_point_to_mesh(X.to(DEV), Meshes([v.to(DEV)], [f.to(DEV)]), max_iterations=3)
    assert 1 <= len(got.t_history) <= 3 and got.rmse.shape == (1,) and got.Xt.shape == (1, 4, 3)
    for t in _flat(got):
        assert torch.isfinite(t).all()
    assert torch.equal(got.RTs.s.cpu(), torch.ones(1))
