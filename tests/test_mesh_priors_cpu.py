"""Host side of the mesh shape priors (torch_renderer_amd.loss): the cached topology the kernels read against a
brute-force Python loop, the Meshes edge methods, save_obj, the argument checks, and the plain-torch restatement
(tests/mesh_priors_ref.py) on the hand-checkable tetrahedron. No GPU."""
import io as _io
import math

import pytest
import torch

from tests.helpers import mesh_arrays
from tests.mesh_priors_ref import brute_topology, fan_mesh, priors_ref, tetrahedron
from torch_renderer_amd import Meshes, kernels
from torch_renderer_amd import loss as L
from torch_renderer_amd.io import load_obj, save_obj
from torch_renderer_amd.utils import ico_sphere


def _ico(level):
    m = ico_sphere(level)
    return m.verts_list()[0], m.faces_list()[0]


def _case(name):
    if name == "ico0":
        return [_ico(0)]
    if name == "fan":
        return [fan_mesh()]
    if name == "teapot":
        v, f, _ = mesh_arrays("teapot")
        return [(v, f)]
    return [_ico(0), _ico(1), fan_mesh()]  # a batch of three different meshes


@pytest.mark.parametrize("name", ["ico0", "fan", "teapot", "batch3"])
def test_topology_equals_brute_force(name):
    meshes = _case(name)
    faces = [f for _, f in meshes]
    Vs = [v.shape[0] for v, _ in meshes]
    t = kernels.mesh_prior_topology(faces, Vs)
    b = brute_topology(faces, Vs)
    N = len(meshes)
    assert (t.N, t.V, t.E, t.P) == (N, sum(Vs), b["edges"].shape[0], b["pairs"].shape[0])
    for k in ("edges", "nbr_ptr", "nbr", "pairs", "pair_ptr", "pair_idx"):
        got = getattr(t, k)
        assert got.dtype == torch.int32 and got.is_contiguous(), k
        assert torch.equal(got.long(), b[k]), k
    assert (t.edges[:, 0] < t.edges[:, 1]).all()
    key = t.edges[:, 0].long() * t.V + t.edges[:, 1].long()
    assert (key[1:] > key[:-1]).all()  # unique, sorted by min * V + max
    for k in ("edge_mesh_idx", "vert_mesh_idx", "num_edges_per_mesh"):
        assert torch.equal(getattr(t, k), b[k]), k
    # weights: 1 / (elements of that kind in the mesh * N), float32
    assert torch.equal(t.edge_w, (b["edge_w"] / N).float())
    assert torch.equal(t.pair_w, (b["pair_w"] / N).float())
    assert torch.equal(t.vert_w[:, 0], (b["vert_w"] / N).float())
    e_of_v = b["num_edges_per_mesh"][b["vert_mesh_idx"]].double()
    assert torch.equal(t.vert_w[:, 1], (1.0 / (e_of_v * N)).float())
    # every mesh's weights sum to 1 / N
    for m in range(N):
        assert abs(t.edge_w[t.edge_mesh_idx == m].double().sum().item() - 1.0 / N) < 1e-6
    if name == "fan":
        assert (t.E, t.P) == (7, 3)
        assert t.nbr_ptr[6] == t.nbr_ptr[5]  # the isolated vertex has no neighbour


@pytest.mark.parametrize("name,E,P", [("ico2", 480, 480), ("cow", 8784, 8784), ("teapot", 3756, 3636)])
def test_known_edge_and_pair_counts(name, E, P):
    if name == "ico2":
        v, f = _ico(2)
    else:
        v, f, _ = mesh_arrays(name)
    t = kernels.mesh_prior_topology([f], [v.shape[0]])
    assert (t.E, t.P) == (E, P)


def test_topology_is_cached_on_the_faces_tensor():
    v, f = _ico(1)
    src = Meshes([v], [f])
    t0 = kernels.mesh_prior_topology(src.faces_list(), [v.shape[0]])
    assert kernels.mesh_prior_topology(src.faces_list(), [v.shape[0]]) is t0
    moved = src.offset_verts(torch.zeros_like(v))  # a deformation step: new vertices, the same faces tensor
    assert kernels.mesh_prior_topology(moved.faces_list(), [v.shape[0]]) is t0
    assert kernels.mesh_prior_topology([f.clone()], [v.shape[0]]) is not t0
    f2 = src.faces_list()[0]
    f2[0] = f2[0].roll(1)  # an in-place edit bumps the version: rebuilt
    assert kernels.mesh_prior_topology([f2], [v.shape[0]]) is not t0


def test_topology_rejects_faces_outside_the_mesh():
    with pytest.raises(ValueError):
        kernels.mesh_prior_topology([torch.tensor([[0, 1, 4]])], [4])


def test_meshes_edge_methods():
    meshes = _case("batch3")
    m = Meshes([v for v, _ in meshes], [f for _, f in meshes])
    b = brute_topology([f for _, f in meshes], [v.shape[0] for v, _ in meshes])
    e = m.edges_packed()
    assert e.dtype == torch.int64 and torch.equal(e, b["edges"])
    assert torch.equal(m.num_edges_per_mesh(), b["num_edges_per_mesh"])
    assert m.num_edges_per_mesh().tolist() == [30, 120, 7]
    assert torch.equal(m.edges_packed_to_mesh_idx(), b["edge_mesh_idx"])
    assert torch.equal(m.verts_packed_to_mesh_idx(), b["vert_mesh_idx"])
    # an extended batch lists every copy, as upstream does
    x = Meshes([meshes[0][0]], [meshes[0][1]]).extend(3)
    assert x.edges_packed().shape == (90, 2) and x.num_edges_per_mesh().tolist() == [30, 30, 30]
    assert x.verts_packed_to_mesh_idx().tolist() == [0] * 12 + [1] * 12 + [2] * 12


def test_save_obj_round_trip(tmp_path):
    v, f = _ico(1)
    v = v + 0.01 * torch.randn(v.shape, generator=torch.Generator().manual_seed(0))
    p = tmp_path / "m.obj"
    save_obj(p, v, f, decimal_places=8)
    text = p.read_text().splitlines()
    assert text[0].startswith("v ") and text[-1] == "f %d %d %d" % tuple((f[-1] + 1).tolist())  # 1-based faces
    assert sum(ln.startswith("v ") for ln in text) == v.shape[0]
    assert sum(ln.startswith("f ") for ln in text) == f.shape[0]
    v2, faces2, aux = load_obj(p)
    assert torch.equal(faces2.verts_idx, f) and aux.verts_uvs is None
    assert torch.allclose(v2, v, rtol=0, atol=1e-7)
    buf = _io.StringIO()  # an open file, default "%f"
    save_obj(buf, v, f)
    assert buf.getvalue().splitlines()[0] == "v %f %f %f" % tuple(v[0].tolist())
    with pytest.raises(ValueError):
        save_obj(buf, v[:, :2], f)


@pytest.mark.parametrize("a", [1.0, 0.37])
def test_restatement_on_the_tetrahedron(a):
    v, f = tetrahedron(a)
    for dtype, tol in ((torch.float32, 1e-6), (torch.float64, 1e-12)):
        (edge, lap, normal), _ = priors_ref([v], [f], 0.0, dtype)
        assert abs(edge.item() - a * a) <= tol * a * a
        assert abs(lap.item() - a * math.sqrt(6.0) / 3.0) <= tol * a
        assert abs(normal.item() - 4.0 / 3.0) <= tol * 2
    (edge, _, _), grads = priors_ref([v], [f], a, torch.float64)
    assert abs(edge.item()) < 1e-24 and grads[0].abs().max() < 1e-12  # every edge at the target length
    # a batch of N copies has the single mesh's loss
    one, _ = priors_ref([v], [f], 0.1, torch.float64)
    three, _ = priors_ref([v, v, v], [f, f, f], 0.1, torch.float64)
    for x, y in zip(one, three):
        assert abs(x.item() - y.item()) < 1e-12


def test_cpu_tensors_raise():
    v, f = _ico(0)
    m = Meshes([v.requires_grad_(True)], [f])
    for fn in (L.mesh_shape_priors, L.mesh_edge_loss, L.mesh_laplacian_smoothing, L.mesh_normal_consistency):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(m)


def test_laplacian_methods():
    v, f = _ico(0)
    m = Meshes([v], [f])
    for method in ("cot", "cotcurv"):
        with pytest.raises(NotImplementedError):
            L.mesh_laplacian_smoothing(m, method=method)
    with pytest.raises(ValueError):
        L.mesh_laplacian_smoothing(m, method="mean")


def test_empty_meshes_give_a_zero_that_requires_grad():
    m = Meshes([torch.zeros(0, 3)], [torch.zeros(0, 3, dtype=torch.int64)])
    outs = (*L.mesh_shape_priors(m), L.mesh_edge_loss(m), L.mesh_laplacian_smoothing(m), L.mesh_normal_consistency(m))
    for out in outs:
        assert out.shape == (1,) and out.dtype == torch.float32 and out.requires_grad and out.item() == 0.0


def test_loss_module_mirrors_losses():
    from torch_renderer_amd import losses

    assert sorted(L.__all__) == ["mesh_edge_loss", "mesh_laplacian_smoothing", "mesh_normal_consistency",
                                 "mesh_shape_priors"]
    for name in L.__all__:
        assert getattr(L, name) is getattr(losses, name)
