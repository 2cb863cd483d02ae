"""point_mesh_face_distance without a GPU: the plain-torch restatement (tests/point_mesh_ref.py) against an independent
float64 formulation and hand-computed values, the degenerate rule, the closed-form gradient, and the host logic of
the public functions, the structures' packed accessors and the C ABI's argument validation (no compute call here)."""
import ctypes
import math

import pytest
import torch

from tests import point_mesh_ref as R
from torch_renderer_amd import Meshes, Pointclouds, _lib, kernels
from torch_renderer_amd.loss import face_point_distance, point_face_distance, point_mesh_face_distance

HAND_TRI = torch.tensor([[[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]]])
# (point, exact squared distance) on HAND_TRI: over the interior above and below the plane; the three edge regions
# (v0v1, v1v2: the hypotenuse x + y = 4, v2v0); the three vertex regions; on the plane inside, on an edge, on a vertex
HAND = [((1.0, 1.0, 2.0), 4.0), ((1.0, 1.0, -3.0), 9.0),
        ((2.0, -1.0, 2.0), 5.0), ((3.0, 3.0, 0.0), 2.0), ((-2.0, 2.0, 0.0), 4.0),
        ((-1.0, -1.0, 0.0), 2.0), ((6.0, -1.0, 0.0), 5.0), ((-1.0, 6.0, 1.0), 6.0),
        ((1.0, 1.0, 0.0), 0.0), ((2.0, 0.0, 0.0), 0.0), ((4.0, 0.0, 0.0), 0.0)]


def hand_points():
    return torch.tensor([p for p, _ in HAND])


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _agree(a, b):
    """1e-12 relative, plus the rounding floor of the difference vector p - c: its components carry at most ~64
    float64 roundings of coordinates of magnitude <= 4 (delta = 64 * 2^-53 * 4), and d = |p - c|^2 moves by at most
    2 sqrt(3 d) delta + 3 delta^2 under them. Without the floor a distance of exactly 0 could not be compared."""
    delta = 64 * 2.0 ** -53 * 4
    tol = 1e-12 * b.abs() + 2 * (3 * b.abs()).sqrt() * delta + 3 * delta ** 2
    assert ((a - b).abs() <= tol).all(), ((a - b).abs() / tol).max().item()


def test_restatement_equals_the_independent_formulation():
    pts = torch.cat([_randn(200, 3, seed=1), hand_points()]).double()
    tris = torch.cat([_randn(150, 3, 3, seed=2), 0.1 * _randn(50, 3, 3, seed=3), HAND_TRI]).double()
    a = R.pair_dist(pts, tris, 0.0, torch.float64)
    b = R.tri_dist_voronoi(pts, tris)
    _agree(a, b)
    # the float32 restatement is the same function to float32 rounding (the project's parity bar)
    c = R.pair_dist(pts, tris, 0.0, torch.float32).double()
    assert ((c - b).abs() <= 1e-4 * b.abs().clamp(min=1.0)).all()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("area", [5e-3, 0.0])
def test_hand_cases_are_exact(dtype, area):
    d = R.pair_dist(hand_points(), HAND_TRI, area, dtype)[:, 0]
    assert d.tolist() == [v for _, v in HAND]
    assert R.tri_dist_voronoi(hand_points(), HAND_TRI)[:, 0].tolist() == [v for _, v in HAND]


def test_area_rule():
    """Right triangles in the z = 0 plane with the right angle at the origin, a point 0.25 above each centroid.
    Legs 0.125 x 0.0625: area 0.0039 < 5e-3, so the triangle is its edges; the centroid's nearest edge is the
    hypotenuse at distance (2 area / 3) / |hyp|, squared (0.0078125 / 3)^2 / 0.01953125 = 1 / 2880, so
    d = 0.0625 + 1 / 2880; at min_triangle_area = 0 it is the plane distance, 0.0625. Legs 0.125 x 0.125: area
    0.0078 >= 5e-3, the plane branch, 0.0625 at both thresholds."""
    h = 0.25
    for legs, want in (((0.125, 0.0625), {5e-3: h * h + 1.0 / 2880.0, 0.0: h * h}),
                       ((0.125, 0.125), {5e-3: h * h, 0.0: h * h})):
        tri = torch.tensor([[[0.0, 0.0, 0.0], [legs[0], 0.0, 0.0], [0.0, legs[1], 0.0]]], dtype=torch.float64)
        p = torch.tensor([[legs[0] / 3, legs[1] / 3, h]], dtype=torch.float64)
        for area, v in want.items():
            d, _, inside = R.pair_terms(p, tri, area)
            assert abs(d.item() - v) <= 1e-12 * v, (legs, area, d.item(), v)
            assert bool(inside) == (v == h * h)
            d32 = R.pair_dist(p, tri, area, torch.float32).item()
            assert abs(d32 - v) <= 1e-6 * v


def _degenerate():
    tris = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]],     # collinear
                         [[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 0.0, 0.0]],     # collinear, the middle vertex last
                         [[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]],     # a point
                         [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 3.0, 0.0]]])    # one edge collapsed
    pts = torch.tensor([[0.5, 1.0, 0.0], [3.0, 0.0, 1.0], [1.0, 1.0, 3.0], [0.0, 1.0, 2.0]])
    return tris, pts


@pytest.mark.parametrize("area", [5e-3, 0.0])
def test_degenerate_triangles_are_finite(area):
    tris, pts = _degenerate()
    for dtype in (torch.float32, torch.float64):
        p = pts.clone().to(dtype).requires_grad_(True)
        t = tris.clone().to(dtype).requires_grad_(True)
        d = R.pair_terms(p[:, None, :], t[None], area)[0]
        assert torch.isfinite(d).all()
        d.sum().backward()
        assert torch.isfinite(p.grad).all() and torch.isfinite(t.grad).all()


@pytest.mark.parametrize("area", [5e-3, 0.0])
def test_degenerate_values_by_hand(area):
    """(The Voronoi-region formulation assumes a proper triangle, so these are checked by hand alone.)"""
    tris, pts = _degenerate()
    d = R.pair_dist(pts, tris, area, torch.float64)
    # point 0 = (0.5, 1, 0): the segment x in [0, 2] at distance 1; the point (1,1,1): 0.25 + 0 + 1; the segment
    # (0,0,0)-(0,3,0): 0.25
    assert d[0].tolist() == [1.0, 1.0, 1.25, 0.25]
    # point 2 = (1, 1, 3): 1 + 9 = 10 from the segment on the x axis, 4 from the point, 1 + 9 = 10 from the y segment
    assert d[2].tolist() == [10.0, 10.0, 4.0, 10.0]


def test_gradient_is_the_closed_form():
    """d/dp = 2 (p - c), d/dv_i = -2 b_i (p - c) with c = sum b_i v_i the closest point (the envelope theorem): the
    float64 autograd gradient of the restatement, for a weighted sum of row-wise pairs that cover the plane branch,
    the edges and the vertices at both thresholds."""
    for area in (5e-3, 0.0):
        p = torch.cat([_randn(300, 3, seed=4).double(), hand_points().double()]).requires_grad_(True)
        t = torch.cat([_randn(300, 3, 3, seed=5).double(), HAND_TRI.double().expand(len(HAND), 3, 3)])
        t = t.clone().requires_grad_(True)
        w = torch.rand(p.shape[0], generator=torch.Generator().manual_seed(6), dtype=torch.float64) + 0.5
        d, b, inside = R.pair_terms(p, t, area)
        assert 0 < int(inside.sum()) < inside.numel()
        (w * d).sum().backward()
        with torch.no_grad():
            c = (b[..., None] * t).sum(1)
            gp = 2 * w[:, None] * (p - c)
            gt = -b[..., None] * gp[:, None, :]
        scale = gp.abs().max().item()
        assert (p.grad - gp).abs().max().item() <= 1e-9 * scale
        assert (t.grad - gt).abs().max().item() <= 1e-9 * scale


# --------------------------------------------------------------------------- host logic
def _mesh(F=4, V=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(V, 3, generator=g), torch.randint(0, V, (F, 3), generator=g)


def test_public_function_argument_errors():
    v, f = _mesh()
    m2 = Meshes([v, v], [f, f])
    with pytest.raises(ValueError, match="meshes and pointclouds must be equal sized batches"):
        point_mesh_face_distance(m2, Pointclouds([_randn(7, 3)]))
    with pytest.raises(ValueError):
        point_mesh_face_distance(v, Pointclouds([_randn(7, 3)]))
    first = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="D = 3"):
        point_face_distance(_randn(7, 2), first, _randn(4, 3, 2), first)
    with pytest.raises(NotImplementedError, match="D = 3"):
        face_point_distance(_randn(7, 4), first, _randn(4, 3, 4), first)
    with pytest.raises(NotImplementedError, match="D = 3"):
        kernels.point_face_nearest(_randn(7, 2), first, first, _randn(5, 2), f, first, first, 0.0)
    with pytest.raises(ValueError):
        point_face_distance(_randn(7, 3), first, _randn(4, 3, 3), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="HIP device tensors"):  # no CPU fallback
        point_mesh_face_distance(Meshes([v], [f]), Pointclouds([_randn(7, 3)]))


def test_packed_accessors_on_heterogeneous_and_extended_batches():
    pc = Pointclouds([_randn(3, 3), torch.zeros(0, 3), _randn(5, 3, seed=1)])
    assert pc.cloud_to_packed_first_idx().tolist() == [0, 3, 3]
    assert pc.packed_to_cloud_idx().tolist() == [0] * 3 + [2] * 5
    assert pc.cloud_to_packed_first_idx().dtype == torch.int64
    ext = pc.extend(2)
    assert ext.cloud_to_packed_first_idx().tolist() == [0, 3, 6, 6, 6, 11]
    assert ext.packed_to_cloud_idx().tolist() == [0] * 3 + [1] * 3 + [4] * 5 + [5] * 5
    one = Pointclouds(_randn(1, 4, 3)).extend(3)
    assert one.cloud_to_packed_first_idx().tolist() == [0, 4, 8] and one.packed_to_cloud_idx().tolist() == \
        [0] * 4 + [1] * 4 + [2] * 4
    (v0, f0), (v1, f1) = _mesh(4, 5), _mesh(2, 6, seed=1)
    m = Meshes([v0, v1, v0], [f0, f1, torch.zeros(0, 3, dtype=torch.int64)])
    assert m.faces_packed_to_mesh_idx().tolist() == [0] * 4 + [1] * 2
    faces, first, count, mx = m._face_table()
    assert faces.dtype == torch.int32 and torch.equal(faces.long(), m.faces_packed())
    assert first.tolist() == [0, 4, 6] and count.tolist() == [4, 2, 0] and mx == 4
    assert m._face_table()[0] is faces  # cached on the faces tensors
    shared = Meshes([v0], [f0]).extend(3)
    assert shared.faces_packed_to_mesh_idx().tolist() == [0] * 4 + [1] * 4 + [2] * 4
    faces, first, count, mx = shared._face_table()
    assert torch.equal(faces.long(), shared.faces_packed()) and first.tolist() == [0, 4, 8] and count.tolist() == [4] * 3
    moved = shared.offset_verts(torch.zeros(15, 3))
    assert moved._face_table()[0] is faces  # an offset_verts result keeps the faces tensors: nothing is rebuilt


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _pm_call(lib, entry, *, N=1, P=8, T=4, V=5, max_points=None, max_faces=None, area=5e-3, nullify=(), ws_bytes=1 << 40,
             tail=None):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)  # non-NULL, never dereferenced
    batch = {"points": p, "P": P, "pf": p, "pc": p, "maxp": P if max_points is None else max_points, "verts": p, "V": V,
             "faces": p, "T": T, "ff": p, "fc": p, "maxf": T if max_faces is None else max_faces, "N": N, "area": area}
    for k in nullify:
        if k in batch:
            batch[k] = None
    if entry == "mr_point_mesh_face_backward":
        rest = {"idx_p": p, "idx_f": p, "coef": p, "grad_out": p, "gdp": None, "gdf": None, "gp": p, "gv": p, "ws": p}
    elif entry == "mr_point_mesh_face_forward":
        rest = {"idx_p": p, "idx_f": p, "coef": p, "out": p, "ws": p}
    else:
        rest = {"dist_p": p, "idx_p": p, "dist_f": p, "idx_f": p, "ws": p}
    for k in nullify:
        if k in rest:
            rest[k] = None
    rc = getattr(lib, entry)(*batch.values(), *rest.values(), ws_bytes, None)
    return rc, lib.mr_last_error()


@pytest.mark.parametrize("entry", ["mr_point_face_nearest", "mr_point_mesh_face_forward", "mr_point_mesh_face_backward"])
def test_capi_validation_is_shared_and_launches_nothing(lib, entry):
    """The three entry points reject bad arguments with a status and a message before any launch or memset (no GPU
    here: the pointers are host memory that is never read)."""
    rc, msg = _pm_call(lib, entry, N=0)
    assert rc == 1 and b"N must be >= 1" in msg
    rc, msg = _pm_call(lib, entry, P=-1)
    assert rc == 1 and b">= 0" in msg
    rc, msg = _pm_call(lib, entry, P=2 ** 31)
    assert rc == 3 and b"32-bit" in msg
    with pytest.raises(NotImplementedError):
        _lib.check(rc)
    assert _pm_call(lib, entry, N=65536)[0] == 3
    rc, msg = _pm_call(lib, entry, max_points=9)
    assert rc == 1 and b"max_points" in msg
    rc, msg = _pm_call(lib, entry, area=-1.0)
    assert rc == 1 and b"min_triangle_area" in msg
    assert _pm_call(lib, entry, area=math.nan)[0] == 1
    for k in ("points", "verts", "faces", "pf", "pc", "ff", "fc", "ws"):
        rc, msg = _pm_call(lib, entry, nullify=(k,))
        assert rc == 1 and b"NULL" in msg, k
    rc, msg = _pm_call(lib, entry, ws_bytes=0)
    assert rc == 4 and b"workspace too small" in msg
    if entry == "mr_point_mesh_face_forward":
        assert _pm_call(lib, entry, nullify=("out",))[0] == 1
    if entry == "mr_point_mesh_face_backward":
        rc, msg = _pm_call(lib, entry, nullify=("coef",))
        assert rc == 1 and b"neither" in msg
        assert _pm_call(lib, entry, nullify=("gp",))[0] == 1 and _pm_call(lib, entry, nullify=("gv",))[0] == 1


def test_capi_workspace_queries(lib):
    a = lib.mr_point_face_nearest_workspace(1, 1000, 320)
    assert a >= 8 * 1320 and lib.mr_point_mesh_face_workspace(1, 1000, 320) == a
    assert lib.mr_point_face_nearest_workspace(4, 20000, 5856) > a
    assert lib.mr_point_face_nearest_workspace(0, 10, 10) == 0 and lib.mr_point_face_nearest_workspace(1, 2 ** 31, 1) == 0
    assert lib.mr_point_mesh_face_backward_workspace(1000, 162) >= 12 * 3 * 1162
    assert lib.mr_point_mesh_face_backward_workspace(-1, 1) == 0
