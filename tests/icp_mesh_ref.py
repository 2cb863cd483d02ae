"""A plain-torch restatement, on the CPU, of ops.iterative_closest_point_to_mesh's rule (include/mi355r.h): the
yardstick of test_icp_mesh_cpu.py / test_gpu_icp_mesh.py, and ``icp_mesh_composed`` is the baseline
tools/icp_mesh_bench.py times on the device.

What the rule fixes in float32 is float32 here, one torch op per operation: the transform (icp_plane_ref.sim_apply_ref),
the point-to-triangle distance with its barycentrics (point_mesh_ref.pair_terms) and the first minimum over the faces,
the closest point q = (b0 v0 + b1 v1) + b2 v2, the normal (the triangle's unit normal where the plane branch returned
the distance, else (p - q) / |p - q|), the validity test. The normal equations are formed in ``dtype`` (float64: the
restatement; float32: the conditioning probe), the step is icp_plane_ref.plane_step_ref. ``icp_mesh_ref`` returns every
iteration's transform, faces, q, n, validity and relative drop, so that two runs can be compared decision by decision.
"""
import math
from typing import NamedTuple

import torch

from tests import point_mesh_ref as PM
from tests.icp_plane_ref import plane_step_ref, sim_apply_ref
from tests.icp_ref import RTs, rotations

EPS = 1e-8
THR = 1e-4   # every case's relative_rmse_thr: at 1e-6 the drop at the noise floor is rounding (icp_plane_ref.THR)
RADII = (1.0, 0.7, 0.5)


def tri_unit_normals(tris, min_triangle_area):
    """(T,3) float32: tri_make's unit normal of tris (T,3,3), zeros where the plane branch is closed."""
    dt = tris.dtype
    v0, v1, v2 = tris[:, 0], tris[:, 1], tris[:, 2]
    e01, w = v1 - v0, -(v0 - v2)
    n = torch.stack((e01[:, 1] * w[:, 2] - e01[:, 2] * w[:, 1], e01[:, 2] * w[:, 0] - e01[:, 0] * w[:, 2],
                     e01[:, 0] * w[:, 1] - e01[:, 1] * w[:, 0]), -1)
    ln = PM._sqrt(PM._dot(n, n))
    plane = (0.5 * ln >= torch.tensor(min_triangle_area, dtype=dt)) & (ln > torch.tensor(EPS, dtype=dt))
    return torch.where(plane[:, None], n / torch.where(plane, ln, torch.ones_like(ln))[:, None], torch.zeros_like(n))


def mesh_tris(verts, faces, min_triangle_area):
    """(tris (T,3,3) float32, usable (T,) bool, unit normals (T,3)) of one mesh: a face with a vertex id out of range
    is not usable (its corners read vertex 0 here and are never used)."""
    verts, faces = verts.detach().cpu().float(), faces.detach().cpu().long().reshape(-1, 3)
    usable = ((faces >= 0) & (faces < verts.shape[0])).all(1)
    tris = verts[torch.where(usable[:, None], faces, torch.zeros_like(faces))] if faces.numel() else verts.new_zeros(0, 3, 3)
    return tris, usable, tri_unit_normals(tris, min_triangle_area)


def closest_ref(p, mesh, min_triangle_area):
    """Steps 1 and 2 for the float32 points p (L,3) against ``mesh`` = mesh_tris(...): (d (L,) float32, face (L,) int64,
    q (L,3), n (L,3)); without a usable face 0 / -1 / 0 / 0."""
    tris, usable, nhat = mesh
    L = p.shape[0]
    if L == 0 or not bool(usable.any()):
        return torch.zeros(L), torch.full((L,), -1, dtype=torch.int64), torch.zeros(L, 3), torch.zeros(L, 3)
    d_all, bary, inside = PM.pair_terms(p[:, None, :], tris[None], min_triangle_area)
    d_all = torch.where(usable[None], d_all, torch.full_like(d_all, float("inf")))
    f = d_all.argmin(dim=1)  # the first minimum
    rows = torch.arange(L)
    d, b, ins, t = d_all[rows, f], bary[rows, f], inside[rows, f], tris[f]
    q = (b[:, 0:1] * t[:, 0] + b[:, 1:2] * t[:, 1]) + b[:, 2:3] * t[:, 2]
    e = p - q
    l = PM._sqrt(PM._dot(e, e))
    far = l > torch.tensor(EPS)
    ne = torch.where(far[:, None], e / torch.where(far, l, torch.ones_like(l))[:, None], torch.zeros_like(e))
    return d, f, q, torch.where(ins[:, None], nhat[f], ne)


class ICPMeshRef(NamedTuple):
    converged: bool
    rmse: object
    Xt: torch.Tensor
    RTs: RTs
    t_history: list
    face_history: list    # per iteration (N, P1) int64: the winning face within the mesh, -1 for none
    q_history: list       # per iteration (N, P1, 3) float32 closest points
    n_history: list       # per iteration (N, P1, 3) float32 normals
    valid_history: list   # per iteration (N, P1) bool
    rel_history: list     # per iteration (N,) float32: the relative rmse drop the status test saw


def icp_mesh_ref(X, verts_list, faces_list, x_lengths=None, init=None, max_iterations=100, relative_rmse_thr=1e-6,
                 max_correspondence_distance=None, min_triangle_area=0.0, dtype=torch.float64):
    """The rule on X (N,P1,3) against the N meshes (verts_list[n] (V_n,3), faces_list[n] (T_n,3); equal list entries
    are prepared once)."""
    X = X.detach().cpu().float()
    N, P1, _ = X.shape
    lx = [P1] * N if x_lengths is None else [int(v) for v in x_lengths.tolist()]
    prepared = {}
    meshes = []
    for v, f in zip(verts_list, faces_list):
        if (id(v), id(f)) not in prepared:
            prepared[id(v), id(f)] = mesh_tris(v, f, min_triangle_area)
        meshes.append(prepared[id(v), id(f)])
    if init is None:
        R, T, s = torch.eye(3)[None].repeat(N, 1, 1), torch.zeros(N, 3), torch.ones(N)
    else:
        R, T, s = (t.detach().cpu().float().clone() for t in init)
    r2 = None
    if max_correspondence_distance is not None:
        d = torch.tensor(max_correspondence_distance, dtype=torch.float32)
        r2 = d * d
    mx = torch.stack([X[n, :lx[n]].double().mean(0) if lx[n] else torch.zeros(3, dtype=torch.float64) for n in range(N)])
    thr = torch.tensor(relative_rmse_thr, dtype=torch.float32)
    prev, rmse, converged = None, None, False
    hist, faces_h, qs, ns, valids, rels = [], [], [], [], [], []
    for _ in range(max_iterations):
        P = sim_apply_ref(X, R, T, s)  # float32
        face = torch.full((N, P1), -1, dtype=torch.int64)
        valid = torch.zeros(N, P1, dtype=torch.bool)
        Q, Nn = torch.zeros(N, P1, 3), torch.zeros(N, P1, 3)
        Rn, Tn = R.clone(), T.clone()
        m = torch.zeros(N)
        for n in range(N):
            d, f, q, nn = closest_ref(P[n, :lx[n]], meshes[n], min_triangle_area)
            face[n, :lx[n]], Q[n, :lx[n]], Nn[n, :lx[n]] = f, q, nn
            valid[n, :lx[n]] = (f >= 0) & (torch.ones_like(d, dtype=torch.bool) if r2 is None else d <= r2)
            v = valid[n]
            m[n] = float(v.sum())
            c64 = s[n].double() * (mx[n] @ R[n].double()) + T[n].double()
            p, qq, nv = P[n, v].to(dtype), Q[n, v].to(dtype), Nn[n, v].to(dtype)
            c = c64.to(dtype)
            r = ((p - qq) * nv).sum(1)
            J = torch.cat([torch.cross(p - c, nv, dim=1), nv], dim=1)  # (m, 6)
            R64, T64 = plane_step_ref(J.T @ J, J.T @ r, R[n], T[n], c64)
            Rn[n], Tn[n] = R64.float(), T64.float()
        R, T = Rn, Tn
        hist.append(RTs(R.clone(), T.clone(), s.clone()))
        faces_h.append(face)
        qs.append(Q)
        ns.append(Nn)
        valids.append(valid)
        P2 = sim_apply_ref(X, R, T, s)
        rr = ((P2.double() - Q.double()) * Nn.double()).sum(2) * valid
        rmse = ((rr * rr).sum(1) / m.double().clamp(min=1.0)).sqrt().float()
        rel = torch.ones(N) if prev is None else (prev - rmse) / prev
        rels.append(rel)
        done = (rel <= thr) | (m == 0)
        prev = rmse
        if bool(done.all()):
            converged = True
            break
    return ICPMeshRef(converged, rmse, sim_apply_ref(X, R, T, s), RTs(R, T, s), hist, faces_h, qs, ns, valids, rels)


# ---------------------------------------------------------------------------------------------------------------------
# Seeded data
# ---------------------------------------------------------------------------------------------------------------------
def bumped_ico(level, phase=0.0):
    """(verts (V,3) float32, faces (T,3) int64), T = 20 * 4**level: the unit ico-sphere scaled by RADII and bumped by a
    smooth field without symmetry, so that every rotation and translation is observable."""
    from torch_renderer_amd.utils import ico_sphere

    m = ico_sphere(level)
    v, f = m.verts_list()[0].double(), m.faces_list()[0].long()
    bump = 1.0 + 0.12 * torch.sin(3.0 * v[:, 0] + 1.0 + phase) * torch.cos(2.0 * v[:, 1] - 0.5) \
        + 0.08 * torch.sin(2.5 * v[:, 2] + 0.3 * v[:, 0] + 2.0 * phase)
    return (v * bump[:, None] * torch.tensor(RADII, dtype=torch.float64)).float(), f


def surface_samples(verts, faces, count, generator, cut=None):
    """(count,3) float64 area-weighted samples of the mesh's surface; ``cut`` = (direction (3,), offset): only points
    with x . direction <= offset are kept (a half space: a partial scan)."""
    v, f = verts.double(), faces.long()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = torch.linalg.cross(b - a, c - a).norm(dim=1)
    out = torch.zeros(0, 3, dtype=torch.float64)
    while out.shape[0] < count:
        k = torch.multinomial(area, 2 * count + 16, replacement=True, generator=generator)
        u = torch.rand(k.shape[0], 2, generator=generator, dtype=torch.float64)
        su = u[:, 0].sqrt()
        pts = (1 - su)[:, None] * a[k] + (su * (1 - u[:, 1]))[:, None] * b[k] + (su * u[:, 1])[:, None] * c[k]
        if cut is not None:
            pts = pts[pts @ cut[0] <= cut[1]]
        out = torch.cat([out, pts])
    return out[:count]


def scan_case(level, lengths, seed, cut=False, shared=False, noise=1e-3, min_deg=10.0, max_deg=25.0, shift=0.17,
              bad_faces=False, pad_to=None):
    """Seeded float32 (X (N,P1,3), x_lengths, verts_list, faces_list, truth RTs taking X onto the meshes). Scan n is a
    surface sample of mesh n plus ``noise`` N(0,1), optionally cut by a half space through 0.2 along a random
    direction, moved by a rotation of min_deg..max_deg degrees and a shift <= ``shift`` per axis; ``pad_to`` widens the
    padded tensor beyond the longest scan. ``shared``: one mesh,
    the same list entry N times. ``bad_faces``: every mesh also gets one collapsed face and one face with a vertex id
    out of range, in front of its faces (so every face index moves by two)."""
    g = torch.Generator().manual_seed(seed)
    N, P1 = len(lengths), max(max(lengths), 1, pad_to or 0)
    X = torch.zeros(N, P1, 3)
    ang = torch.deg2rad(min_deg + (max_deg - min_deg) * torch.rand(N, generator=g))
    Rm = rotations(torch.randn(N, 3, generator=g), ang)  # float64
    Tm = shift * (2 * torch.rand(N, 3, generator=g, dtype=torch.float64) - 1)
    def mesh(n):
        v, f = bumped_ico(level, phase=0.7 * n)
        if bad_faces:
            f = torch.cat([torch.tensor([[3, 3, 3], [0, 1, BAD_ID]]), f])
        return v, f

    base = mesh(0) if shared else None
    verts_list, faces_list = [], []
    for n in range(N):
        v, f = base if shared else mesh(n)
        verts_list.append(v)
        faces_list.append(f)
        cutn = None
        if cut:
            d = torch.randn(3, generator=g, dtype=torch.float64)
            cutn = (d / d.norm(), 0.2)
        good = f[((f >= 0) & (f < v.shape[0])).all(1)]
        pts = surface_samples(v, good, lengths[n], g, cutn)
        pts = pts + noise * torch.randn(lengths[n], 3, generator=g, dtype=torch.float64)
        X[n, :lengths[n]] = (pts @ Rm[n] + Tm[n]).float()
    Rt = Rm.transpose(1, 2)  # p = (x - Tm) Rm^T
    truth = RTs(Rt.float(), (-torch.bmm(Tm[:, None], Rt)[:, 0]).float(), torch.ones(N))
    xl = None if all(ln == P1 for ln in lengths) else torch.tensor(lengths)
    return X, xl, verts_list, faces_list, truth


# name -> (scan_case arguments, call options): the GPU suite's inputs (test_gpu_icp_mesh.py), whose condition
# test_icp_mesh_cpu.py checks. Four points cannot determine six unknowns (A has rank <= 4 and the step is decided by
# the damping, which float32 moments cannot reproduce), so the 1 x 4 x 20 shape is not a registration case: it is
# test_gpu_icp_mesh.py's closest-points input (TINY), and the smallest registration runs 24 points against T = 20.
# "many": 166 clouds in a tensor padded to 16,385 points (33 query tiles each) against T = 1,280, where the scan's
# geometry picks its largest face chunk (test_icp_mesh_cpu.py asks mr_icp_mesh_geometry). Every cloud is 40 points long,
# so all but the first query tile of a cloud leave at once, and the motions are small (2-5 degrees, shifts <= 0.03):
# with 10-25 degrees the worst of so many short clouds took the float32 and float64 restatements 6e-5 apart in two
# iterations. Only the kernels layer takes a tensor padded beyond its longest cloud (Pointclouds pad to the longest).
# "small": T = 20 is one partly filled chunk of the smallest size.
MANY = dict(level=3, lengths=[40] * 166, seed=4, shared=True, min_deg=2.0, max_deg=5.0, shift=0.03, pad_to=16385)
CASES = {
    "small": (dict(level=0, lengths=[24], seed=11), {}),
    "het": (dict(level=2, lengths=[300, 150, 40], seed=1, cut=True), {}),
    "tiles": (dict(level=2, lengths=[600, 600], seed=2), {}),
    "fine": (dict(level=3, lengths=[257], seed=3), {}),
    "many": (MANY, {"max_iterations": 2}),
    "shared": (dict(level=2, lengths=[200, 120], seed=5, shared=True, cut=True), {}),
    "init": (dict(level=2, lengths=[300, 150, 40], seed=6, cut=True), {"init": True}),
    "capped": (dict(level=2, lengths=[300, 150, 40], seed=7, cut=True), {"max_iterations": 2}),
    "maxd": (dict(level=2, lengths=[300], seed=8, min_deg=10.0, max_deg=12.0),
             {"displace": 40, "max_correspondence_distance": 0.2}),
    "edges": (dict(level=4, lengths=[300, 150], seed=9), {"min_triangle_area": 5e-3, "max_iterations": 3}),
    "badfaces": (dict(level=2, lengths=[150, 90], seed=10, bad_faces=True), {}),
}
# "edges": every face of the level-4 mesh (T = 5,120) lies below the area, so the target is the mesh's wireframe. A
# scan of the surface does not settle on it (the float64 restatement ran 20 iterations to an rmse of 7e-3 and the
# float32 one 25), so the case is capped: it checks the edges-only path, not convergence.
# "badfaces": the vertex id that is out of range. The library checks a face's ids against the packed batch's vertex
# count (a mesh's ids are offset by the vertices before it), so the id is one no offset brings back into range.
BAD_ID = 1 << 30
DISPLACED = 40   # "maxd": 40 source points are moved by (0.6, 0.6, 0.6)
_CACHE: dict = {}


def tiny():
    """The 1 cloud x 4 points x T = 20 input of the closest-points test: (X (1,4,3), verts, faces)."""
    if "tiny" not in _CACHE:
        X, _, vl, fl, _ = scan_case(0, [4], seed=12)
        _CACHE["tiny"] = (X, vl[0], fl[0])
    return _CACHE["tiny"]


def case(name):
    """(X, x_lengths, verts_list, faces_list, keyword arguments of icp_mesh_ref, truth) of a case, on the CPU,
    computed once and never modified. "init" starts 4 degrees and a 0.02 shift off the truth; "maxd" moves the 40
    points furthest along (1, 1, 1) outwards by 0.6, beyond the distance."""
    if ("case", name) not in _CACHE:
        data, opts = CASES[name]
        X, xl, vl, fl, truth = scan_case(**data)
        kw = {"relative_rmse_thr": THR, **opts}
        displace = kw.pop("displace", 0)
        if displace:
            X = X.clone()
            for n in range(X.shape[0]):
                X[n, torch.topk(X[n].double().sum(1), displace).indices] += 0.6
        if kw.pop("init", False):
            N = X.shape[0]
            g = torch.Generator().manual_seed(99)
            dR = rotations(torch.randn(N, 3, generator=g), torch.full((N,), math.radians(4.0))).float()
            kw["init"] = RTs(torch.bmm(truth.R, dR), truth.T + 0.02 * (2 * torch.rand(N, 3, generator=g) - 1), truth.s)
        _CACHE["case", name] = (X, xl, vl, fl, kw, truth)
    return _CACHE["case", name]


def restated(name, dtype):
    """icp_mesh_ref of a case with moments in `dtype`, computed once."""
    if (name, dtype) not in _CACHE:
        X, xl, vl, fl, kw, _ = case(name)
        _CACHE[name, dtype] = icp_mesh_ref(X, vl, fl, xl, dtype=dtype, **kw)
    return _CACHE[name, dtype]


def pose_error(R, T, truth):
    """(rotation angle in degrees (N,), translation distance (N,)) of (R, T) against the true transform, float64."""
    dR = torch.bmm(R.double().cpu(), truth.R.double().transpose(1, 2))
    cos = ((dR.diagonal(dim1=1, dim2=2).sum(1) - 1.0) / 2.0).clamp(-1.0, 1.0)
    return torch.rad2deg(torch.acos(cos)), (T.double().cpu() - truth.T.double()).norm(dim=1)


def icp_mesh_composed(X, verts, faces, init=None, max_iterations=100, relative_rmse_thr=1e-6, min_triangle_area=0.0):
    """The same estimator composed from torch ops on the tensors' device, float32, every cloud against the one mesh
    (verts (V,3), faces (T,3)): pair_terms over (N, P, T) -> argmin -> closest point and normal -> normal equations ->
    torch.linalg.solve, the convergence test every iteration (one host read). Materialises several (N, P, T, 3)
    tensors. Returns (converged, rmse, Xt, (R, T, s), iterations)."""
    N, P, _ = X.shape
    dev, dt = X.device, X.dtype
    tris = verts[faces.long()]
    nhat = tri_unit_normals(tris, min_triangle_area)
    R = torch.eye(3, device=dev, dtype=dt)[None].repeat(N, 1, 1)
    T, s = torch.zeros(N, 3, device=dev, dtype=dt), torch.ones(N, device=dev, dtype=dt)
    if init is not None:
        R, T, s = init
    eye6 = torch.eye(6, device=dev, dtype=dt)[None]
    Xt = s[:, None, None] * torch.bmm(X, R) + T[:, None, :]
    prev, rmse, converged, it = None, None, False, 0
    for it in range(1, max_iterations + 1):
        d, bary, inside = PM.pair_terms(Xt[:, :, None, :], tris[None, None], min_triangle_area)
        f = d.argmin(dim=2)
        b = bary.gather(2, f[..., None, None].expand(-1, -1, 1, 3))[:, :, 0]
        ins = inside.gather(2, f[..., None])[..., 0]
        del d, bary, inside
        t = tris[f]
        q = (b[..., 0:1] * t[..., 0, :] + b[..., 1:2] * t[..., 1, :]) + b[..., 2:3] * t[..., 2, :]
        e = Xt - q
        n = torch.where(ins[..., None], nhat[f], e / e.norm(dim=2, keepdim=True).clamp(min=EPS))
        c = Xt.mean(1, keepdim=True)
        r = ((Xt - q) * n).sum(2)
        J = torch.cat([torch.cross(Xt - c, n, dim=2), n], dim=2)
        A = torch.bmm(J.transpose(1, 2), J)
        bb = torch.bmm(J.transpose(1, 2), r[..., None])[..., 0]
        lam = 1e-9 * torch.diagonal(A, dim1=1, dim2=2).sum(1) / 6.0
        xi = torch.linalg.solve(A + lam[:, None, None] * eye6, -bb)
        w, tt = xi[:, :3], xi[:, 3:]
        K = torch.zeros(N, 3, 3, device=dev, dtype=dt)
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -w[:, 2], w[:, 1], w[:, 2]
        K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 0], -w[:, 1], w[:, 0]
        Et = torch.linalg.matrix_exp(K).transpose(1, 2)
        c = c[:, 0]
        R = torch.bmm(R, Et)
        T = torch.bmm((T - c)[:, None], Et)[:, 0] + c + tt
        Xt = s[:, None, None] * torch.bmm(X, R) + T[:, None, :]
        rmse = (((Xt - q) * n).sum(2) ** 2).mean(1).sqrt()
        rel = torch.ones_like(rmse) if prev is None else (prev - rmse) / prev
        if bool((rel <= relative_rmse_thr).all()):
            converged = True
            break
        prev = rmse
    return converged, rmse, Xt, (R, T, s), it
