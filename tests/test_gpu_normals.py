"""estimate_pointcloud_normals / estimate_pointcloud_local_coord_frames on the MI355X (csrc/mr_normals.hip) against
the float64 restatement of tests/normals_ref.py (neighbour sets from a float32 stable sort, numpy.linalg.eigh).

Shapes: the split path (a scan and a merge) with one sphere of 300 points, two cow clouds of lengths (733, 257)
padded to 733 and one sphere of 1,100 points; the one-launch path with 256 clouds of 70 points; K = 5, 16, 32, 33, 50
(33 and 50 run in the 64 bucket). For every valid point, with tr = trace(C_ref):

* cov and curvatures within 1e-4 tr per entry (the covariance pins the neighbour set);
* frames: per-column residual |C_ref v - lambda v| <= 1e-4 tr, orthonormal to 1e-5, column 1 = cross(column 0, column 2)
  to 1e-5 when disambiguated, padded rows exactly 0;
* the normal: sin(angle to the reference normal) <= 2e-4 tr / (lambda_1 - lambda_0) (Davis-Kahan under the covariance
  bar) where the reference gap (lambda_1 - lambda_0) / tr >= 0.02, which must keep >= 95 % of the points;
* signs: with the returned vector v and the float64 projections proj_k = v . d_k, tau_k = 1e-5 |d_k|, no vector's
  sign may contradict the rule beyond tau (see _certainly_wrong), and >= 90 % of the points must be decisive;
* without disambiguation every column's largest component is positive where it leads the second by 1e-3.

Then: the result does not depend on the path (split against one launch, bit for bit), two runs are bitwise equal,
translated / rescaled / duplicated / collinear clouds, and the public interface with HIP graph capture.
"""
import functools

import numpy as np
import pytest
import torch

from tests import normals_ref as NR
from torch_renderer_amd import kernels
from torch_renderer_amd.ops import estimate_pointcloud_local_coord_frames, estimate_pointcloud_normals
from torch_renderer_amd.structures import Pointclouds

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KS = (5, 16, 32, 33, 50)


@functools.lru_cache(maxsize=None)
def cloud(name):
    """(points (N,P,3) float32, lengths or None) on the CPU (never modified)."""
    if name == "sphere300":
        return NR.sphere(300)[None], None
    if name == "sphere1100":
        return NR.sphere(1100, seed=1)[None], None
    if name == "cow":
        return NR.cow_clouds()
    if name == "batch70":  # 256 flattened gaussian blobs, each in its own orientation and place
        g = torch.Generator().manual_seed(70)
        x = torch.randn(256, 70, 3, generator=g, dtype=torch.float64) * torch.tensor([1.0, 0.6, 0.1], dtype=torch.float64)
        q, _ = torch.linalg.qr(torch.randn(256, 3, 3, generator=g, dtype=torch.float64))
        return (x @ q + torch.randn(256, 1, 3, generator=g, dtype=torch.float64)).float(), None
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ref(name, K, disambiguate=True):
    pts, lengths = cloud(name)
    return NR.frames_ref(pts, lengths, K, disambiguate)


def run(pts, lengths, K, disambiguate=True):
    cur, frm, cov = kernels.point_frames(pts.to(DEV), None if lengths is None else lengths.to(DEV), K, disambiguate,
                                         return_cov=True)
    torch.cuda.synchronize()
    assert cur.dtype == frm.dtype == cov.dtype == torch.float32
    return {"cur": cur.cpu().double().numpy(), "frames": frm.cpu().double().numpy(),
            "cov": NR.cov33(cov.cpu().numpy())}


# --------------------------------------------------------------------------- the checks (numpy, float64)
def check_values(out, r, disambiguate=True, what=""):
    """cov, curvatures and frames of `out` against the reference `r` at every valid point; exact zeros elsewhere."""
    ok = r["valid"]
    assert ok.any()
    for k in ("cur", "frames", "cov"):
        assert np.isfinite(out[k]).all(), (what, k)
        assert (out[k][~ok] == 0).all(), (what, k, "padded rows")
    C, tr = r["cov"][ok], np.trace(r["cov"][ok], axis1=1, axis2=2)
    lam, V = out["cur"][ok], out["frames"][ok]
    e_cov = np.abs(out["cov"][ok] - C).reshape(-1, 9).max(1)
    e_cur = np.abs(lam - r["cur"][ok]).max(1)
    res = np.linalg.norm(C @ V - V * lam[:, None, :], axis=1).max(1)
    orth = np.abs(np.swapaxes(V, 1, 2) @ V - np.eye(3)).reshape(-1, 9).max(1)
    nz = tr > 0
    rel = lambda e: (e[nz] / tr[nz]).max() if nz.any() else 0.0  # noqa: E731
    print(f"[normals] {what}: {ok.sum()} points, max / trace: cov {rel(e_cov):.2e}, curvatures {rel(e_cur):.2e}, "
          f"residual {rel(res):.2e}; |V^T V - I| {orth.max():.2e}")
    assert (e_cov <= 1e-4 * tr).all(), what
    assert (e_cur <= 1e-4 * tr).all(), what
    assert (res <= 1e-4 * tr).all(), what
    assert (orth <= 1e-5).all(), what
    if disambiguate:
        assert np.abs(np.cross(V[:, :, 0], V[:, :, 2]) - V[:, :, 1]).max() <= 1e-5, what


def check_normal_direction(out, r, what=""):
    ok = r["valid"]
    lam, tr = r["cur"][ok], r["cur"][ok].sum(1)
    gap = lam[:, 1] - lam[:, 0]
    keep = gap >= 0.02 * tr
    left_out = 1.0 - keep.mean()
    n, nr = out["frames"][ok][:, :, 0], r["frames"][ok][:, :, 0]
    sin = np.linalg.norm(np.cross(n, nr), axis=1)
    print(f"[normals] {what}: the gap filter leaves out {100 * left_out:.2f} %, max sin * gap / trace "
          f"{(sin[keep] * gap[keep] / tr[keep]).max():.2e}")
    assert left_out <= 0.05, what
    assert (sin[keep] * gap[keep] <= 2e-4 * tr[keep]).all(), what


def _certainly_wrong(v, d, K):
    """Per point: does the sign of the returned vector v (M,3) contradict the rule beyond tau_k = 1e-5 |d_k|?

    The rule negates the eigenvector u iff 2 #{u . d_k > 0} < K, so a returned v is right if it was kept
    (2 #{v . d_k > 0} >= K) or negated (2 #{v . d_k < 0} < K). The second clause matters: d_0 = 0 (the point itself)
    projects to 0 on both sides, so for an odd K a rightly negated vector can still have 2 #{v . d_k > 0} = K - 1.
    Certainly wrong: neither holds even with every projection inside +-tau counted in the vector's favour.
    Also returns the decisive points: 2 #{proj > tau} >= K or 2 #{proj > -tau} < K."""
    proj = np.einsum("mki,mi->mk", d, v)
    tau = 1e-5 * np.linalg.norm(d, axis=2)
    not_kept = 2 * (proj > -tau).sum(1) < K
    not_negated = 2 * (proj < -tau).sum(1) >= K
    decisive = (2 * (proj > tau).sum(1) >= K) | not_kept
    return not_kept & not_negated, decisive


def check_signs(out, r, K, what=""):
    ok = r["valid"]
    d = r["d"][ok]
    for col in (0, 2):
        wrong, decisive = _certainly_wrong(out["frames"][ok][:, :, col], d, K)
        print(f"[normals] {what} column {col}: {100 * decisive.mean():.1f} % decisive, {wrong.sum()} certainly wrong")
        assert decisive.mean() >= 0.9, (what, col)
        assert not wrong.any(), (what, col)


def check_largest_positive(out, r, what=""):
    V = out["frames"][r["valid"]]
    a = np.sort(np.abs(V), axis=1)
    lead = a[:, 2, :] - a[:, 1, :] > 1e-3
    big = np.take_along_axis(V, np.argmax(np.abs(V), axis=1)[:, None, :], axis=1)[:, 0, :]
    assert lead.mean() > 0.9 and (big[lead] > 0).all(), what


# --------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", ["sphere300", "cow", "sphere1100", "batch70"])
def test_frames_against_the_reference(name, K):
    pts, lengths = cloud(name)
    splits = kernels.frames_geometry(pts.shape[0], pts.shape[1], K)[2]
    assert (splits == 1) == (name == "batch70")
    what = f"{name} K = {K}"
    out, r = run(pts, lengths, K), ref(name, K)
    check_values(out, r, True, what)
    check_normal_direction(out, r, what)  # on the CPU reference the gap filter leaves out <= 2.3 % in every case
    if name != "batch70":  # the spheres and the cow: 100 % of the reference's points are decisive
        check_signs(out, r, K, what)
    if name.startswith("sphere") and K >= 16:  # all neighbours lie on the inner side: the normals point inwards
        p = pts[0].double().numpy()
        inward = -(out["frames"][0, :, :, 0] * p).sum(1) / np.linalg.norm(p, axis=1)
        assert (inward >= 0.9).all(), (what, inward.min())


@pytest.mark.parametrize("name,K", [("sphere300", 16), ("cow", 33), ("batch70", 50)])
def test_frames_without_disambiguation(name, K):
    pts, lengths = cloud(name)
    out, r = run(pts, lengths, K, False), ref(name, K, False)
    check_values(out, r, False, f"{name} K = {K} undisambiguated")
    check_largest_positive(out, r, f"{name} K = {K}")


# --------------------------------------------------------------------------- path independence, determinism
@pytest.mark.parametrize("name,K", [("sphere300", 16), ("sphere300", 50), ("sphere1100", 16), ("sphere1100", 50)])
def test_result_does_not_depend_on_the_path(name, K):
    """The same cloud alone (split: a scan and a merge) and as member 137 of a batch of 256 (one launch; at 1,100
    points the scan crosses the 1,024-target LDS chunk): bitwise equal, and equal to a second run."""
    pts, _ = cloud(name)
    P = pts.shape[1]
    assert kernels.frames_geometry(1, P, K)[2] > 1 and kernels.frames_geometry(256, P, K)[2] == 1
    batch = torch.randn(256, P, 3, generator=torch.Generator().manual_seed(5))
    batch[137] = pts[0]
    for dis in (True, False):
        alone = kernels.point_frames(pts.to(DEV), None, K, dis, return_cov=True)
        again = kernels.point_frames(pts.to(DEV), None, K, dis, return_cov=True)
        many = kernels.point_frames(batch.to(DEV), None, K, dis, return_cov=True)
        for a, b, m in zip(alone, again, many):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
            assert torch.equal(a[0].view(torch.int32), m[137].view(torch.int32)), (name, K, dis)


# --------------------------------------------------------------------------- robustness
def test_translated_cloud_stays_within_the_bars():
    pts = cloud("sphere300")[0] + 100.0  # rounded to float32 here: the reference sees the same input
    out, r = run(pts, None, 16), NR.frames_ref(pts, None, 16)
    check_values(out, r, True, "sphere300 + 100")
    check_normal_direction(out, r, "sphere300 + 100")


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_rescaled_cloud_gives_the_same_frames(scale):
    base, lengths = cloud("cow")
    pts = base * scale
    out, r = run(pts, lengths, 16), NR.frames_ref(pts, lengths, 16)
    what = f"cow * {scale:g}"
    check_values(out, r, True, what)
    check_normal_direction(out, r, what)
    check_signs(out, r, 16, what)
    # curvatures scale by the square, frames not at all: against the unscaled reference
    r1 = ref("cow", 16)
    ok = r1["valid"]
    tr = r1["cur"][ok].sum(1)
    assert (np.abs(out["cur"][ok] / scale ** 2 - r1["cur"][ok]).max(1) <= 1e-4 * tr).all()
    gap = r1["cur"][ok][:, 1] - r1["cur"][ok][:, 0]
    keep = gap >= 0.02 * tr
    sin = np.linalg.norm(np.cross(out["frames"][ok][:, :, 0], r1["frames"][ok][:, :, 0]), axis=1)
    assert (sin[keep] * gap[keep] <= 2e-4 * tr[keep]).all()


def test_duplicated_and_collinear_clouds():
    g = torch.Generator().manual_seed(3)
    five = torch.randn(5, 3, generator=g)
    dup = five.repeat(8, 1)[None]  # 40 points: 5 distinct ones, 8 times each
    for dis in (True, False):
        out = run(dup, None, 8, dis)
        assert (out["cur"] == 0).all() and (out["cov"] == 0).all()
        V = out["frames"][0]
        assert np.isfinite(V).all() and np.abs(np.swapaxes(V, 1, 2) @ V - np.eye(3)).max() <= 1e-5
        assert (np.abs(V) == np.eye(3)).all()  # the identity up to the signs
    t = torch.linspace(-1.0, 1.0, 100)[:, None]
    line = (t * torch.tensor([[1.0, 2.0, 3.0]]) + 0.5)[None]
    out, r = run(line, None, 8), NR.frames_ref(line, None, 8)
    V = out["frames"][0]
    assert all(np.isfinite(out[k]).all() for k in out)
    assert np.abs(np.swapaxes(V, 1, 2) @ V - np.eye(3)).max() <= 1e-5
    tr = np.trace(r["cov"][0], axis1=1, axis2=2)
    assert (np.abs(out["cur"][0] - r["cur"][0]).max(1) <= 1e-4 * tr).all()
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    assert (np.abs(np.abs(V[:, :, 2] @ axis) - 1) <= 1e-5).all()  # the main direction is the line


# --------------------------------------------------------------------------- the public interface
def test_public_interface():
    pts, lengths = cloud("cow")
    K = 16
    cur, frm = kernels.point_frames(pts.to(DEV), lengths.to(DEV), K)
    pc = Pointclouds([pts[0].to(DEV), pts[1, :257].to(DEV)])
    c2, f2 = estimate_pointcloud_local_coord_frames(pc, neighborhood_size=K)
    assert c2.shape == (2, 733, 3) and f2.shape == (2, 733, 3, 3) and c2.dtype == torch.float32
    assert torch.equal(c2, cur) and torch.equal(f2, frm)
    assert torch.equal(estimate_pointcloud_normals(pc, K), frm[..., 0])
    # a tensor input: every cloud has P points; float64 in, float64 out (the coordinates are read as float32)
    one = pts[:1].to(DEV)
    c3, f3 = estimate_pointcloud_local_coord_frames(one, K, use_symeig_workaround=False)
    assert torch.equal(c3, cur[:1]) and torch.equal(f3, frm[:1])
    c4, f4 = estimate_pointcloud_local_coord_frames(one.double(), K)
    assert c4.dtype == f4.dtype == torch.float64 and torch.equal(c4, c3.double()) and torch.equal(f4, f3.double())
    n4 = estimate_pointcloud_normals(one.double(), K, False)
    assert n4.dtype == torch.float64 and n4.shape == (1, 733, 3)
    assert torch.equal(n4.float(), kernels.point_frames(one, None, K, False)[1][..., 0])
    # the default neighbourhood of 50 runs (the 64 bucket) and gives unit normals
    n50 = estimate_pointcloud_normals(one)
    assert torch.allclose(n50.norm(dim=-1), torch.ones(1, 733, device=DEV), atol=1e-5)
    # grad mode off: an input that requires grad is accepted
    with torch.no_grad():
        assert torch.equal(estimate_pointcloud_normals(one.clone().requires_grad_(True), K), f3[..., 0])
    with pytest.raises(NotImplementedError):
        estimate_pointcloud_normals(one.clone().requires_grad_(True), K)


@pytest.mark.parametrize("name,K", [("sphere300", 50), ("batch70", 16)])
def test_hip_graph_capture_replays_the_eager_call(name, K):
    pts = cloud(name)[0].to(DEV)

    def step():
        return estimate_pointcloud_local_coord_frames(pts, neighborhood_size=K)

    eager = step()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up on the side stream: workspace sizes cached, allocator primed
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for u, w in zip(eager, captured):
        assert torch.equal(u, w)
