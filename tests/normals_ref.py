"""Float64 restatement of estimate_pointcloud_local_coord_frames on the CPU: the yardstick of test_normals_cpu.py /
test_gpu_normals.py.

Per cloud, on the float32-rounded input: the neighbour sets come from ``knn_ref.sorted_dists`` (float32 distances in
the kernels' operation order, a STABLE sort: the lowest index among equal distances), which is what the kernel's
neighbourhood is defined as; everything after that is float64. d_k = p_k - p_i, m = mean d_k, C = mean (d_k - m)
(d_k - m)^T, ``numpy.linalg.eigh`` (ascending), then the sign step of the rule:

* disambiguate: columns 0 and 2 negated iff 2 #{k: v . d_k > 0} < K, column 1 = cross(column 0, column 2);
* otherwise every column's component of largest magnitude positive (the lowest axis among equal magnitudes).

C == 0 gives zero curvatures and the identity before the sign step. Rows past a length are zeros.
"""
import functools

import numpy as np
import torch

from tests.knn_ref import sorted_dists
from tests.points_ref import _lengths

TRIU = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # the order of the kernels' cov output


def sphere(P, seed=0, radius=1.0):
    """P points on a noise-free sphere (float32, (P,3)): normalised gaussians."""
    x = torch.randn(P, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return (radius * x / x.norm(dim=1, keepdim=True)).float()


@functools.lru_cache(maxsize=None)
def cow_clouds():
    """(points (2,733,3) float32, lengths [733, 257]): the cow asset's vertices with stride 4, and the first 257 of
    those with stride 11, zero padded."""
    from torch_renderer_amd.assets import load_asset_arrays

    v = torch.from_numpy(np.asarray(load_asset_arrays("cow")["verts"], dtype=np.float32))
    a, b = v[::4], v[::11][:257]
    pts = torch.zeros(2, a.shape[0], 3)
    pts[0], pts[1, :b.shape[0]] = a, b
    return pts, torch.tensor([a.shape[0], b.shape[0]])


def sign_by_largest(v):
    """Columns of v (..., 3, 3) signed so that their component of largest magnitude is positive (lowest axis on ties)."""
    big = np.argmax(np.abs(v), axis=-2)  # argmax takes the first among equals
    val = np.take_along_axis(v, big[..., None, :], axis=-2)
    return v * np.where(val < 0, -1.0, 1.0)


def frames_ref(points, lengths=None, K=50, disambiguate=True):
    """dict of float64 numpy arrays: cov (N,P,3,3), cur (N,P,3), frames (N,P,3,3), d (N,P,K,3) the neighbours minus
    the point, idx (N,P,K) int64, valid (N,P) bool."""
    p32 = points.detach().cpu().float()
    N, P = p32.shape[0], p32.shape[1]
    ls = _lengths(lengths, N, P)
    out = {"cov": np.zeros((N, P, 3, 3)), "cur": np.zeros((N, P, 3)), "frames": np.zeros((N, P, 3, 3)),
           "d": np.zeros((N, P, K, 3)), "idx": np.zeros((N, P, K), dtype=np.int64), "valid": np.zeros((N, P), dtype=bool)}
    for n in range(N):
        L = ls[n]
        if L < K:
            continue
        _, order = sorted_dists(p32[n, :L], p32[n, :L])
        idx = order[:, :K].numpy()
        p = p32[n, :L].double().numpy()
        d = p[idx] - p[:, None, :]
        e = d - d.mean(1, keepdims=True)
        cov = np.einsum("pki,pkj->pij", e, e) / K
        w, v = np.linalg.eigh(cov)
        zero = np.abs(cov).reshape(L, 9).max(1) == 0
        w[zero], v[zero] = 0.0, np.eye(3)
        if disambiguate:
            for col in (0, 2):
                proj = np.einsum("pki,pi->pk", d, v[:, :, col])
                flip = 2 * (proj > 0).sum(1) < K
                v[:, :, col] = np.where(flip[:, None], -v[:, :, col], v[:, :, col])
            v[:, :, 1] = np.cross(v[:, :, 0], v[:, :, 2])
        else:
            v = sign_by_largest(v)
        out["cov"][n, :L], out["cur"][n, :L], out["frames"][n, :L] = cov, w, v
        out["d"][n, :L], out["idx"][n, :L], out["valid"][n, :L] = d, idx, True
    return out


def cov6(cov):
    """(..., 3, 3) -> (..., 6) upper triangle in the kernels' order."""
    return np.stack([cov[..., i, j] for i, j in TRIU], -1)


def cov33(c6):
    """(..., 6) -> (..., 3, 3) symmetric."""
    c6 = np.asarray(c6, dtype=np.float64)
    out = np.zeros(c6.shape[:-1] + (3, 3))
    for a, (i, j) in enumerate(TRIU):
        out[..., i, j] = out[..., j, i] = c6[..., a]
    return out
