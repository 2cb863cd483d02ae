"""``pytorch3d.ops`` names: ``sample_points_from_meshes`` (mesh_deformer.py:299-352 and deform_mesh_from_pcd.py:
160-212 sample 1000 points of the target and of the deformed source every step).

The random draws are torch calls on the meshes' device — ``torch.multinomial`` over the padded per-mesh face areas
(with replacement) and ``torch.rand(2, N, S)`` — so ``torch.manual_seed`` reproduces a call. The face areas
(kernels.face_areas) and the construction of the points with its backward (kernels.SamplePoints) are native
(csrc/mr_points.hip).
"""
from __future__ import annotations

import weakref

import torch

from .kernels import SamplePoints, _require_cuda, face_areas

_FACES_CACHE: dict = {}


def _packed_faces(faces_list, Vs):
    """(faces int32 (F,3) over packed vertex ids, per-mesh face counts) of the meshes, checked once against their
    vertex counts on the host and cached on the identity and version of the faces tensors (a steady loop, whose
    Meshes.offset_verts result keeps the source's faces tensors, does no host work here)."""
    key = tuple(id(f) for f in faces_list) + tuple(Vs)
    hit = _FACES_CACHE.get(key)
    if hit is not None and all(r() is f and ver == f._version for r, ver, f in zip(hit[0], hit[1], faces_list)):
        return hit[2]
    out, off = [], 0
    for f, V in zip(faces_list, Vs):
        if f.numel() and (int(f.min()) < 0 or int(f.max()) >= V):
            raise ValueError("sample_points_from_meshes: faces index vertices outside the mesh")
        out.append(f.reshape(-1, 3).to(torch.int32) + off)
        off += V
    if off >= 2 ** 31 // 3:
        raise NotImplementedError("sample_points_from_meshes: the packed batch is too large for 32-bit vertex ids")
    res = (torch.cat(out, 0).contiguous(), [int(f.shape[0]) for f in faces_list])
    if len(_FACES_CACHE) > 64:
        _FACES_CACHE.clear()
    _FACES_CACHE[key] = ([weakref.ref(f) for f in faces_list], [f._version for f in faces_list], res)
    return res


def sample_points_from_meshes(meshes, num_samples: int = 10000, return_normals: bool = False,
                              return_textures: bool = False):
    """pytorch3d.ops.sample_points_from_meshes: (N, num_samples, 3) points drawn uniformly from the surface of each
    mesh (a face in proportion to its area, then uniformly inside it); zeros for a mesh without faces.
    Differentiable w.r.t. the meshes' vertex tensors; a ``Meshes.extend(N)`` batch draws independently per copy and
    its shared vertices take the summed gradient once. Normals and textures are not built."""
    if return_normals or return_textures:
        raise NotImplementedError("sample_points_from_meshes: return_normals / return_textures are not built")
    if meshes.isempty():
        raise ValueError("Meshes are empty.")
    N, S = len(meshes), int(num_samples)
    if meshes.is_shared():  # one copy of the vertices: every mesh of the batch indexes it
        verts = meshes.shared_verts()
        faces, counts = _packed_faces([meshes.shared_faces()], (verts.shape[0],))
        counts, first = counts * N, [0] * N
    else:
        vl = meshes.verts_list()
        verts = torch.cat(vl, 0)
        faces, counts = _packed_faces(meshes.faces_list(), tuple(v.shape[0] for v in vl))
        first = [sum(counts[:i]) for i in range(N)]
    _require_cuda(verts, faces)
    dev = verts.device
    with torch.no_grad():
        areas = face_areas(verts, faces)
        if meshes.is_shared():
            face_idx = torch.multinomial(areas.view(1, -1).expand(N, -1), S, replacement=True)
        elif all(c == counts[0] for c in counts):
            face_idx = torch.multinomial(areas.view(N, -1), S, replacement=True) + \
                torch.tensor(first, device=dev).view(N, 1)
        else:  # padded areas of the meshes that have faces; the others keep the id -1 (rows of zeros)
            valid = [i for i, c in enumerate(counts) if c > 0]
            padded = torch.zeros((len(valid), max(counts)), device=dev)
            for r, i in enumerate(valid):
                padded[r, :counts[i]] = areas[first[i]:first[i] + counts[i]]
            drawn = torch.multinomial(padded, S, replacement=True) + \
                torch.tensor([first[i] for i in valid], device=dev).view(-1, 1)
            if len(valid) == N:
                face_idx = drawn
            else:
                face_idx = torch.full((N, S), -1, dtype=torch.int64, device=dev)
                face_idx[torch.tensor(valid, device=dev)] = drawn
        uv = torch.rand(2, N, S, device=dev)
    return SamplePoints.apply(verts, faces, face_idx, uv)
