"""Plain-torch restatement of the three mesh shape priors (PyTorch3D's mesh_edge_loss, mesh_laplacian_smoothing
(method="uniform") and mesh_normal_consistency), the yardstick of test_mesh_priors_cpu.py / test_gpu_mesh_priors.py
and the baseline tools/prior_bench.py times on the device. Independent of the package's topology builder: the
topology here comes from a brute-force Python loop over the faces.

N = meshes in the batch; every loss is sum(weight * term) / N with weight = 1 / (the element's mesh's count of
that element):

* edge: per unique undirected edge (v0, v1): (|v0 - v1| - target_length)^2
* Laplacian: per vertex i, |Lv_i| with Lv_i = mean of its neighbours - v_i (-v_i for an isolated vertex)
* normal consistency: per unique edge (e0, e1) and unordered pair of faces containing it, with opposite vertices
  a, b: 1 - n0.n1 / (max(|n0|, 1e-8) max(|n1|, 1e-8)), n0 = (e1 - e0) x (a - e0), n1 = -(e1 - e0) x (b - e0)
"""
import torch


def brute_topology(faces_list, Vs):
    """Brute-force topology of a batch over packed vertex ids, every list in the order the package documents:
    edges sorted by min * V + max; each vertex's neighbours ascending; pairs (e0, e1, a, b) sorted by edge, then
    by the position of a's and b's faces among the faces on that edge (face order, then corner order); each
    vertex's (pair, role) entries 4 * pair + role ascending. Returns a dict of int64 tensors and float64 weights."""
    N = len(faces_list)
    Vt = int(sum(Vs))
    on_edge = {}  # (min, max) -> [(face, corner, opposite vertex)]
    vmesh, off = [], 0
    fid = 0
    for m, (f, V) in enumerate(zip(faces_list, Vs)):
        vmesh += [m] * int(V)
        for tri in f.tolist():
            t = [x + off for x in tri]
            for corner, (i, j, k) in enumerate(((1, 2, 0), (2, 0, 1), (0, 1, 2))):  # edge (t_i, t_j), opposite t_k
                key = (min(t[i], t[j]), max(t[i], t[j]))
                on_edge.setdefault(key, []).append((fid, corner, t[k]))
            fid += 1
        off += int(V)
    edges = sorted(on_edge, key=lambda e: e[0] * max(Vt, 1) + e[1])
    nbrs = [[] for _ in range(Vt)]
    for a, b in edges:
        nbrs[a].append(b)
        nbrs[b].append(a)
    nbrs = [sorted(n) for n in nbrs]
    pairs = []
    for e in edges:
        inc = sorted(on_edge[e])
        for i in range(len(inc)):
            for j in range(i + 1, len(inc)):
                pairs.append((e[0], e[1], inc[i][2], inc[j][2]))
    roles = [[] for _ in range(Vt)]
    for p, q in enumerate(pairs):
        for r, v in enumerate(q):
            roles[v].append(4 * p + r)
    e_per, p_per = [0] * N, [0] * N
    for a, _ in edges:
        e_per[vmesh[a]] += 1
    for q in pairs:
        p_per[vmesh[q[0]]] += 1

    def csr(lists):
        ptr = [0]
        for x in lists:
            ptr.append(ptr[-1] + len(x))
        return torch.tensor(ptr, dtype=torch.int64), torch.tensor([y for x in lists for y in x], dtype=torch.int64)

    nbr_ptr, nbr = csr(nbrs)
    pair_ptr, pair_idx = csr(roles)
    vm = torch.tensor(vmesh, dtype=torch.int64)
    e = torch.tensor(edges, dtype=torch.int64).reshape(-1, 2)
    p = torch.tensor(pairs, dtype=torch.int64).reshape(-1, 4)
    Vs_t = torch.tensor([int(v) for v in Vs], dtype=torch.float64)
    return {
        "N": N, "V": Vt, "edges": e, "pairs": p, "nbr_ptr": nbr_ptr, "nbr": nbr, "pair_ptr": pair_ptr,
        "pair_idx": pair_idx, "vert_mesh_idx": vm, "edge_mesh_idx": vm[e[:, 0]],
        "num_edges_per_mesh": torch.tensor(e_per, dtype=torch.int64),
        "num_pairs_per_mesh": torch.tensor(p_per, dtype=torch.int64),
        # gather lists of the Laplacian: row nbr_src[k] takes vertex nbr[k]
        "nbr_src": torch.repeat_interleave(torch.arange(Vt), nbr_ptr[1:] - nbr_ptr[:-1]),
        "deg": (nbr_ptr[1:] - nbr_ptr[:-1]),
        "edge_w": 1.0 / torch.tensor(e_per, dtype=torch.float64)[vm[e[:, 0]]],
        "vert_w": 1.0 / Vs_t[vm],
        "pair_w": 1.0 / torch.tensor(p_per, dtype=torch.float64)[vm[p[:, 0]]],
    }


def topology_to(topo, device, dtype):
    """The tensors of brute_topology on `device`, the weights in `dtype`."""
    out = {}
    for k, v in topo.items():
        if torch.is_tensor(v):
            v = v.to(device=device, dtype=dtype) if v.is_floating_point() else v.to(device)
        out[k] = v
    return out


def priors_from_topology(vp, topo, target_length=0.0):
    """(edge, laplacian, normal) losses (0-dim, dtype of vp) of packed vertices vp (V,3) from torch ops."""
    N = topo["N"]
    e, p = topo["edges"], topo["pairs"]
    d = vp[e[:, 0]] - vp[e[:, 1]]
    edge = (((d.norm(dim=1) - target_length) ** 2) * topo["edge_w"]).sum() / N
    s = torch.zeros_like(vp).index_add(0, topo["nbr_src"], vp[topo["nbr"]])
    lv = s / topo["deg"].clamp(min=1).to(vp.dtype)[:, None] - vp
    lap = (lv.norm(dim=1) * topo["vert_w"]).sum() / N
    v0 = vp[p[:, 0]]
    dd, pa, pb = vp[p[:, 1]] - v0, vp[p[:, 2]] - v0, vp[p[:, 3]] - v0
    n0 = torch.cross(dd, pa, dim=1)
    n1 = -torch.cross(dd, pb, dim=1)
    cos = (n0 * n1).sum(1) / (n0.norm(dim=1).clamp(min=1e-8) * n1.norm(dim=1).clamp(min=1e-8))
    normal = ((1.0 - cos) * topo["pair_w"]).sum() / N
    return edge, lap, normal


def priors_ref(verts_list, faces_list, target_length=0.0, dtype=torch.float32, topo=None):
    """Losses and their gradients on the CPU in `dtype`: ((edge, lap, normal) values, [three gradients w.r.t. the
    packed vertices (V,3)])."""
    if topo is None:
        topo = brute_topology(faces_list, [v.shape[0] for v in verts_list])
    topo = topology_to(topo, "cpu", dtype)
    vp = torch.cat([v.detach().cpu().to(dtype) for v in verts_list], 0).requires_grad_(True)
    losses = priors_from_topology(vp, topo, target_length)
    grads = []
    for loss in losses:
        g, = torch.autograd.grad(loss, vp, retain_graph=True, allow_unused=True)
        grads.append(torch.zeros_like(vp) if g is None else g)
    return tuple(x.detach() for x in losses), grads


def fan_mesh():
    """Three faces on edge (0, 1) plus an isolated vertex: 6 vertices, E = 7, P = 3."""
    verts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.4, 0.9, 0.1], [0.5, -0.8, 0.3], [0.6, 0.2, 0.9],
                          [2.0, 1.0, -0.5]])
    faces = torch.tensor([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=torch.int64)
    return verts, faces


def tetrahedron(a=1.0):
    """Regular tetrahedron of edge length a (float64 vertices): edge loss a^2, Laplacian a sqrt(6) / 3, normal
    consistency 4/3."""
    s = a / (2.0 * 2.0 ** 0.5)
    verts = torch.tensor([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]],
                         dtype=torch.float64) * s
    faces = torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=torch.int64)
    return verts, faces
