"""Cloud-to-mesh ICP — ops.iterative_closest_point_to_mesh, whose loop runs on the device (csrc/mr_icpmesh.hip) —
against (2) the same estimator composed from torch ops on the same GPU (tests/icp_mesh_ref.icp_mesh_composed, which
materialises (clouds, points, faces, 3) tensors and therefore runs on the first --composed-clouds clouds only) and (3)
what a caller could do before: sample_points_from_meshes + estimate_pointcloud_normals +
iterative_closest_point_to_plane, the scan registered onto the samples. Milliseconds per registration of the batch.

    python tools/icp_mesh_bench.py [--reps 3] [--windows 7] [--out profiles/icp_mesh_bench.json]

The model is the unit cow (T = 5,856): the cow asset centred on its bounding box and scaled to a largest extent of 1.
Data (a), the registration batch made against it: 300 scans, each 200-800 area-weighted surface
samples with 1e-4 noise, moved by three axis rotations of up to 45 degrees each and an in-plane shift of 0.5 N(0,1), cut
by a half space through the scan's mean; the start is the true translation undone to 0.05 N(0,1), no rotation.
Data (b): one full scan of 20,000 samples moved by 10 degrees about (1, 2, 3) and a 0.05 shift, started from the
identity. max_iterations = 100, relative_rmse_thr = 1e-4 (tests/icp_mesh_ref.THR). One process; the routes alternate
window by window after a warm-up of each; every window ends in a device synchronise; the median and the min..max spread
over the windows are reported, with the iterations run, the kernel launches per iteration and each kernel's device
time (torch.profiler), and the pose error against the known truth: the rotation angle between the estimate and the
truth and the distance between the translations, per cloud. One point -> face scan of the same shape is measured with
kernels.point_face_nearest (whose single launch runs both directions: it cannot be asked for direction 0 alone, so it
is shown beside the time of the loop's own scan kernel). No threshold: the claims are judged from the measured values
and written into the JSON.
"""
import argparse
import json
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests.helpers import mesh_arrays  # noqa: E402
from tests.icp_mesh_ref import THR, icp_mesh_composed, pose_error, surface_samples  # noqa: E402
from tests.icp_ref import RTs, rotations  # noqa: E402
from tools.icp_bench import count_launches, interleaved, summary  # noqa: E402
from torch_renderer_amd import Meshes, Pointclouds, kernels  # noqa: E402
from torch_renderer_amd.ops import (SimilarityTransform, estimate_pointcloud_normals,  # noqa: E402
                                    iterative_closest_point_to_mesh, iterative_closest_point_to_plane,
                                    sample_points_from_meshes)

DEV = "cuda:0"
NORMALS_K = 16
SAMPLES = 5000   # route 3's samples of the model


def unit_cow():
    """(verts (2930,3) float32, faces (5856,3)): the cow centred on its bounding box, its largest extent scaled to 1."""
    verts, faces, _ = mesh_arrays("cow")
    lo, hi = verts.min(0).values, verts.max(0).values
    return ((verts.double() - (lo + hi).double() / 2) / float((hi - lo).max())).float(), faces


def registration_scans(verts, faces, N=300, seed=0):
    """(X (N,P,3) zero padded, lengths, init, truth) on the CPU: scan n is x = p R_n + T_n of its surface samples p,
    so the truth taking the scan back onto the mesh is R' = R^T, T' = -(T R^T)."""
    g = torch.Generator().manual_seed(seed)
    R = torch.eye(3, dtype=torch.float64)[None].repeat(N, 1, 1)
    for axis in range(3):
        a = torch.zeros(N, 3)
        a[:, axis] = 1.0
        R = torch.bmm(R, rotations(a, torch.rand(N, generator=g) * math.pi / 4))
    T = 0.5 * torch.randn(N, 3, generator=g, dtype=torch.float64)
    T[:, 2] = 0.0
    clouds = []
    for n in range(N):
        k = int(torch.randint(200, 800, (1,), generator=g))
        p = surface_samples(verts, faces, k, g) + 1e-4 * torch.randn(k, 3, generator=g, dtype=torch.float64)
        x = p @ R[n] + T[n]
        clouds.append(x[x[:, 0] > x[:, 0].mean()].float())
    lengths = torch.tensor([c.shape[0] for c in clouds])
    X = torch.zeros(N, int(lengths.max()), 3)
    for n, c in enumerate(clouds):
        X[n, :c.shape[0]] = c
    Rt = R.transpose(1, 2)
    truth = RTs(Rt.float(), (-torch.bmm(T[:, None], Rt)[:, 0]).float(), torch.ones(N))
    # translation-only start: p ~ x - T, the true shift known to 0.05
    init = SimilarityTransform(torch.eye(3)[None].repeat(N, 1, 1), (-T + 0.05 * torch.randn(N, 3, generator=g)).float(),
                               torch.ones(N))
    return X, lengths, init, truth


def full_scan(verts, faces, P=20000, seed=1):
    g = torch.Generator().manual_seed(seed)
    p = surface_samples(verts, faces, P, g) + 1e-4 * torch.randn(P, 3, generator=g, dtype=torch.float64)
    R = rotations(torch.tensor([[1.0, 2.0, 3.0]]), torch.tensor([math.radians(10.0)]))
    T = torch.tensor([[0.03, -0.03, 0.03]], dtype=torch.float64)
    X = (p @ R[0] + T[0]).float()[None]
    Rt = R.transpose(1, 2)
    truth = RTs(Rt.float(), (-torch.bmm(T[:, None], Rt)[:, 0]).float(), torch.ones(1))
    return X, None, SimilarityTransform(torch.eye(3)[None], torch.zeros(1, 3), torch.ones(1)), truth


def kernel_times(step):
    """{kernel name: [launches, total device microseconds]} of one call, from torch.profiler; None with the reason
    where the profiler does not give them (a record, not a condition)."""
    try:
        from torch.profiler import ProfilerActivity, profile

        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        out = {}
        for e in prof.events():
            if str(e.device_type).endswith("CUDA") and not e.name.lower().startswith(("memcpy", "memset")):
                m = re.search(r"\bk_\w+", e.name)  # the library's kernels; anything else under its own name
                name = m.group(0) if m else e.name[:48]
                rec = out.setdefault(name, [0, 0.0])
                rec[0] += 1
                rec[1] += float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0) or 0.0)
        return out, None
    except Exception as ex:
        return None, repr(ex)[:200]


def pose(R, T, truth):
    ang, shift = pose_error(R, T, truth)
    return {"rotation_error_deg_median": ang.median().item(), "rotation_error_deg_max": ang.max().item(),
            "translation_error_median": shift.median().item(), "translation_error_max": shift.max().item(),
            "clouds_within_1_degree": int((ang < 1.0).sum()), "clouds": int(ang.numel())}


def bench_point(label, verts, faces, X, lengths, init, truth, reps, windows, composed_clouds, composed_iterations,
                max_iterations=100, thr=THR):
    N, P = X.shape[:2]
    vd, fd = verts.to(DEV), faces.to(DEV)
    Xd = X.to(DEV)
    ld = None if lengths is None else lengths.to(DEV)
    init_d = SimilarityTransform(*(t.to(DEV) for t in init))
    model = Meshes([vd], [fd])
    meshes = model.extend(N) if N > 1 else model
    scans = Xd if lengths is None else Pointclouds([Xd[i, :int(n)] for i, n in enumerate(lengths)])
    # route 3's target: samples of the model and their estimated normals, once, outside the timed region
    torch.manual_seed(0)
    Yd = sample_points_from_meshes(meshes, SAMPLES).detach()
    Nd = estimate_pointcloud_normals(Yd, NORMALS_K).contiguous()
    nc = min(N, composed_clouds)

    def mesh_call():
        return iterative_closest_point_to_mesh(scans, meshes, init_d, max_iterations, thr)

    def composed():
        # full clouds only: the first nc clouds, each cut to the shortest of them
        k = P if lengths is None else int(lengths[:nc].min())
        return icp_mesh_composed(Xd[:nc, :k], vd, fd, tuple(t[:nc] for t in init_d), composed_iterations, thr)

    def today():
        return iterative_closest_point_to_plane(scans, Yd, Nd, init_d, max_iterations, thr)

    out = {"point": label, "clouds": N, "scan_points_padded": P, "faces": int(faces.shape[0]),
           "scan_lengths": None if lengths is None else [int(lengths.min()), int(lengths.max())],
           "max_iterations": max_iterations, "relative_rmse_thr": thr, "model_samples_of_route_3": SAMPLES,
           "normals_neighborhood": NORMALS_K}
    m, c, t = mesh_call(), composed(), today()
    times = interleaved({"mesh": mesh_call, "today_sampled_plane": today}, reps, windows)
    ctimes = interleaved({"mesh_torch": composed}, 1, max(2, windows // 2), warmup=1)
    runs = {"mesh": (m.converged, len(m.t_history), m.RTs.R, m.RTs.T, truth, mesh_call),
            "today_sampled_plane": (t.converged, len(t.t_history), t.RTs.R, t.RTs.T, truth, today),
            "mesh_torch": (c[0], c[4], c[3][0], c[3][1], RTs(*(v[:nc] for v in truth)), composed)}
    for k, (conv, iters, R, T, tr, fn) in runs.items():
        out[k] = summary(times[k] if k in times else ctimes[k])
        out[k].update(iterations=int(iters), converged=bool(conv),
                      ms_per_iteration_median=out[k]["ms_median"] / max(int(iters), 1), pose=pose(R, T, tr))
        n, err = count_launches(fn)
        out[k]["kernel_launches"] = n
        out[k]["kernel_launches_per_iteration"] = None if n is None else n / max(int(iters), 1)
        if err:
            out[k]["launch_count_error"] = err
    out["mesh_torch"].update(clouds=nc, points_per_cloud=int(P if lengths is None else lengths[:nc].min()),
                             max_iterations=composed_iterations,
                             note="the composed estimator materialises (clouds, points, faces, 3) tensors: it runs on a "
                                  "part of the batch, full clouds only, with its own iteration cap; compare per iteration "
                                  "and per cloud")
    for k, sol, call in (("mesh", m, iterative_closest_point_to_mesh), ("today_sampled_plane", t, None)):
        if sol.converged or len(sol.t_history) < 2:
            continue  # stopped by the cap: how many clouds were still above the threshold in the last iteration
        n1 = len(sol.t_history) - 1
        before = (iterative_closest_point_to_mesh(scans, meshes, init_d, n1, thr) if call else
                  iterative_closest_point_to_plane(scans, Yd, Nd, init_d, n1, thr))
        rel = (before.rmse - sol.rmse) / before.rmse
        out[k]["clouds_above_threshold_in_last_iteration"] = int((~(rel <= thr)).sum())
        out[k]["largest_relative_drop_in_last_iteration"] = rel.abs().max().item()
    kt, err = kernel_times(mesh_call)
    out["mesh"]["kernel_device_us"] = kt
    if err:
        out["mesh"]["kernel_time_error"] = err
    # one point -> face scan of the same shape: point_face_nearest (both directions in its one launch), and the loop's
    # own scan plus closest points (mesh_closest_points)
    lens = [P] * N if lengths is None else lengths.tolist()
    packed = torch.cat([Xd[i, :lens[i]] for i in range(N)])
    first = torch.tensor([0] + lens[:-1]).cumsum(0).to(DEV)
    count = torch.tensor(lens).to(DEV)
    T_ = int(faces.shape[0])
    fi = faces.to(torch.int32).to(DEV)
    ff, fc = torch.zeros(N, dtype=torch.int64, device=DEV), torch.full((N,), T_, dtype=torch.int64, device=DEV)
    batch = kernels.PointMeshBatch(None, ld, P, fi, ff, fc, T_)
    rts0 = torch.cat([init_d.R.reshape(N, 9), init_d.T, init_d.s[:, None]], 1).contiguous()

    def pfn():
        return kernels.point_face_nearest(packed, first, count, vd, fi, ff, fc, 0.0, max(lens), T_)

    def closest():
        return kernels.mesh_closest_points(Xd, vd, batch, rts0, 0.0)

    st = interleaved({"point_face_nearest_both_directions": pfn, "mesh_closest_points": closest}, reps, windows)
    out["scan"] = {k: summary(v) for k, v in st.items()}
    it = out["mesh"]["ms_per_iteration_median"]
    out["iteration_over_point_face_nearest"] = it / out["scan"]["point_face_nearest_both_directions"]["ms_median"]
    out["iteration_over_mesh_closest_points"] = it / out["scan"]["mesh_closest_points"]["ms_median"]
    if kt:
        scan_us = sum(v[1] for k, v in kt.items() if "icpm_scan" in k)
        all_us = sum(v[1] for v in kt.values())
        out["mesh"]["scan_share_of_device_time"] = scan_us / all_us if all_us else None
    out["per_cloud_per_iteration_us"] = {
        "mesh": 1e3 * it / N, "mesh_torch": 1e3 * out["mesh_torch"]["ms_per_iteration_median"] / nc,
        "today_sampled_plane": 1e3 * out["today_sampled_plane"]["ms_per_iteration_median"] / N}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--clouds", type=int, default=300)
    ap.add_argument("--big", type=int, default=20000)
    ap.add_argument("--composed-clouds", type=int, default=16)
    ap.add_argument("--composed-iterations", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_mesh_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("icp_mesh_bench: needs the GPU (no CPU timing)")
    verts, faces = unit_cow()
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "library": kernels._lib.LIB_PATH
           if not os.environ.get("MI355R_LIB") else os.path.basename(os.environ["MI355R_LIB"]),
           "status_batch": kernels.ICP_STATUS_BATCH, "points": []}
    out["library"] = os.path.basename(out["library"])
    points = ((f"registration batch: {a.clouds} cut scans against the cow", registration_scans(verts, faces, a.clouds)),
              (f"one full scan of {a.big} points against the cow", full_scan(verts, faces, a.big)))
    for label, data in points:
        r = bench_point(label, verts, faces, *data, a.reps, a.windows, a.composed_clouds,
                        a.composed_iterations if data[1] is not None else 4)
        out["points"].append(r)
        print(f"{label}: " + "; ".join(
            f"{k} {r[k]['ms_median']:.2f} ms [{r[k]['ms_min']:.2f}..{r[k]['ms_max']:.2f}] in {r[k]['iterations']} "
            f"iterations (converged {r[k]['converged']}, {r[k]['kernel_launches_per_iteration']} launches each), rotation "
            f"error median {r[k]['pose']['rotation_error_deg_median']:.3f} max {r[k]['pose']['rotation_error_deg_max']:.3f} "
            f"deg, translation error max {r[k]['pose']['translation_error_max']:.2e}"
            for k in ("mesh", "mesh_torch", "today_sampled_plane"))
            + f"; scans {json.dumps(r['scan'])}; iteration / point_face_nearest "
            f"{r['iteration_over_point_face_nearest']:.2f}, / mesh_closest_points "
            f"{r['iteration_over_mesh_closest_points']:.2f}", flush=True)
    reg = out["points"][0]
    out["claims"] = {
        "converges_on_the_registration_batch_where_cloud_to_cloud_hits_the_cap":
            bool(reg["mesh"]["converged"] and not reg["today_sampled_plane"]["converged"]),
        "mesh_converged": [p["mesh"]["converged"] for p in out["points"]],
        "today_converged": [p["today_sampled_plane"]["converged"] for p in out["points"]],
        # about one scan: within 25 % of the loop's own scan + closest points, judged on the medians
        "an_iteration_costs_about_one_scan": all(p["iteration_over_mesh_closest_points"] <= 1.25 for p in out["points"]),
        "iteration_over_point_face_nearest": [p["iteration_over_point_face_nearest"] for p in out["points"]],
        "iteration_over_mesh_closest_points": [p["iteration_over_mesh_closest_points"] for p in out["points"]]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out["claims"]))


if __name__ == "__main__":
    main()
