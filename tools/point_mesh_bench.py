"""point_mesh_face_distance (loss.point_mesh_face_distance, csrc/mr_pointmesh.hip) against the same loss composed from
torch ops on the same GPU (tests/point_mesh_ref.loss_composed: broadcast (P, T) pair distances -> min -> gather ->
autograd), forward alone and forward + backward, in microseconds per step; and beside them the step the exact
distance stands in for, sample_points_from_meshes + chamfer_distance against the same cloud.

    python tools/point_mesh_bench.py [--steps 200] [--windows 7] [--out profiles/point_mesh_bench.json]

Settings: (a) the fitting loops': ico_sphere(2) source (T = 320), 1,000 target points, N = 1; (b) the unit-normalised
cow (T = 5,856) against 5,000 and 20,000 points. Each at min_triangle_area 0 and 5e-3. One process; the versions
alternate window by window after a warm-up of all; every window ends in a device synchronise; the per-step median and
the min..max spread over the windows are reported. The forward-alone time also gives pair evaluations per second (2 P T
pairs per step, both directions), an end-to-end rate that includes the launches around the scan. If the composition
runs out of memory at a size, the point count is halved until it fits and the size that ran is recorded.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests.helpers import mesh_arrays  # noqa: E402
from tests.point_mesh_ref import loss_composed  # noqa: E402
from torch_renderer_amd import Meshes, Pointclouds  # noqa: E402
from torch_renderer_amd.loss import chamfer_distance, point_mesh_face_distance  # noqa: E402
from torch_renderer_amd.ops import sample_points_from_meshes  # noqa: E402
from torch_renderer_amd.utils import ico_sphere  # noqa: E402

DEV = "cuda:0"


def run(versions, windows, warmup=3):
    """versions: {name: (fn, steps per window)} -> {name: timing record}; the versions alternate window by window."""
    for fn, _ in versions.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in versions}
    for _ in range(windows):
        for k, (fn, n) in versions.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e6 / n)
    return {k: {"us_per_step_median": statistics.median(ts), "us_per_step_min": min(ts), "us_per_step_max": max(ts),
                "windows": len(ts), "steps_per_window": versions[k][1]} for k, ts in times.items()}


def bench_point(name, verts, faces, points, area, steps, windows):
    leaf = verts.clone().requires_grad_(True)
    fi = faces.to(DEV)
    pcl = Pointclouds([points])
    S = points.shape[0]

    def fused_fwd():
        with torch.no_grad():
            point_mesh_face_distance(Meshes([leaf], [fi]), pcl, area)

    def fused():
        leaf.grad = None
        point_mesh_face_distance(Meshes([leaf], [fi]), pcl, area).backward()

    def torch_fwd():
        with torch.no_grad():
            loss_composed(points, leaf, fi, area)

    def composed():
        leaf.grad = None
        loss_composed(points, leaf, fi, area).backward()

    def sample_chamfer():
        leaf.grad = None
        s = sample_points_from_meshes(Meshes([leaf], [fi]), S)
        chamfer_distance(points[None], s)[0].backward()

    P, T = points.shape[0], faces.shape[0]
    # the composition's steps per window shrink with the (P, T, 3) tensors it materialises
    slow = max(3, min(steps, int(steps * 3.2e5 / (P * T))))
    fused()
    g_fused, l_fused = leaf.grad.clone(), point_mesh_face_distance(Meshes([leaf], [fi]), pcl, area).item()
    torch.cuda.reset_peak_memory_stats()
    composed()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    l_torch = loss_composed(points, leaf.detach(), fi, area).item()
    rel = (g_fused - leaf.grad).abs().max().item() / max(leaf.grad.abs().max().item(), 1e-30)
    point = {"point": name, "P": P, "T": T, "V": verts.shape[0], "min_triangle_area": area, "loss_fused": l_fused,
             "loss_torch": l_torch, "grad_rel_diff_fused_vs_torch": rel, "torch_peak_bytes_allocated": peak}
    point.update(run({"fused_forward": (fused_fwd, steps), "fused": (fused, steps), "torch_forward": (torch_fwd, slow),
                      "torch": (composed, slow), "sample_chamfer": (sample_chamfer, steps)}, windows))
    point["torch_over_fused_forward"] = point["torch_forward"]["us_per_step_median"] / \
        point["fused_forward"]["us_per_step_median"]
    point["torch_over_fused"] = point["torch"]["us_per_step_median"] / point["fused"]["us_per_step_median"]
    point["fused_over_sample_chamfer"] = point["fused"]["us_per_step_median"] / \
        point["sample_chamfer"]["us_per_step_median"]
    point["pair_evaluations_per_forward"] = 2 * P * T
    point["pair_evaluations_per_second_end_to_end"] = 2 * P * T / (point["fused_forward"]["us_per_step_median"] * 1e-6)
    return point


def fitting(area, steps, windows):
    sph = ico_sphere(2)
    cow_v, cow_f, _ = mesh_arrays("cow")
    torch.manual_seed(0)
    target = sample_points_from_meshes(Meshes([cow_v.to(DEV)], [cow_f.to(DEV)]), 1000)[0].contiguous()
    return bench_point("ico_sphere(2) source, 1,000 points drawn once from the cow, N = 1",
                       sph.verts_list()[0].float().to(DEV), sph.faces_list()[0], target, area, steps, windows)


def cow(P, area, steps, windows):
    v, f, _ = mesh_arrays("cow")
    v = (v - v.mean(0)) / (v - v.mean(0)).abs().max()
    pts = (0.5 * torch.randn(P, 3, generator=torch.Generator().manual_seed(P))).to(DEV)
    while True:
        try:
            r = bench_point(f"unit-normalised cow, {pts.shape[0]} points, N = 1", v.to(DEV), f, pts, area,
                            max(steps // 4, 10), windows)
            r["points_asked"] = P
            return r
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            pts = pts[:pts.shape[0] // 2].contiguous()
            if pts.shape[0] < 500:
                raise


def below_share(area):
    from torch_renderer_amd.kernels import face_areas

    v, f, _ = mesh_arrays("cow")
    v = (v - v.mean(0)) / (v - v.mean(0)).abs().max()
    a = face_areas(v.to(DEV), f.to(DEV))
    return {"cow_faces_below_min_triangle_area": float((a < area).float().mean()), "cow_median_face_area": float(a.median())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_mesh_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("point_mesh_bench: needs the GPU (no CPU timing)")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "points": []}
    out.update(below_share(5e-3))
    for area in (0.0, 5e-3):
        for fn in (lambda: fitting(area, a.steps, a.windows), lambda: cow(5000, area, a.steps, a.windows),
                   lambda: cow(20000, area, a.steps, a.windows)):
            r = fn()
            out["points"].append(r)
            print(f"{r['point']} (area {area:g}): forward fused {r['fused_forward']['us_per_step_median']:.1f} us, torch "
                  f"{r['torch_forward']['us_per_step_median']:.1f} us ({r['torch_over_fused_forward']:.1f}x); forward + "
                  f"backward fused {r['fused']['us_per_step_median']:.1f} "
                  f"[{r['fused']['us_per_step_min']:.1f}..{r['fused']['us_per_step_max']:.1f}], torch "
                  f"{r['torch']['us_per_step_median']:.1f} [{r['torch']['us_per_step_min']:.1f}.."
                  f"{r['torch']['us_per_step_max']:.1f}] ({r['torch_over_fused']:.1f}x); sample + chamfer "
                  f"{r['sample_chamfer']['us_per_step_median']:.1f} us; "
                  f"{r['pair_evaluations_per_second_end_to_end']:.3e} pairs/s", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
