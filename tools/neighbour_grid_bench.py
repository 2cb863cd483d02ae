"""estimate_pointcloud_normals and ball_query through a PointGrid (k_frames_grid of csrc/mr_normals.hip,
k_ball_query_grid of csrc/mr_ballquery.hip) against the same calls without a grid, and what the plane ICP's
``Y_normals=None`` costs before and after, in microseconds per call.

    python tools/neighbour_grid_bench.py [--windows 7] [--out profiles/neighbour_grid_bench.json]

Shapes: normals at 1 x 20,000 (unit cube and samples of the cow's surface) and 1 x 200,000 with K = 16 and K = 50, and
at 300 x 2,000 with K = 16 (where the grid is expected to lose); ball_query at 20,000 against itself with K = 16 and
radius 0.06 and 0.005, at 200,000 against itself with radius 0.02, and at 32 x 512 x 4,096 with K = 32 and radius 0.2;
iterative_closest_point_to_plane(scan, grid, None, neighborhood_size=16) at 1 x 200,000 -> 200,000. Four versions per
shape: the call without a grid (the baseline: that code is the parent's), the grid's build alone, the call over a grid
built before, and build + call. Every shape runs in a child process of its own under a time limit; the run stops at the
first child that fails. Inside a child the results are first compared bitwise (anything but 0 differences ends the
child), then the versions alternate window by window after a warm-up of all, every window ends in a device
synchronise, and the per-call median and the min..max spread over the windows are reported, with the distances the
search evaluates per query (the kernel's counter) and the grid's dims.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (call, label, N, P1, P2, K, radius, calls per window of the baseline, of the grid versions, seconds allowed)
POINTS = [("normals", "unit cube", 1, 20000, 20000, 16, None, 20, 50, 240),
          ("normals", "unit cube", 1, 20000, 20000, 50, None, 5, 20, 240),
          ("normals", "cow surface", 1, 20000, 20000, 16, None, 20, 50, 240),
          ("normals", "cow surface", 1, 20000, 20000, 50, None, 5, 20, 240),
          ("normals", "unit cube", 1, 200000, 200000, 16, None, 2, 20, 300),
          ("normals", "unit cube", 1, 200000, 200000, 50, None, 1, 10, 420),
          ("normals", "unit cube", 300, 2000, 2000, 16, None, 5, 5, 300),
          ("ball_query", "unit cube against itself", 1, 20000, 20000, 16, 0.06, 20, 50, 240),
          ("ball_query", "unit cube against itself", 1, 20000, 20000, 16, 0.005, 20, 50, 240),
          ("ball_query", "unit cube against itself", 1, 200000, 200000, 16, 0.02, 2, 20, 300),
          ("ball_query", "unit cube", 32, 512, 4096, 32, 0.2, 50, 50, 240),
          ("plane_icp", "unit sphere scan, rotated 0.05 rad", 1, 200000, 200000, 16, None, 1, 2, 420)]
DEV = "cuda:0"


def cow_surface(P, seed):
    """(1,P,3): samples of the cow's surface, a face in proportion to its area and uniform inside it."""
    import torch

    from tests.helpers import mesh_arrays

    g = torch.Generator().manual_seed(seed)
    verts, faces, _ = mesh_arrays("cow")
    a, b, c = (verts[faces[:, k]] for k in range(3))
    areas = 0.5 * torch.cross(b - a, c - a, dim=1).norm(dim=1)
    fi = torch.multinomial(areas, P, replacement=True, generator=g)
    u, v = torch.rand(P, generator=g), torch.rand(P, generator=g)
    s = u.sqrt()
    return ((1 - s)[:, None] * a[fi] + (s * (1 - v))[:, None] * b[fi] + (s * v)[:, None] * c[fi])[None]


def run(versions, windows, warmup=2):
    import torch

    for fn, _ in versions.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in versions}
    for _ in range(windows):
        for k, (fn, n) in versions.items():  # alternate the versions window by window
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e6 / n)
    return {k: {"us_per_call_median": statistics.median(ts), "us_per_call_min": min(ts), "us_per_call_max": max(ts),
                "windows": len(ts), "calls_per_window": versions[k][1]} for k, ts in times.items()}


def differ(a, b):
    import torch

    return int(sum((x.view(torch.int32) != y.view(torch.int32)).sum() for x, y in zip(a, b)))


def against_brute(r, keys):
    for k in keys:
        r[k]["brute_force_over_this"] = r["brute_force"]["us_per_call_median"] / r[k]["us_per_call_median"]
        # the claim's test: this version's slowest window below the brute-force call's fastest
        r[k]["max_below_the_brute_force_minimum"] = r[k]["us_per_call_max"] < r["brute_force"]["us_per_call_min"]
        r[k]["min_above_the_brute_force_maximum"] = r[k]["us_per_call_min"] > r["brute_force"]["us_per_call_max"]


def bench_point(i, windows):
    import torch

    from torch_renderer_amd import kernels, ops

    call, label, N, P1, P2, K, radius, nb, ng, _ = POINTS[i]
    g = torch.Generator().manual_seed(i)
    point = {"call": call, "N": N, "P1": P1, "P2": P2, "K": K, "brute_force_distance_evaluations_per_query": P2}
    visited = torch.zeros(1, dtype=torch.int64, device=DEV)

    def describe(grid):
        dims, cell, most = kernels.point_grid_describe(grid, N, P2)
        point["grid"] = {"dims_of_cloud_0": dims[0].tolist(), "cell_size_of_cloud_0": cell[0, 3].item(),
                         "largest_cell_of_any_cloud": int(most.max()), "bytes": grid.numel()}

    if call == "normals":
        pts = (cow_surface(P2, seed=i) if label.startswith("cow") else torch.rand(N, P2, 3, generator=g)).to(DEV)
        point["point"] = f"normals, {N} x {P2}, K = {K}, {label}"
        grid = kernels.point_grid_build(pts)
        describe(grid)
        a = kernels.point_frames(pts, None, K, return_cov=True)
        b = kernels.point_frames(pts, None, K, return_cov=True, grid=grid, visited=visited)
        point["values_that_differ"] = differ(a, b)
        versions = {"brute_force": (lambda: kernels.point_frames(pts, None, K), nb),
                    "build": (lambda: kernels.point_grid_build(pts), ng),
                    "search": (lambda: kernels.point_frames(pts, None, K, grid=grid), ng),
                    "build_search": (lambda: kernels.point_frames(pts, None, K, grid=kernels.point_grid_build(pts)), ng)}
    elif call == "ball_query":
        p2 = torch.rand(N, P2, 3, generator=g).to(DEV)
        p1 = p2 if "itself" in label else torch.rand(N, P1, 3, generator=g).to(DEV)
        point["point"] = f"ball_query, {N} x {P1} x {P2}, K = {K}, radius {radius}, {label}"
        point["radius"] = radius
        grid = kernels.point_grid_build(p2)
        describe(grid)
        a = kernels.ball_query(p1, p2, K=K, radius=radius)
        b = kernels.ball_query_grid(p1, p2, grid, K=K, radius=radius, visited=visited)
        point["values_that_differ"] = differ(a, b)
        point["hits_per_query_kept"] = float((a[1] >= 0).sum()) / (N * P1)
        versions = {"brute_force": (lambda: kernels.ball_query(p1, p2, K=K, radius=radius), nb),
                    "build": (lambda: kernels.point_grid_build(p2), ng),
                    "search": (lambda: kernels.ball_query_grid(p1, p2, grid, K=K, radius=radius), ng),
                    "build_search": (lambda: kernels.ball_query_grid(p1, p2, kernels.point_grid_build(p2), K=K,
                                                                     radius=radius), ng)}
    else:
        y = torch.randn(N, P2, 3, generator=g)
        y = (y / y.norm(dim=-1, keepdim=True)).to(DEV)
        c, s = torch.cos(torch.tensor(0.05)).item(), torch.sin(torch.tensor(0.05)).item()
        R = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], device=DEV)
        x = (y[:, torch.randperm(P2, generator=g)[:P1].to(DEV)] @ R + 0.01).contiguous()
        point["point"] = f"iterative_closest_point_to_plane(scan, grid, None, neighborhood_size={K}), {N} x {P1} -> {P2}, {label}"
        pg = ops.PointGrid(y)
        describe(pg.buffer)
        normals = ops.estimate_pointcloud_normals(y, K)
        through = ops.estimate_pointcloud_normals(pg, K)
        kernels.point_frames(y, None, K, grid=pg.buffer, visited=visited)
        want = ops.iterative_closest_point_to_plane(x, pg, normals)
        got = ops.iterative_closest_point_to_plane(x, pg, None, neighborhood_size=K)
        point["values_that_differ"] = differ((normals, want.rmse, want.Xt, *want.RTs), (through, got.rmse, got.Xt, *got.RTs))
        point["iterations"], point["converged"] = len(got.t_history), bool(got.converged)
        # brute_force: the call as it was (the brute-force normals, then the loop through the grid); build_search: the
        # call as it is, on a grid built before as the call takes it; build / search: the normals' share alone
        versions = {"brute_force": (lambda: ops.iterative_closest_point_to_plane(
                        x, pg, ops.estimate_pointcloud_normals(y, K)), nb),
                    "loop_with_given_normals": (lambda: ops.iterative_closest_point_to_plane(x, pg, normals), ng),
                    "normals_brute_force": (lambda: ops.estimate_pointcloud_normals(y, K), nb),
                    "search": (lambda: ops.estimate_pointcloud_normals(pg, K), ng),
                    "build": (lambda: kernels.point_grid_build(y), ng),
                    "build_search": (lambda: ops.iterative_closest_point_to_plane(x, pg, None, neighborhood_size=K), ng)}
    torch.cuda.synchronize()
    if point["values_that_differ"] != 0:
        raise SystemExit(f"neighbour_grid_bench: {point['point']}: {point['values_that_differ']} values differ")
    point["distance_evaluations_per_query"] = visited.item() / (N * P1 if call == "ball_query" else N * P2)
    r = run(versions, windows)
    against_brute(r, ("search", "build_search"))
    if call == "plane_icp":
        for k, share_of in (("normals_brute_force", "brute_force"), ("search", "build_search")):
            r[k]["share_of_the_call"] = r[k]["us_per_call_median"] / r[share_of]["us_per_call_median"]
    point["forward"] = r
    return point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbour_grid_bench.json"))
    ap.add_argument("--point", type=int, default=None, help="run one shape in this process and print its JSON")
    ap.add_argument("--only", type=int, nargs="*", default=None, help="the shapes to run (default: all)")
    a = ap.parse_args()
    if a.point is not None:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("neighbour_grid_bench: needs the GPU (no CPU timing)")
        r = bench_point(a.point, a.windows)
        r["device"], r["torch_version"] = torch.cuda.get_device_name(0), torch.__version__
        print("NEIGHBOUR_GRID_BENCH_POINT " + json.dumps(r), flush=True)
        return
    out = {"points": []}
    rows = []
    for i, p in enumerate(POINTS):  # a fresh child per shape, each under its own time limit
        if a.only is not None and i not in a.only:
            continue
        cmd = ["timeout", "-k", "10", str(p[9]), sys.executable, os.path.abspath(__file__), "--point", str(i),
               "--windows", str(a.windows)]
        res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [l for l in res.stdout.splitlines() if l.startswith("NEIGHBOUR_GRID_BENCH_POINT ")]
        if res.returncode != 0 or not lines:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"neighbour_grid_bench: shape {i} ended with status {res.returncode}; nothing further is "
                             "started")
        r = json.loads(lines[-1][len("NEIGHBOUR_GRID_BENCH_POINT "):])
        out["device"], out["torch"] = r.pop("device"), r.pop("torch_version")
        out["points"].append(r)
        f = r["forward"]

        def cell(k):
            v = f[k]
            return f"{v['us_per_call_median']:,.0f} [{v['us_per_call_min']:,.0f}..{v['us_per_call_max']:,.0f}]"

        rows.append(f"| {r['point']} | {cell('brute_force')} | {cell('build')} | {cell('search')} | "
                    f"{cell('build_search')} | {f['build_search']['brute_force_over_this']:.2f}x | "
                    f"{r['distance_evaluations_per_query']:.0f} of {r['P2']} | {r['values_that_differ']} |")
        if r["call"] == "plane_icp":
            rows.append(f"| the normals' share of that call | {cell('normals_brute_force')} = "
                        f"{100 * f['normals_brute_force']['share_of_the_call']:.1f} % | | {cell('search')} = "
                        f"{100 * f['search']['share_of_the_call']:.1f} % | loop alone "
                        f"{cell('loop_with_given_normals')} | | | |")
        print(rows[-1], flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:  # after every shape: a later child's failure keeps what was measured
            json.dump(out, fh, indent=1)
    print("| Shape | brute force, us | build | search | build + search | brute / (build + search) | distances per query "
          "| values that differ |")
    print("|---|---|---|---|---|---|---|---|")
    print("\n".join(rows))


if __name__ == "__main__":
    main()
