"""knn_points through a PointGrid (csrc/mr_grid.hip) against the brute-force knn_points (csrc/mr_knn.hip, the call
without grid=), forward only, in microseconds per call.

    python tools/knn_grid_bench.py [--windows 7] [--out profiles/knn_grid_bench.json]

Shapes: 1 x 20,000 x 20,000 at K = 8, 1 x 200,000 x 200,000 at K = 8 and 1 x 1,000,000 x 1,000,000 at K = 1, uniform
in the unit cube; 300 x 2,000 x 400 at K = 4 (the ICP scripts' batch, where the grid is expected to lose); 20,000
samples of the cow's surface against themselves at K = 16. Four versions per shape: the brute-force call, the grid's
build alone, the search alone over a grid built before, and build + search. Every shape runs in a child process of its
own under a time limit; the run stops at the first child that fails. Inside a child the versions alternate window by
window after a warm-up of all, every window ends in a device synchronise, and the per-call median and the min..max
spread over the windows are reported, with each version's kernel launches per call (torch.profiler), the distances the
search evaluates per query (the kernel's counter), the grid's dims, and how many neighbour indices differ between the
two searches (it must be 0).
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

# (label, N, P1, P2, K, calls per window of the brute-force call, of the grid versions, seconds allowed)
POINTS = [("unit cube", 1, 20000, 20000, 8, 20, 50, 240), ("unit cube", 1, 200000, 200000, 8, 2, 20, 300),
          ("unit cube", 1, 1000000, 1000000, 1, 1, 10, 420), ("unit cube", 300, 2000, 400, 4, 50, 50, 240),
          ("cow surface against itself", 1, 20000, 20000, 16, 20, 50, 240)]
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


def count_launches(step):
    import torch

    try:
        from torch.profiler import ProfilerActivity, profile

        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")
                 and not e.name.lower().startswith(("memcpy", "memset"))]
        return len(names), None
    except Exception as ex:  # the count is a record, not a condition
        return None, repr(ex)[:200]


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
    out = {}
    for k, ts in times.items():
        n, err = count_launches(versions[k][0])
        out[k] = {"us_per_call_median": statistics.median(ts), "us_per_call_min": min(ts), "us_per_call_max": max(ts),
                  "windows": len(ts), "calls_per_window": versions[k][1], "kernel_launches_per_call": n}
        if err:
            out[k]["launch_count_error"] = err
    return out


def bench_point(i, windows):
    import torch

    from torch_renderer_amd import kernels

    label, N, P1, P2, K, nb, ng, _ = POINTS[i]
    g = torch.Generator().manual_seed(i)
    if label.startswith("cow"):
        p2 = cow_surface(P2, seed=i).to(DEV)
        p1 = p2
    else:
        p1, p2 = torch.rand(N, P1, 3, generator=g).to(DEV), torch.rand(N, P2, 3, generator=g).to(DEV)
    point = {"point": f"{N} x {P1} x {P2}, K = {K}, {label}", "N": N, "P1": P1, "P2": P2, "K": K,
             "brute_force_distance_evaluations_per_query": P2}

    grid = kernels.point_grid_build(p2)
    dims, cell, most = kernels.point_grid_describe(grid, N, P2)
    point["grid"] = {"dims_of_cloud_0": dims[0].tolist(), "cell_size_of_cloud_0": cell[0, 3].item(),
                     "largest_cell_of_any_cloud": int(most.max()), "bytes": grid.numel()}
    visited = torch.zeros(1, dtype=torch.int64, device=DEV)
    dg, ig = kernels.knn_points_grid(p1, p2, grid, K=K, visited=visited)
    db, ib = kernels.knn_points(p1, p2, K=K)
    point["neighbours"] = {"indices": ib.numel(), "differ": int((ig != ib).sum()),
                           "distances_that_differ": int((dg.view(torch.int32) != db.view(torch.int32)).sum())}
    point["distance_evaluations_per_query"] = visited.item() / (N * P1)

    def brute():
        kernels.knn_points(p1, p2, K=K)

    def build():
        kernels.point_grid_build(p2)

    def search():
        kernels.knn_points_grid(p1, p2, grid, K=K)

    def build_search():
        kernels.knn_points_grid(p1, p2, kernels.point_grid_build(p2), K=K)

    r = run({"brute_force": (brute, nb), "build": (build, ng), "search": (search, ng),
             "build_search": (build_search, ng)}, windows)
    for k in ("search", "build_search"):
        r[k]["brute_force_over_this"] = r["brute_force"]["us_per_call_median"] / r[k]["us_per_call_median"]
        # the claim's test: this version's median below the brute-force call's fastest window
        r[k]["median_below_the_brute_force_minimum"] = r[k]["us_per_call_median"] < r["brute_force"]["us_per_call_min"]
        r[k]["max_below_the_brute_force_minimum"] = r[k]["us_per_call_max"] < r["brute_force"]["us_per_call_min"]
    point["forward"] = r
    return point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_grid_bench.json"))
    ap.add_argument("--point", type=int, default=None, help="run one shape in this process and print its JSON")
    a = ap.parse_args()
    if a.point is not None:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("knn_grid_bench: needs the GPU (no CPU timing)")
        r = bench_point(a.point, a.windows)
        r["device"], r["torch_version"] = torch.cuda.get_device_name(0), torch.__version__
        print("KNN_GRID_BENCH_POINT " + json.dumps(r), flush=True)
        return
    out = {"points": []}
    rows = []
    for i, p in enumerate(POINTS):  # a fresh child per shape, each under its own time limit
        cmd = ["timeout", "-k", "10", str(p[7]), sys.executable, os.path.abspath(__file__), "--point", str(i),
               "--windows", str(a.windows)]
        res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [l for l in res.stdout.splitlines() if l.startswith("KNN_GRID_BENCH_POINT ")]
        if res.returncode != 0 or not lines:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"knn_grid_bench: shape {i} ended with status {res.returncode}; nothing further is started")
        r = json.loads(lines[-1][len("KNN_GRID_BENCH_POINT "):])
        out["device"], out["torch"] = r.pop("device"), r.pop("torch_version")
        out["points"].append(r)
        f = r["forward"]

        def cell(k):
            v = f[k]
            return f"{v['us_per_call_median']:,.0f} [{v['us_per_call_min']:,.0f}..{v['us_per_call_max']:,.0f}]"

        rows.append(f"| {r['point']} | {cell('brute_force')} | {cell('build')} | {cell('search')} | "
                    f"{cell('build_search')} | {f['build_search']['brute_force_over_this']:.2f}x | "
                    f"{r['distance_evaluations_per_query']:.0f} of {r['P2']} | "
                    f"{f['brute_force']['kernel_launches_per_call']} / {f['build']['kernel_launches_per_call']} / "
                    f"{f['search']['kernel_launches_per_call']} | {r['neighbours']['differ']} |")
        print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("| Shape | brute force, us | build | search | build + search | brute / (build + search) | distances per query "
          "| launches: brute / build / search | indices that differ |")
    print("|---|---|---|---|---|---|---|---|---|")
    print("\n".join(rows))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
