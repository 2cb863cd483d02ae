"""The ICP loops with ``Y`` as points (the brute-force scan k_icp_nn) against ``Y`` as a PointGrid (k_icp_nn_grid, a ring
walk through a uniform grid of the targets), both estimators, in one process on one GPU.

    python tools/icp_grid_bench.py [--reps 3] [--windows 7] [--out profiles/icp_grid_bench.json]

Three versions of every call: ``points`` (kernels.icp / kernels.icp_plane as they were), ``grid`` (the same call with a
grid built once outside the timed region) and ``build_and_grid`` (kernels.point_grid_build inside it). Before anything
is timed the histories of the two routes are asserted equal, bit for bit. The versions alternate window by window after
a warm-up of each; every window ends in a device synchronise; the median and the min..max spread over the windows are
reported, with the iterations run, the microseconds per iteration, the kernel launches per iteration (torch.profiler)
and, for the grid, the distances evaluated per source point and iteration (the ``visited`` counter).

Shapes: the registration batch of tools/icp_bench.py (300 x 2,000 -> 100-400); the 1 x 20,000 -> 20,000 surface pair
of tools/icp_plane_bench.py; the same pair at 200,000 -> 200,000, where the points route is capped at a
``max_iterations`` that keeps a window under a second and the grid route runs at that cap and at 100 (where the
capped run shows that the points route's window at 100 stays under a second too, it is timed there as well), with the
distances a source point evaluates in a few single iterations; and, for the plane estimator, the 20,000 pair with the
target cut by a half-space, with and without max_correspondence_distance.
No threshold: the claims are judged from the spread and written into the JSON.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.icp_bench import count_launches, interleaved, registration_data, summary  # noqa: E402
from tools.icp_plane_bench import NORMALS_K, surface_pair  # noqa: E402
from torch_renderer_amd import Pointclouds, kernels  # noqa: E402
from torch_renderer_amd.ops import SimilarityTransform, estimate_pointcloud_normals  # noqa: E402

DEV = "cuda:0"
PLANE_THR = 1e-4   # tools/icp_plane_bench.py says why the plane estimator is not run at 1e-6
BIG_CAP = 20       # max_iterations of the points route at 200,000 x 200,000


def _equal(a, b):
    return a[0] == b[0] and a[1] == b[1] and all(
        torch.equal(u.view(torch.int32), w.view(torch.int32)) for u, w in zip(a[2:], b[2:]))


def bench_point(label, plane, X, Y, lengths, init, reps, windows, max_iterations=100, max_dist=None, normals=None,
                time_points=True):
    """One estimator on one shape. ``time_points=False`` times only the two grid versions (the brute-force route would
    take minutes) and skips the equality assertion, which a capped run of the same shape has made."""
    pl = None if lengths is None else lengths.to(DEV)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    init_d = None if init is None else SimilarityTransform(*(t.to(DEV) for t in init))
    queries = X.shape[0] * X.shape[1]
    if plane:
        thr = PLANE_THR

        def call(grid=None, visited=None):
            return kernels.icp_plane(Xd, Yd, normals, None, pl, init_d, max_iterations, thr, max_dist, grid=grid,
                                     visited=visited)
    else:
        thr = 1e-6

        def call(grid=None, visited=None):
            return kernels.icp(Xd, Yd, None, pl, init_d, max_iterations, thr, 0, grid=grid, visited=visited)

    built = kernels.point_grid_build(Yd, pl)
    visited = torch.zeros(1, dtype=torch.int64, device=DEV)
    g = call(built, visited)
    iters = int(g[1])
    out = {"point": label, "estimator": "point_to_plane" if plane else "point_to_point", "clouds": X.shape[0],
           "source_points": X.shape[1], "target_points_padded": Y.shape[1],
           "target_lengths": None if lengths is None else [int(lengths.min()), int(lengths.max())],
           "max_iterations": max_iterations, "relative_rmse_thr": thr, "max_correspondence_distance": max_dist,
           "iterations": iters, "converged": bool(g[0]),
           "grid_distances_per_query_and_iteration": visited.item() / (max(iters, 1) * queries),
           "points_distances_per_query_and_iteration": float(Y.shape[1] if lengths is None else lengths.float().mean())}
    versions = {"grid": lambda: call(built), "build_and_grid": lambda: call(kernels.point_grid_build(Yd, pl))}
    if time_points:
        p = call()
        assert _equal(p, g), f"{label}: the grid route's history differs from the points route's"
        out["histories_equal"] = True
        versions = {"points": call, **versions}
    times = interleaved(versions, reps, windows)
    for k, fn in versions.items():
        out[k] = summary(times[k])
        out[k].update(us_per_iteration_median=1e3 * out[k]["ms_median"] / max(iters, 1),
                      us_per_iteration_min=1e3 * out[k]["ms_min"] / max(iters, 1),
                      us_per_iteration_max=1e3 * out[k]["ms_max"] / max(iters, 1))
        n, err = count_launches(fn)
        out[k]["kernel_launches"] = n
        out[k]["kernel_launches_per_iteration"] = None if n is None else n / max(iters, 1)
        if err:
            out[k]["launch_count_error"] = err
    if time_points:
        out["points_over_grid"] = out["points"]["ms_median"] / out["grid"]["ms_median"]
        out["points_over_build_and_grid"] = out["points"]["ms_median"] / out["build_and_grid"]["ms_median"]
        # faster by more than the window-to-window spread: the slowest grid window against the fastest points one
        out["grid_faster_beyond_spread"] = out["grid"]["ms_max"] < out["points"]["ms_min"]
        out["build_and_grid_faster_beyond_spread"] = out["build_and_grid"]["ms_max"] < out["points"]["ms_min"]
        out["points_faster_beyond_spread"] = out["points"]["ms_max"] < out["grid"]["ms_min"]
    return out


def _call(plane, X, Y, lengths, init, normals, max_iterations, visited=None):
    """The grid route of one estimator, on a grid built for the call."""
    pl = None if lengths is None else lengths.to(DEV)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    init_d = None if init is None else SimilarityTransform(*(t.to(DEV) for t in init))
    grid = kernels.point_grid_build(Yd, pl)
    if plane:
        return kernels.icp_plane(Xd, Yd, normals, None, pl, init_d, max_iterations, PLANE_THR, None, grid=grid,
                                 visited=visited)
    return kernels.icp(Xd, Yd, None, pl, init_d, max_iterations, 1e-6, 0, grid=grid, visited=visited)


def call_iterations(plane, X, Y, lengths, init, normals, max_iterations=100):
    return _call(plane, X, Y, lengths, init, normals, max_iterations)[1]


def visited_profile(label, plane, X, Y, lengths, init, normals, last):
    """The distances a source point evaluates in iteration i, for a few i: the ``visited`` counter of the runs capped at
    i and at i - 1 iterations. It shows where the walk is dear: far from alignment a source point lies rings away from
    the surface the targets sample."""
    queries = X.shape[0] * X.shape[1]

    def total(k):
        if k == 0:
            return 0
        visited = torch.zeros(1, dtype=torch.int64, device=DEV)
        _call(plane, X, Y, lengths, init, normals, k, visited)
        return visited.item()

    picks = sorted({i for i in (1, 2, 3, 5, 10, 20, last) if 1 <= i <= last})
    return {"point": label + ", distances per query in iteration i (grid route)",
            "estimator": "point_to_plane" if plane else "point_to_point",
            "profile": {str(i): (total(i) - total(i - 1)) / queries for i in picks}}


def _normals(Y, lengths):
    Yd = Y.to(DEV)
    target = Yd if lengths is None else Pointclouds([Yd[i, :int(n)] for i, n in enumerate(lengths)])
    return estimate_pointcloud_normals(target, NORMALS_K).contiguous()  # once, outside the timed region


def _line(r):
    ks = [k for k in ("points", "grid", "build_and_grid") if isinstance(r.get(k), dict)]
    return (f"{r['point']} [{r['estimator']}]: {r['iterations']} iterations; " + "; ".join(
        f"{k} {r[k]['ms_median']:.3f} ms [{r[k]['ms_min']:.3f}..{r[k]['ms_max']:.3f}] "
        f"({r[k]['us_per_iteration_median']:.1f} us an iteration, {r[k]['kernel_launches_per_iteration']} launches)"
        for k in ks) + f"; {r['grid_distances_per_query_and_iteration']:.1f} distances per query and iteration")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--clouds", type=int, default=300)
    ap.add_argument("--mid", type=int, default=20000)
    ap.add_argument("--big", type=int, default=200000)
    ap.add_argument("--max-dist", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_grid_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("icp_grid_bench: needs the GPU (no CPU timing)")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "status_batch": kernels.ICP_STATUS_BATCH, "points": []}

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def add(r):
        out["points"].append(r)
        print(_line(r), flush=True)
        with open(a.out, "w") as fh:  # after every point: a run that is cut short leaves what it measured
            json.dump(out, fh, indent=1)
        return r

    reg = registration_data(a.clouds)
    reg_n = _normals(reg[1], reg[2])
    mid = surface_pair(a.mid)
    mid_n = _normals(mid[1], None)
    big = surface_pair(a.big)
    big_n = _normals(big[1], None)
    for plane, rn, mn, bn in ((False, None, None, None), (True, reg_n, mid_n, big_n)):
        r = add(bench_point(f"registration batch {a.clouds} x 2000 -> 100-400", plane, *reg, a.reps, a.windows, normals=rn))
        out.setdefault("claim_3_registration_batch_grid_loses_or_ties", []).append(not r["grid_faster_beyond_spread"])
        r = add(bench_point(f"1 x {a.mid} -> {a.mid} surface pair", plane, *mid, a.reps, a.windows, normals=mn))
        out.setdefault("claim_2_prebuilt_grid_faster_at_mid", []).append(r["grid_faster_beyond_spread"])
        r = add(bench_point(f"1 x {a.big} -> {a.big} surface pair, max_iterations {BIG_CAP}", plane, *big, 1, a.windows,
                            max_iterations=BIG_CAP, normals=bn))
        out.setdefault("claim_1_build_and_grid_faster_at_big_capped", []).append(r["build_and_grid_faster_beyond_spread"])
        # at 100 the points route is timed too where its window stays under a second, judged from the capped run's
        # time per iteration (the scan's cost does not depend on the iteration) and the iterations the grid route runs
        full_iters = int(call_iterations(plane, *big, bn))
        fits = r["points"]["us_per_iteration_median"] * full_iters < 1e6
        r = add(bench_point(f"1 x {a.big} -> {a.big} surface pair, max_iterations 100", plane, *big, 1, a.windows,
                            normals=bn, time_points=fits))
        r["points_window_under_a_second"] = fits
        if fits:
            out.setdefault("claim_1_build_and_grid_faster_at_big_run_to_the_end", []).append(
                r["build_and_grid_faster_beyond_spread"])
        out["points"].append(visited_profile(f"1 x {a.big} -> {a.big} surface pair", plane, *big, bn, full_iters))
        print(json.dumps(out["points"][-1]), flush=True)
    # the plane estimator on a cut scan: the target loses the half-space x > its median, the source keeps every point
    X, Y, _, init = mid
    cut = Y[:, Y[0, :, 0] <= Y[0, :, 0].median()].contiguous()
    cut_n = _normals(cut, None)
    for d in (None, a.max_dist):
        add(bench_point(f"1 x {a.mid} -> {cut.shape[1]} cut scan, max_correspondence_distance {d}", True, X, cut, None,
                        init, a.reps, a.windows, max_dist=d, normals=cut_n))
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
