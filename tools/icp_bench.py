"""The registration scripts' ICP (pytorch3d_icp_registeration.py:154-185) — ops.iterative_closest_point, whose loop runs
on the device (csrc/mr_points.hip, k_icp_*) — against the same algorithm composed from torch ops on the same GPU
(tests/icp_ref.icp_composed: cdist -> argmin -> gather -> torch.linalg.svd, with upstream's convergence test and its
host read every iteration), in milliseconds per registration of the whole batch.

    python tools/icp_bench.py [--reps 3] [--windows 7] [--out profiles/icp_bench.json]

Points: 300 clouds of 2,000 source points sampled from the cow, 100-400 target points each (the moved source, a
random subset cut by a half space, 1e-4 noise), the true translation plus 0.05 noise as init_transform,
max_iterations = 100: once with the targets' lengths, and once as the reference calls it, on the zero-padded target
tensor without lengths. One process; the versions alternate window by window after a warm-up of each; every window
ends in a device synchronise; the median and the min..max spread over the windows are reported, with the iterations
run, each version's kernel launches per iteration (torch.profiler) and the library's time for every size of the
batch of iterations it enqueues between two reads of the device status (kernels.ICP_STATUS_BATCH is the default).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests.helpers import mesh_arrays  # noqa: E402
from tests.icp_ref import icp_composed, rotations  # noqa: E402
from torch_renderer_amd import kernels  # noqa: E402
from torch_renderer_amd.ops import SimilarityTransform, iterative_closest_point  # noqa: E402

DEV = "cuda:0"
BATCHES = (1, 2, 4, 8, 16, 32, 100)


def registration_data(N=300, P1=2000, seed=0):
    """(X (N,P1,3), Y (N,P2,3) zero padded, y_lengths, init) on the CPU. Every cloud is moved by its own rotation
    (three axis rotations of up to pi/4 composed) and an in-plane shift of 0.5 N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    verts, _, _ = mesh_arrays("cow")
    X = torch.stack([verts[torch.randint(0, verts.shape[0], (P1,), generator=g)] for _ in range(N)])
    R = torch.eye(3, dtype=torch.float64)[None].repeat(N, 1, 1)
    for axis in range(3):
        a = torch.zeros(N, 3)
        a[:, axis] = 1.0
        R = torch.bmm(R, rotations(a, torch.rand(N, generator=g) * math.pi / 4))
    T = 0.5 * torch.randn(N, 3, generator=g)
    T[:, 2] = 0.0
    moved = torch.bmm(X, R.float()) + T[:, None]
    clouds = []
    for n in range(N):
        k = int(torch.randint(200, 800, (1,), generator=g))
        t = moved[n, torch.randint(0, P1, (k,), generator=g)] + 1e-4 * torch.randn(k, 3, generator=g)
        clouds.append(t[t[:, 0] > t[:, 0].mean()])
    lengths = torch.tensor([c.shape[0] for c in clouds])
    Y = torch.zeros(N, int(lengths.max()), 3)
    for n, c in enumerate(clouds):
        Y[n, :c.shape[0]] = c
    init = SimilarityTransform(torch.eye(3)[None].repeat(N, 1, 1), T + 0.05 * torch.randn(N, 3, generator=g),
                               torch.ones(N))
    return X, Y, lengths, init


def count_launches(step):
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


def interleaved(versions, reps, windows, warmup=2):
    """{name: [ms per call, one entry a window]}: the versions alternate window by window."""
    for fn in versions.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in versions}
    for _ in range(windows):
        for k, fn in versions.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / reps)
    return times


def summary(ts):
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "windows": len(ts)}


def bench_point(label, X, Y, lengths, init, reps, windows, max_iterations=100):
    pl = None if lengths is None else lengths.to(DEV)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    init_d = SimilarityTransform(*(t.to(DEV) for t in init))

    def fused(batch=None):
        return kernels.icp(Xd, Yd, None, pl, init_d, max_iterations, 1e-6, 0, status_batch=batch)

    def composed():
        return icp_composed(Xd, Yd, pl, init_d, max_iterations, 1e-6)

    f, c = fused(), composed()
    point = {"point": label, "clouds": X.shape[0], "source_points": X.shape[1], "target_points_padded": Y.shape[1],
             "target_lengths": None if lengths is None else [int(lengths.min()), int(lengths.max())],
             "max_iterations": max_iterations,
             "iterations": {"fused": f[1], "torch": c[4]}, "converged": {"fused": f[0], "torch": c[0]},
             "rmse_max_abs_diff_fused_vs_torch": (f[2] - c[1]).abs().max().item(), "rmse_max": c[1].max().item()}
    times = interleaved({"fused": fused, "torch": composed}, reps, windows)
    for k, fn, iters in (("fused", fused, f[1]), ("torch", composed, c[4])):
        point[k] = summary(times[k])
        n, err = count_launches(fn)
        point[k]["kernel_launches"] = n
        point[k]["kernel_launches_per_iteration"] = None if n is None else n / max(iters, 1)
        if err:
            point[k]["launch_count_error"] = err
    point["torch_over_fused"] = point["torch"]["ms_median"] / point["fused"]["ms_median"]
    # faster by more than the run-to-run spread: the slowest fused window against the fastest composed one
    point["fused_faster_beyond_spread"] = point["fused"]["ms_max"] < point["torch"]["ms_min"]
    bt = interleaved({b: (lambda b=b: fused(b)) for b in BATCHES}, reps, windows)
    point["status_batch"] = {str(b): summary(bt[b]) for b in BATCHES}
    point["status_batch_fastest"] = min(BATCHES, key=lambda b: statistics.median(bt[b]))
    return point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--clouds", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("icp_bench: needs the GPU (no CPU timing)")
    X, Y, lengths, init = registration_data(a.clouds)
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "status_batch_default": kernels.ICP_STATUS_BATCH, "status_batches_tried": list(BATCHES), "points": []}
    for label, l in (("targets with lengths", lengths), ("the reference's call: zero-padded targets, no lengths", None)):
        r = bench_point(label, X, Y, l, init, a.reps, a.windows)
        out["points"].append(r)
        print(f"{label}: fused {r['fused']['ms_median']:.2f} ms [{r['fused']['ms_min']:.2f}..{r['fused']['ms_max']:.2f}] "
              f"in {r['iterations']['fused']} iterations, torch {r['torch']['ms_median']:.2f} ms "
              f"[{r['torch']['ms_min']:.2f}..{r['torch']['ms_max']:.2f}] in {r['iterations']['torch']}, torch/fused "
              f"{r['torch_over_fused']:.1f}x, launches per iteration {r['fused']['kernel_launches_per_iteration']} vs "
              f"{r['torch']['kernel_launches_per_iteration']}; status batch "
              + ", ".join(f"{b}: {v['ms_median']:.2f}" for b, v in r["status_batch"].items()), flush=True)
    out["fused_faster_beyond_spread_at_every_point"] = all(p["fused_faster_beyond_spread"] for p in out["points"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
