"""knn_points (ops.knn_points, csrc/mr_knn.hip) against the same result composed from torch ops on the same GPU
(cdist -> topk(largest=False) -> gather, which materialises the (N, P1, P2) matrix), forward and forward + backward, in
microseconds per step.

    python tools/knn_bench.py [--windows 7] [--out profiles/knn_bench.json]

Shapes: 1 x 20,000 x 20,000 at K = 8; 300 x 2,000 x 400 at K = 4 (the ICP scripts' batch); 1 x 1,000 x 1,000 at
K = 16; and K = 1 at the first shape, beside kernels.nearest_points on the same clouds (which searches BOTH directions,
x -> y and y -> x: twice the distance evaluations of the K = 1 scan). Every shape runs in a child process of its own
under a time limit; the run stops at the first child that fails. Inside a child the two versions alternate window by
window after a warm-up of both, every window ends in a device synchronise, and the per-step median and the min..max
spread over the windows are reported, with each version's kernel launches per step (torch.profiler), the launch
geometry (kernels.knn_geometry), and how many neighbour indices differ between the composition and the kernels
(cdist takes its matmul form, which rounds differently on near-ties).
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

# (N, P1, P2, K, steps per window of the kernels, of the composition, seconds allowed)
POINTS = [(1, 20000, 20000, 8, 20, 5, 240), (300, 2000, 400, 4, 50, 10, 240), (1, 1000, 1000, 16, 200, 200, 180),
          (1, 20000, 20000, 1, 20, 5, 240)]
DEV = "cuda:0"


def composed(p1, p2, K):
    """(dists, idx) of knn_points from torch ops: the search carries no gradient, the gather does."""
    import torch

    with torch.no_grad():
        idx = torch.cdist(p1, p2).topk(K, dim=2, largest=False).indices
    nn = p2[:, :, None].expand(-1, -1, K, -1).gather(1, idx[..., None].expand(-1, -1, -1, 3))
    return ((p1[:, :, None] - nn) ** 2).sum(-1), idx


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


def run(versions, windows, warmup=3):
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
        out[k] = {"us_per_step_median": statistics.median(ts), "us_per_step_min": min(ts), "us_per_step_max": max(ts),
                  "windows": len(ts), "steps_per_window": versions[k][1], "kernel_launches_per_step": n}
        if err:
            out[k]["launch_count_error"] = err
    return out


def bench_point(i, windows):
    import torch

    from torch_renderer_amd import kernels
    from torch_renderer_amd.ops import knn_points

    N, P1, P2, K, nk, nt, _ = POINTS[i]
    g = torch.Generator().manual_seed(i)
    p1 = torch.randn(N, P1, 3, generator=g).to(DEV).requires_grad_(True)
    p2 = torch.randn(N, P2, 3, generator=g).to(DEV).requires_grad_(True)
    a, b = p1.detach(), p2.detach()
    qpg, splits, chunk = kernels.knn_geometry(N, P1, P2, K)
    point = {"point": f"{N} x {P1} x {P2}, K = {K}", "N": N, "P1": P1, "P2": P2, "K": K,
             "geometry": {"queries_per_group": qpg, "splits": splits, "lds_chunk": chunk},
             "distance_evaluations": N * P1 * P2, "matrix_bytes_the_composition_materialises": 4 * N * P1 * P2}

    ik = knn_points(a, b, K=K).idx
    dt, it = composed(a, b, K)
    differ = ik != it
    point["neighbours"] = {"indices": ik.numel(), "differ": int(differ.sum()),
                           "queries_with_a_difference": int(differ.any(-1).sum())}

    def k_fwd():
        knn_points(a, b, K=K)

    def t_fwd():
        composed(a, b, K)

    def k_both():
        p1.grad = p2.grad = None
        knn_points(p1, p2, K=K).dists.sum().backward()

    def t_both():
        p1.grad = p2.grad = None
        composed(p1, p2, K)[0].sum().backward()

    k_both()
    gk = p1.grad.clone()
    t_both()
    point["grad_rel_diff_kernels_vs_torch"] = (gk - p1.grad).abs().max().item() / p1.grad.abs().max().item()
    for name, kf, tf in (("forward", k_fwd, t_fwd), ("forward_backward", k_both, t_both)):
        r = run({"kernels": (kf, nk), "torch": (tf, nt)}, windows)
        r["torch_over_kernels"] = r["torch"]["us_per_step_median"] / r["kernels"]["us_per_step_median"]
        point[name] = r
    point["forward"]["kernels"]["evaluations_per_second"] = \
        N * P1 * P2 / (point["forward"]["kernels"]["us_per_step_median"] * 1e-6)
    if K == 1:  # beside the K = 1 scan of nearest_points, which does both directions

        def nearest():
            kernels.nearest_points(a, b)

        r = run({"kernels": (k_fwd, nk), "nearest_points": (nearest, nk)}, windows)
        point["nearest_points_both_directions"] = r["nearest_points"]
        point["nearest_points_both_directions"]["distance_evaluations"] = 2 * N * P1 * P2
        point["knn_k1_one_direction"] = r["kernels"]
    return point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench.json"))
    ap.add_argument("--point", type=int, default=None, help="run one shape in this process and print its JSON")
    a = ap.parse_args()
    if a.point is not None:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("knn_bench: needs the GPU (no CPU timing)")
        r = bench_point(a.point, a.windows)
        r["device"], r["torch_version"] = torch.cuda.get_device_name(0), torch.__version__
        print("KNN_BENCH_POINT " + json.dumps(r), flush=True)
        return
    out = {"points": []}
    for i, p in enumerate(POINTS):  # a fresh child per shape, each under its own time limit
        cmd = ["timeout", "-k", "10", str(p[6]), sys.executable, os.path.abspath(__file__), "--point", str(i),
               "--windows", str(a.windows)]
        res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [l for l in res.stdout.splitlines() if l.startswith("KNN_BENCH_POINT ")]
        if res.returncode != 0 or not lines:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"knn_bench: shape {i} ended with status {res.returncode}; nothing further is started")
        r = json.loads(lines[-1][len("KNN_BENCH_POINT "):])
        out["device"], out["torch"] = r.pop("device"), r.pop("torch_version")
        out["points"].append(r)
        for name in ("forward", "forward_backward"):
            k, t = r[name]["kernels"], r[name]["torch"]
            print(f"{r['point']} {name}: kernels {k['us_per_step_median']:.1f} us/step [{k['us_per_step_min']:.1f}.."
                  f"{k['us_per_step_max']:.1f}], torch {t['us_per_step_median']:.1f} [{t['us_per_step_min']:.1f}.."
                  f"{t['us_per_step_max']:.1f}], torch/kernels {r[name]['torch_over_kernels']:.2f}x, launches "
                  f"{k['kernel_launches_per_step']} vs {t['kernel_launches_per_step']}", flush=True)
        if "nearest_points_both_directions" in r:
            print(f"{r['point']}: knn K = 1 (one direction) {r['knn_k1_one_direction']['us_per_step_median']:.1f} us, "
                  f"nearest_points (both directions) {r['nearest_points_both_directions']['us_per_step_median']:.1f} us",
                  flush=True)
        print(f"{r['point']}: {r['neighbours']['differ']} of {r['neighbours']['indices']} indices differ from the "
              f"composition; splits {r['geometry']['splits']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
