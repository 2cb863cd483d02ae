"""sample_farthest_points (ops.sample_farthest_points, csrc/mr_fps.hip) against the same algorithm composed from torch
ops on the same GPU, batched over N, in microseconds per call.

    python tools/fps_bench.py [--windows 7] [--out profiles/fps_bench.json]

The composition runs K sequential rounds; a round gathers the last selected point of every cloud, takes the squared
distances of all points to it, folds them into the running minimum with ``torch.minimum`` and picks the next point
with ``argmax``. Shapes: 1 x 20,000 -> K = 1,000; 300 x 2,000 -> K = 500 (the ICP scripts' batch); 1 x 2,000 ->
K = 1,000 (one small cloud: latency only); and one streamed shape, 1 x 200,000 -> K = 256. Every shape runs in a
child process of its own under a time limit; the run stops at the first child that fails. Inside a child the two
versions alternate window by window after a warm-up of both, every window ends in a device synchronise, and the
per-call median and the min..max spread over the windows are reported, with each version's kernel launches per call
(torch.profiler), the launch geometry (kernels.farthest_geometry) and how many selected indices differ between the
composition and the kernels (the composition's sum may round, and its argmax may break ties, differently).
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

# (N, P, K, calls per window of the kernels, of the composition, seconds allowed)
POINTS = [(1, 20000, 1000, 20, 3, 240), (300, 2000, 500, 20, 3, 240), (1, 2000, 1000, 50, 3, 240),
          (1, 200000, 256, 5, 3, 240)]
DEV = "cuda:0"


def composed(points, K):
    """(selected_points, selected_idx) from torch ops, every cloud starting at index 0."""
    import torch

    N, P, _ = points.shape
    rows = torch.arange(N, device=points.device)
    idx = torch.empty((N, K), dtype=torch.int64, device=points.device)
    m = torch.full((N, P), float("inf"), device=points.device)
    cur = torch.zeros(N, dtype=torch.int64, device=points.device)
    for k in range(K):
        idx[:, k] = cur
        if k + 1 == K:
            break
        last = points[rows, cur]
        m = torch.minimum(m, ((points - last[:, None]) ** 2).sum(-1))
        cur = m.argmax(1)
    return points.gather(1, idx[..., None].expand(-1, -1, 3)), idx


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
    from torch_renderer_amd.ops import sample_farthest_points

    N, P, K, nk, nt, _ = POINTS[i]
    pts = torch.randn(N, P, 3, generator=torch.Generator().manual_seed(i)).to(DEV)
    threads, per, streamed = kernels.farthest_geometry(N, P, K)
    point = {"point": f"{N} x {P} -> K = {K}", "N": N, "P": P, "K": K,
             "geometry": {"threads": threads, "points_per_thread": per, "streamed": streamed}}
    ik = sample_farthest_points(pts, K=K)[1]
    it = composed(pts, K)[1]
    differ = ik != it
    first = differ.int().argmax(1)[differ.any(1)]  # after its first difference a cloud's selections are another chain
    point["selected"] = {"indices": ik.numel(), "differ": int(differ.sum()), "clouds_with_a_difference":
                         int(differ.any(1).sum()), "earliest_round_of_a_difference":
                         int(first.min()) if first.numel() else None}

    def k_fwd():
        sample_farthest_points(pts, K=K)

    def t_fwd():
        composed(pts, K)

    r = run({"kernels": (k_fwd, nk), "torch": (t_fwd, nt)}, windows)
    r["torch_over_kernels"] = r["torch"]["us_per_call_median"] / r["kernels"]["us_per_call_median"]
    r["kernels"]["us_per_round"] = r["kernels"]["us_per_call_median"] / K
    r["torch"]["us_per_round"] = r["torch"]["us_per_call_median"] / K
    point["forward"] = r
    return point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps_bench.json"))
    ap.add_argument("--point", type=int, default=None, help="run one shape in this process and print its JSON")
    a = ap.parse_args()
    if a.point is not None:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("fps_bench: needs the GPU (no CPU timing)")
        r = bench_point(a.point, a.windows)
        r["device"], r["torch_version"] = torch.cuda.get_device_name(0), torch.__version__
        print("FPS_BENCH_POINT " + json.dumps(r), flush=True)
        return
    out = {"points": []}
    for i, p in enumerate(POINTS):  # a fresh child per shape, each under its own time limit
        cmd = ["timeout", "-k", "10", str(p[5]), sys.executable, os.path.abspath(__file__), "--point", str(i),
               "--windows", str(a.windows)]
        res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [l for l in res.stdout.splitlines() if l.startswith("FPS_BENCH_POINT ")]
        if res.returncode != 0 or not lines:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"fps_bench: shape {i} ended with status {res.returncode}; nothing further is started")
        r = json.loads(lines[-1][len("FPS_BENCH_POINT "):])
        out["device"], out["torch"] = r.pop("device"), r.pop("torch_version")
        out["points"].append(r)
        k, t = r["forward"]["kernels"], r["forward"]["torch"]
        print(f"{r['point']}: kernels {k['us_per_call_median']:.1f} us/call [{k['us_per_call_min']:.1f}.."
              f"{k['us_per_call_max']:.1f}], torch {t['us_per_call_median']:.1f} [{t['us_per_call_min']:.1f}.."
              f"{t['us_per_call_max']:.1f}], torch/kernels {r['forward']['torch_over_kernels']:.2f}x, launches "
              f"{k['kernel_launches_per_call']} vs {t['kernel_launches_per_call']}; {r['selected']['differ']} of "
              f"{r['selected']['indices']} indices differ; geometry {r['geometry']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
