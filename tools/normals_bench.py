"""estimate_pointcloud_local_coord_frames (ops, csrc/mr_normals.hip) against the same result composed from torch ops on
the same GPU, in microseconds per call.

    python tools/normals_bench.py [--windows 7] [--out profiles/normals_bench.json]

The composition is upstream's route: neighbours -> gather (N,P,K,3) -> covariances (N,P,3,3) -> torch.linalg.eigh ->
the same sign step. At K = 16 the neighbours come from ops.knn_points (this library's kernel); at K = 50, which
knn_points (K <= 32) cannot do, from torch.cdist -> topk, which materialises the (N,P,P) matrix.

Shapes: 1 x 20,000, 300 x 2,000 and 1 x 2,000 at K = 16; 1 x 20,000 and 300 x 2,000 at K = 50. Every shape runs in a
child process of its own under a time limit; the run stops at the first child that fails. Inside a child the two
versions alternate window by window after a warm-up of both, every window ends in a device synchronise, and the
per-call median and the min..max spread over the windows are reported, with each version's kernel launches per call
(torch.profiler), the launch geometry (kernels.frames_geometry), and how far the two results are apart (cdist takes
its matmul form, which rounds differently on near-ties: a point whose K-th and (K+1)-th neighbours swap gets another
covariance).
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
POINTS = [(1, 20000, 16, 20, 5, 240), (300, 2000, 16, 10, 3, 300), (1, 2000, 16, 100, 20, 180),
          (1, 20000, 50, 5, 3, 300), (300, 2000, 50, 3, 2, 420)]
DEV = "cuda:0"


def composed(p, K):
    """(curvatures, frames) from torch ops, disambiguated."""
    import torch

    from torch_renderer_amd.ops import knn_points

    if K <= 32:
        idx = knn_points(p, p, K=K).idx
    else:
        idx = torch.cdist(p, p).topk(K, dim=2, largest=False).indices
    nb = p[:, :, None].expand(-1, -1, K, -1).gather(1, idx[..., None].expand(-1, -1, -1, 3))
    d = nb - p[:, :, None]
    e = d - d.mean(2, keepdim=True)
    cov = (e[..., :, None] * e[..., None, :]).mean(2)
    cur, frm = torch.linalg.eigh(cov)
    n, z = frm[..., 0], frm[..., 2]
    flip = lambda v: torch.where((2 * ((d * v[:, :, None]).sum(-1) > 0).sum(-1) < K)[..., None], -v, v)  # noqa: E731
    n, z = flip(n), flip(z)
    return cur, torch.stack((n, torch.cross(n, z, dim=-1), z), dim=-1)


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
    from torch_renderer_amd.ops import estimate_pointcloud_local_coord_frames

    N, P, K, nk, nt, _ = POINTS[i]
    p = torch.randn(N, P, 3, generator=torch.Generator().manual_seed(i)).to(DEV)
    bucket, qpg, splits, chunk = kernels.frames_geometry(N, P, K)
    point = {"point": f"{N} x {P}, K = {K}", "N": N, "P": P, "K": K,
             "geometry": {"bucket": bucket, "queries_per_group": qpg, "splits": splits, "lds_chunk": chunk},
             "distance_evaluations": N * P * P,
             "neighbours_of_the_composition": "ops.knn_points" if K <= 32 else "torch.cdist -> topk"}
    with torch.no_grad():
        ck, fk = estimate_pointcloud_local_coord_frames(p, K)
        ct, ft = composed(p, K)
        gap = (ct[..., 1] - ct[..., 0]) / ct.sum(-1)
        sin = torch.linalg.cross(fk[..., 0], ft[..., 0]).norm(dim=-1)
        rel = (ck - ct).abs().amax(-1) / ct.sum(-1)
        point["agreement"] = {
            "max_curvature_diff_over_trace": rel.max().item(),
            "points_with_curvature_diff_over_trace_above_1e-5": int((rel > 1e-5).sum()),
            "max_sin_between_normals_where_gap_ge_0.02": sin[gap >= 0.02].max().item(),
            "normals_of_opposite_sign": int(((fk[..., 0] * ft[..., 0]).sum(-1) < 0).sum()),
            "points": N * P}

        def k_call():
            estimate_pointcloud_local_coord_frames(p, K)

        def t_call():
            composed(p, K)

        r = run({"kernels": (k_call, nk), "torch": (t_call, nt)}, windows)
    r["torch_over_kernels"] = r["torch"]["us_per_call_median"] / r["kernels"]["us_per_call_median"]
    r["kernels"]["evaluations_per_second"] = N * P * P / (r["kernels"]["us_per_call_median"] * 1e-6)
    point["forward"] = r
    return point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_bench.json"))
    ap.add_argument("--point", type=int, default=None, help="run one shape in this process and print its JSON")
    a = ap.parse_args()
    if a.point is not None:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("normals_bench: needs the GPU (no CPU timing)")
        r = bench_point(a.point, a.windows)
        r["device"], r["torch_version"] = torch.cuda.get_device_name(0), torch.__version__
        print("NORMALS_BENCH_POINT " + json.dumps(r), flush=True)
        return
    out = {"points": []}
    for i, p in enumerate(POINTS):  # a fresh child per shape, each under its own time limit
        cmd = ["timeout", "-k", "10", str(p[5]), sys.executable, os.path.abspath(__file__), "--point", str(i),
               "--windows", str(a.windows)]
        res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [l for l in res.stdout.splitlines() if l.startswith("NORMALS_BENCH_POINT ")]
        if res.returncode != 0 or not lines:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"normals_bench: shape {i} ended with status {res.returncode}; nothing further is started")
        r = json.loads(lines[-1][len("NORMALS_BENCH_POINT "):])
        out["device"], out["torch"] = r.pop("device"), r.pop("torch_version")
        out["points"].append(r)
        k, t = r["forward"]["kernels"], r["forward"]["torch"]
        print(f"{r['point']}: kernels {k['us_per_call_median']:.1f} us/call [{k['us_per_call_min']:.1f}.."
              f"{k['us_per_call_max']:.1f}], torch {t['us_per_call_median']:.1f} [{t['us_per_call_min']:.1f}.."
              f"{t['us_per_call_max']:.1f}], torch/kernels {r['forward']['torch_over_kernels']:.2f}x, launches "
              f"{k['kernel_launches_per_call']} vs {t['kernel_launches_per_call']}, splits {r['geometry']['splits']}",
              flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:  # written after every shape: a later child's failure keeps the earlier numbers
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
