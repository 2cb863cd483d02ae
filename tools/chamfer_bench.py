"""The geometry-fitting step's point losses — sample both meshes, chamfer_distance, backward — fused
(ops.sample_points_from_meshes + loss.chamfer_distance, csrc/mr_points.hip) against the same step composed from
torch ops on the same GPU (tests/points_ref.sample_composed / chamfer_composed: cdist -> min -> gather), in
microseconds per step.

    python tools/chamfer_bench.py [--steps 300] [--windows 7] [--out profiles/chamfer_bench.json]

Points: ico_sphere(2) source and cow target at S = 1000 samples (mesh_deformer.py:299-352's setting), and a pair of
20,000-point clouds, chamfer only. One process; the two versions alternate window by window after a warm-up of
both; every window ends in a device synchronise; the per-step median and the min..max spread over the windows are
reported, with each version's kernel launches per step (torch.profiler) and the native forward and backward passes'
time between device events (back-to-back C ABI calls), and for the nearest-neighbour pass its distance evaluations
per second.
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
from tests.points_ref import chamfer_composed, sample_composed  # noqa: E402
from torch_renderer_amd import Meshes, _lib, kernels  # noqa: E402
from torch_renderer_amd.loss import chamfer_distance  # noqa: E402
from torch_renderer_amd.ops import sample_points_from_meshes  # noqa: E402
from torch_renderer_amd.utils import ico_sphere  # noqa: E402

DEV = "cuda:0"


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


def native_pass_times(x, y, iters=200):
    """us per mr_chamfer_forward (memset + 3 launches) and per mr_chamfer_backward (memset + 2 launches)."""
    L = _lib.load()
    p = _lib.ptr
    dev = x.device
    N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
    flags = _lib.MR_CHAMFER_POINT_MEAN | _lib.MR_CHAMFER_BATCH_MEAN
    wsb = int(L.mr_chamfer_workspace(N, P1, P2))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    bwsb = int(L.mr_chamfer_backward_workspace(N, P1, P2))
    bws = torch.empty(bwsb, dtype=torch.uint8, device=dev)
    ix = torch.empty((N, P1), dtype=torch.int32, device=dev)
    iy = torch.empty((N, P2), dtype=torch.int32, device=dev)
    coef, out, one = torch.empty((2, N), device=dev), torch.empty(1, device=dev), torch.ones(1, device=dev)
    gx, gy = torch.empty_like(x), torch.empty_like(y)
    st = _lib.stream_handle(dev)

    def fwd():
        _lib.check(L.mr_chamfer_forward(p(x), p(y), N, P1, P2, None, None, None, 2, flags, p(ix), p(iy), p(coef),
                                        p(out), p(ws), wsb, st))

    def bwd():
        _lib.check(L.mr_chamfer_backward(p(x), p(y), N, P1, P2, 2, flags, p(ix), p(iy), p(coef), p(one), p(gx), p(gy),
                                         p(bws), bwsb, st))

    res = {}
    for name, fn in (("forward", fwd), ("backward", bwd)):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        res[name] = {"us_per_call": a.elapsed_time(b) * 1e3 / iters}
    res["forward"]["distance_evaluations"] = 2 * N * P1 * P2
    res["forward"]["evaluations_per_second"] = 2 * N * P1 * P2 / (res["forward"]["us_per_call"] * 1e-6)
    return res


def run(point, versions, windows, warmup=20):
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
    for k, ts in times.items():
        n, err = count_launches(versions[k][0])
        point[k] = {"us_per_step_median": statistics.median(ts), "us_per_step_min": min(ts), "us_per_step_max": max(ts),
                    "windows": len(ts), "steps_per_window": versions[k][1], "kernel_launches_per_step": n}
        if err:
            point[k]["launch_count_error"] = err
    point["torch_over_fused"] = point["torch"]["us_per_step_median"] / point["fused"]["us_per_step_median"]
    return point


def bench_loop_step(steps, windows, S=1000):
    sph = ico_sphere(2)
    cow_v, cow_f, _ = mesh_arrays("cow")
    sv, sf = sph.verts_list()[0].float().to(DEV), sph.faces_list()[0].to(DEV)
    tv, tf = cow_v.to(DEV), cow_f.to(DEV)
    leaf = sv.clone().requires_grad_(True)
    trg = Meshes([tv], [tf])

    def fused():
        leaf.grad = None
        a = sample_points_from_meshes(trg, S)
        b = sample_points_from_meshes(Meshes([leaf], [sf]), S)
        loss, _ = chamfer_distance(a, b)
        loss.backward()

    def composed():
        leaf.grad = None
        a = sample_composed(tv, tf, S)
        b = sample_composed(leaf, sf, S)
        chamfer_composed(a, b).backward()

    point = {"point": f"ico_sphere(2) source, cow target, S = {S}: sample both, chamfer, backward",
             "V_source": sv.shape[0], "F_source": sf.shape[0], "V_target": tv.shape[0], "F_target": tf.shape[0]}
    run(point, {"fused": (fused, steps), "torch": (composed, steps)}, windows)
    g = torch.Generator().manual_seed(0)
    point["native"] = native_pass_times(torch.randn(1, S, 3, generator=g).to(DEV),
                                        torch.randn(1, S, 3, generator=g).to(DEV))
    return point


def neighbour_disagreement(x, y):
    """Where the fused neighbours of x differ from the composition's (torch.cdist takes its matmul form above 25
    points, which rounds differently): how many points, and for how many of them each side's choice is the
    nearer one by the float64 squared distance."""
    ix = kernels.nearest_points(x, y)[1].long()
    it = torch.cdist(x, y).argmin(dim=2)
    xd, yd = x.double(), y.double()

    def d64(idx):
        return ((xd - yd.gather(1, idx[..., None].expand(-1, -1, 3))) ** 2).sum(-1)

    df, dt = d64(ix), d64(it)
    differ = ix != it
    return {"points": ix.numel(), "differ": int(differ.sum()), "fused_is_nearer_in_float64": int((df < dt).sum()),
            "torch_is_nearer_in_float64": int((dt < df).sum())}


def bench_clouds(steps, windows, P=20000):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, P, 3, generator=g).to(DEV).requires_grad_(True)
    y = torch.randn(1, P, 3, generator=g).to(DEV).requires_grad_(True)

    def fused():
        x.grad = y.grad = None
        chamfer_distance(x, y)[0].backward()

    def composed():
        x.grad = y.grad = None
        chamfer_composed(x, y).backward()

    fused()
    gf = x.grad.clone()
    composed()
    agree = (gf - x.grad).abs().max().item() / x.grad.abs().max().item()
    point = {"point": f"{P} x {P} clouds: chamfer, backward", "grad_rel_diff_fused_vs_torch": agree,
             "neighbours": neighbour_disagreement(x.detach(), y.detach()),
             "matrix_bytes_the_composition_materialises": 4 * P * P}
    run(point, {"fused": (fused, steps), "torch": (composed, max(steps // 10, 5))}, windows, warmup=5)
    point["native"] = native_pass_times(x.detach(), y.detach())
    return point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chamfer_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chamfer_bench: needs the GPU (no CPU timing)")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "points": []}
    for fn in (bench_loop_step, bench_clouds):
        r = fn(a.steps, a.windows)
        out["points"].append(r)
        print(f"{r['point']}: fused {r['fused']['us_per_step_median']:.1f} us/step "
              f"[{r['fused']['us_per_step_min']:.1f}..{r['fused']['us_per_step_max']:.1f}], torch "
              f"{r['torch']['us_per_step_median']:.1f} [{r['torch']['us_per_step_min']:.1f}.."
              f"{r['torch']['us_per_step_max']:.1f}], torch/fused {r['torch_over_fused']:.2f}x, launches "
              f"{r['fused']['kernel_launches_per_step']} vs {r['torch']['kernel_launches_per_step']}; native fwd "
              f"{r['native']['forward']['us_per_call']:.1f} us, bwd {r['native']['backward']['us_per_call']:.1f} us",
              flush=True)
    out["fused_not_slower_at_every_point"] = all(p["torch_over_fused"] >= 1.0 for p in out["points"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
