"""The pose search's inner step — score S rigid-pose hypotheses of one cloud pair by chamfer distance — fused
(loss.posed_chamfer_distance, k_posed_nn / k_posed_final of csrc/mr_points.hip) against (a) the library composition
it replaces: torch repeat / bmm / add that materialise the S transformed clouds, then
chamfer_distance(batch_reduction=None); and (b) the same with the chamfer composed from torch ops
(tests/points_ref.chamfer_composed per cloud: cdist -> argmin -> gather -> mean). Microseconds per step, forward
alone and forward + backward to (R, T).

    python tools/pose_chamfer_bench.py [--steps 200] [--windows 7] [--out profiles/pose_chamfer_bench.json]

The two shapes of the reference's scripts: S = 1000 hypotheses, 1000 source points, a target of ~500 (cow surface
samples cropped at the centroid's x, chamfer_loss_evaluation.py:105-126) and S = 400, 500 source points, ~250 target
points (pytorch3d_icp_evaluation.py:158-239). One process; the versions alternate window by window after a warm-up
of all; every window ends in a device synchronise; the per-step median and the min..max spread over the windows are
reported, with each version's kernel launches per step (torch.profiler) and, for the fused pass, the time of
back-to-back C ABI calls between device events and its distance evaluations per second. The bar: the fused median
below the fastest window of (a).
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
from tools.chamfer_bench import count_launches  # noqa: E402
from torch_renderer_amd import Meshes, _lib, kernels  # noqa: E402
from torch_renderer_amd.loss import chamfer_distance, posed_chamfer_distance  # noqa: E402
from torch_renderer_amd.ops import sample_points_from_meshes  # noqa: E402
from torch_renderer_amd.transforms import euler_angles_to_matrix  # noqa: E402

DEV = "cuda:0"


def composed_batch(x, y):
    """tests/points_ref.chamfer_composed without its batch mean: (N,) from cdist -> argmin -> gather -> mean."""
    with torch.no_grad():
        d = torch.cdist(x, y)
        ix, iy = d.argmin(dim=2), d.argmin(dim=1)
    cx = ((x - y.gather(1, ix[..., None].expand(-1, -1, 3))) ** 2).sum(-1).mean(1)
    cy = ((y - x.gather(1, iy[..., None].expand(-1, -1, 3))) ** 2).sum(-1).mean(1)
    return cx + cy


def materialise(x, y, R, T):
    """What the scripts do each round: S copies of both clouds, the source ones transformed."""
    S = R.shape[0]
    return torch.bmm(x.repeat(S, 1, 1), R) + T[:, None], y.repeat(S, 1, 1)


def clouds(P1):
    """Source: P1 samples of the cow's surface. Target: P1 other samples cropped at the centroid's x."""
    v, f, _ = mesh_arrays("cow")
    mesh = Meshes([v.to(DEV)], [f.to(DEV)])
    torch.manual_seed(0)
    x = sample_points_from_meshes(mesh, P1)[0]
    t = sample_points_from_meshes(mesh, P1)[0]
    y = t[t[:, 0] > t[:, 0].mean()]
    return x.contiguous(), y.contiguous()


def native_pass(x, y, R, T, want_grad, iters=200):
    """us per mr_posed_chamfer (two launches) between device events, the poses already packed."""
    L = _lib.load()
    p = _lib.ptr
    S, P1, P2 = R.shape[0], x.shape[0], y.shape[0]
    rts = kernels._pack_rts(R, T, None)
    out = torch.empty(S, device=DEV)
    pg = torch.empty((S, 13), device=DEV) if want_grad else None
    wsb = int(L.mr_posed_chamfer_workspace(S, P1, P2))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    st = _lib.stream_handle(x.device)

    def fn():
        _lib.check(L.mr_posed_chamfer(p(x), p(y), P1, P2, p(rts), S, 2, _lib.MR_CHAMFER_POINT_MEAN, p(out), None, None,
                                      p(pg), p(ws), wsb, st))

    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / iters
    return {"us_per_call": us, "distance_evaluations": 2 * S * P1 * P2,
            "evaluations_per_second": 2 * S * P1 * P2 / (us * 1e-6)}


def run(versions, windows, warmup=10):
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
    res = {}
    for k, ts in times.items():
        n, err = count_launches(versions[k][0])
        res[k] = {"us_per_step_median": statistics.median(ts), "us_per_step_min": min(ts), "us_per_step_max": max(ts),
                  "windows": len(ts), "steps_per_window": versions[k][1], "kernel_launches_per_step": n}
        if err:
            res[k]["launch_count_error"] = err
    res["a_over_fused"] = res["library_composition"]["us_per_step_median"] / res["fused"]["us_per_step_median"]
    res["b_over_fused"] = res["torch_composition"]["us_per_step_median"] / res["fused"]["us_per_step_median"]
    res["fused_median_below_min_of_a"] = res["fused"]["us_per_step_median"] < res["library_composition"]["us_per_step_min"]
    return res


def bench_shape(S, P1, steps, windows):
    x, y = clouds(P1)
    g = torch.Generator().manual_seed(S)
    R = euler_angles_to_matrix(torch.randn(S, 3, generator=g), "XYZ").to(DEV).requires_grad_(True)
    T = (0.2 * torch.randn(S, 3, generator=g)).to(DEV).requires_grad_(True)

    def fwd(loss_of):
        def step():
            with torch.no_grad():
                return loss_of()
        return step

    def fwd_bwd(loss_of):
        def step():
            R.grad = T.grad = None
            loss_of().sum().backward()
        return step

    losses = {"fused": lambda: posed_chamfer_distance(x, y, R, T),
              "library_composition": lambda: chamfer_distance(*materialise(x, y, R, T), batch_reduction=None)[0],
              "torch_composition": lambda: composed_batch(*materialise(x, y, R, T))}
    fused, lib = losses["fused"]().detach(), losses["library_composition"]().detach()
    point = {"point": f"S = {S} poses, P1 = {P1}, P2 = {y.shape[0]}", "S": S, "P1": P1, "P2": y.shape[0],
             "max_abs_diff_fused_vs_library_composition": (fused - lib).abs().max().item()}
    slow = max(steps // 4, 5)
    for mode, wrap in (("forward", fwd), ("forward_backward", fwd_bwd)):
        point[mode] = run({"fused": (wrap(losses["fused"]), steps),
                           "library_composition": (wrap(losses["library_composition"]), steps),
                           "torch_composition": (wrap(losses["torch_composition"]), slow)}, windows)
    point["native"] = {"forward": native_pass(x, y, R.detach(), T.detach(), False),
                       "forward_with_pose_grad": native_pass(x, y, R.detach(), T.detach(), True)}
    return point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_chamfer_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_chamfer_bench: needs the GPU (no CPU timing)")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "points": []}
    for S, P1 in ((1000, 1000), (400, 500)):
        r = bench_shape(S, P1, a.steps, a.windows)
        out["points"].append(r)
        for mode in ("forward", "forward_backward"):
            m = r[mode]
            f, la, tb = m["fused"], m["library_composition"], m["torch_composition"]
            print(f"{r['point']}, {mode}: fused {f['us_per_step_median']:.1f} us/step [{f['us_per_step_min']:.1f}.."
                  f"{f['us_per_step_max']:.1f}], (a) {la['us_per_step_median']:.1f} [{la['us_per_step_min']:.1f}.."
                  f"{la['us_per_step_max']:.1f}] = {m['a_over_fused']:.2f}x, (b) {tb['us_per_step_median']:.1f} "
                  f"[{tb['us_per_step_min']:.1f}..{tb['us_per_step_max']:.1f}] = {m['b_over_fused']:.2f}x; launches "
                  f"{f['kernel_launches_per_step']} / {la['kernel_launches_per_step']} / "
                  f"{tb['kernel_launches_per_step']}", flush=True)
        n = r["native"]["forward"]
        print(f"  native forward {n['us_per_call']:.1f} us = {n['evaluations_per_second']:.3e} evaluations/s, with the "
              f"pose gradient {r['native']['forward_with_pose_grad']['us_per_call']:.1f} us", flush=True)
    out["fused_median_below_min_of_a_everywhere"] = all(p[m]["fused_median_below_min_of_a"] for p in out["points"]
                                                        for m in ("forward", "forward_backward"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
