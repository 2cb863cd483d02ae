"""Fused mesh shape priors (loss.mesh_shape_priors fwd + bwd) against the same three losses composed from torch
ops on the same GPU (tests/mesh_priors_ref.priors_from_topology run on the device), in microseconds per step.

    python tools/prior_bench.py [--steps 1000] [--windows 7] [--out profiles/prior_bench.json]

Meshes: the cow (V = 2,930) and subdivided_sphere(2) (V = 40,962, the C5 mesh). One process; the two versions
alternate window by window after a warm-up of both; every window ends in a device synchronise; the per-step
median and the min..max spread over the windows are reported, with each version's kernel launches per step
(torch.profiler) and the two native passes' time between device events (back-to-back launches of the C ABI
calls), their algorithmic bytes and share of the HBM rate. Both versions' topologies are built before timing.
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
from tests.mesh_priors_ref import brute_topology, priors_from_topology, topology_to  # noqa: E402
from torch_renderer_amd import Meshes, _lib, kernels  # noqa: E402
from torch_renderer_amd.loss import mesh_shape_priors  # noqa: E402
from torch_renderer_amd.utils import subdivided_sphere  # noqa: E402

HBM_MEASURED = 6.29e12  # B/s, float4 copy on the MI355X (8.0e12 spec)
TARGET_LENGTH = 0.05


def algorithmic_bytes(V, E, P, blocks):
    """Bytes each native pass must move, from the shapes (every array once; gathers counted at their payload)."""
    fwd_r = 12 * V + 8 * E + 4 * E + 4 * (V + 1) + 4 * 2 * E + 8 * V + 16 * P + 4 * P
    fwd_w = 16 * V + 64 * P + 24 * blocks
    bwd_r = 12 * V + 8 * (V + 1) + 4 * 2 * E + 8 * V + 4 * 4 * P + 16 * V + 64 * P
    bwd_w = 12 * V
    return {"forward": fwd_r + fwd_w, "backward": bwd_r + bwd_w}


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


def native_pass_times(v, topo, iters=500):
    """us per mr_mesh_priors_forward (its two launches) and per mr_mesh_priors_backward, back to back."""
    L = _lib.load()
    p = _lib.ptr
    dev = v.device
    wsb = int(L.mr_mesh_priors_workspace(topo.V, topo.E, topo.P))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.empty(3, device=dev)
    one = torch.ones((), device=dev)
    gv = torch.empty_like(v)
    st = _lib.stream_handle(dev)

    def fwd():
        _lib.check(L.mr_mesh_priors_forward(p(v), topo.V, p(topo.edges), p(topo.edge_w), topo.E, p(topo.nbr_ptr),
                                            p(topo.nbr), p(topo.vert_w), p(topo.pairs), p(topo.pair_w), topo.P,
                                            TARGET_LENGTH, _lib.MR_PRIOR_ALL, 1, p(out), p(ws), wsb, st))

    def bwd():
        _lib.check(L.mr_mesh_priors_backward(p(v), topo.V, p(topo.nbr_ptr), p(topo.nbr), p(topo.vert_w),
                                             p(topo.pair_ptr), p(topo.pair_idx), topo.E, topo.P, TARGET_LENGTH,
                                             _lib.MR_PRIOR_ALL, p(one), p(one), p(one), p(ws), p(gv), st))

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
        res[name] = a.elapsed_time(b) * 1e3 / iters
    return res


def bench_mesh(name, verts, faces, steps, windows):
    dev = torch.device("cuda:0")
    f = faces.to(dev)
    leaf = verts.to(dev).requires_grad_(True)
    btopo = topology_to(brute_topology([faces], [verts.shape[0]]), dev, torch.float32)
    topo = kernels.mesh_prior_topology([f], [verts.shape[0]])

    def fused():
        leaf.grad = None
        e, lp, n = mesh_shape_priors(Meshes([leaf], [f]), TARGET_LENGTH)
        (e + lp + n).backward()

    def composed():
        leaf.grad = None
        e, lp, n = priors_from_topology(leaf, btopo, TARGET_LENGTH)
        (e + lp + n).backward()

    fused()
    g_fused = leaf.grad.clone()
    composed()
    g_torch = leaf.grad.clone()
    torch.cuda.synchronize()
    agree = (g_fused - g_torch).abs().max().item() / g_torch.abs().max().item()

    versions = {"fused": (fused, 4 * steps), "torch": (composed, steps)}
    for fn, _ in versions.values():  # warm up both
        for _ in range(50):
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
    res = {"mesh": name, "V": topo.V, "E": topo.E, "P": topo.P, "grad_rel_diff_fused_vs_torch": agree}
    for k, ts in times.items():
        n, err = count_launches(versions[k][0])
        res[k] = {"us_per_step_median": statistics.median(ts), "us_per_step_min": min(ts), "us_per_step_max": max(ts),
                  "windows": len(ts), "steps_per_window": versions[k][1], "kernel_launches_per_step": n}
        if err:
            res[k]["launch_count_error"] = err
    res["torch_over_fused"] = res["torch"]["us_per_step_median"] / res["fused"]["us_per_step_median"]
    blocks = (max(topo.V, topo.E, topo.P) + 255) // 256
    nat = native_pass_times(leaf.detach(), topo)
    byt = algorithmic_bytes(topo.V, topo.E, topo.P, blocks)
    res["native"] = {k: {"us_per_call": nat[k], "algorithmic_bytes": byt[k],
                         "share_of_measured_hbm_rate": byt[k] / HBM_MEASURED / (nat[k] * 1e-6)} for k in nat}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prior_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prior_bench: needs the GPU (no CPU timing)")
    cow_v, cow_f, _ = mesh_arrays("cow")
    sph = subdivided_sphere(2)
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "target_length": TARGET_LENGTH,
           "hbm_rate_used_Bps": HBM_MEASURED, "meshes": []}
    for name, v, f in (("cow", cow_v, cow_f), ("subdivided_sphere(2)", sph.verts_list()[0], sph.faces_list()[0])):
        r = bench_mesh(name, v, f, a.steps, a.windows)
        out["meshes"].append(r)
        print(f"{name}: fused {r['fused']['us_per_step_median']:.1f} us/step "
              f"[{r['fused']['us_per_step_min']:.1f}..{r['fused']['us_per_step_max']:.1f}], torch "
              f"{r['torch']['us_per_step_median']:.1f} [{r['torch']['us_per_step_min']:.1f}.."
              f"{r['torch']['us_per_step_max']:.1f}], torch/fused {r['torch_over_fused']:.2f}x, launches "
              f"{r['fused']['kernel_launches_per_step']} vs {r['torch']['kernel_launches_per_step']}", flush=True)
    out["fused_not_slower_on_every_mesh"] = all(m["torch_over_fused"] >= 1.0 for m in out["meshes"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    if not out["fused_not_slower_on_every_mesh"]:
        raise SystemExit("prior_bench: the fused path is slower than the torch composition")


if __name__ == "__main__":
    main()
