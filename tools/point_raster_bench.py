"""Point-cloud rendering on the HIP kernels (PointsRenderer: mr_project_points -> mr_rasterize_points ->
mr_composite_points_*, csrc/mr_pointraster.hip), milliseconds per step, forward alone and forward + backward to the
points and features.

    python tools/point_raster_bench.py [--steps 10] [--windows 5] [--out profiles/point_raster_bench.json]

(a) the library workload: 20,000 points sampled from the cow, 64 canonical views, 512x512, alpha compositing of RGB
    features, at radius = 0.01, K = 8 (upstream's defaults) and at radius = 0.003, K = 10 (the reference's).
(b) the same step composed from torch ops on the same GPU (pixel-versus-point d2, mask, topk smallest, gather,
    cumprod compositing) at a size it can hold, since it materialises N * HW * P distances: 128x128, 5,000 points,
    N = 8 views; the kernels are timed at that size too, and the two images compared.
(c) a sweep of P at (a)'s first setting with N = 8 views, forward only: the rasterizer is a brute-force scan (every
    (view, tile) streams the whole cloud), so its time per point is flat until the fixed costs are amortised and stays
    flat after; the sweep records where, i.e. from where a binning pass could begin to pay.

One process; a warm-up of every version, then the versions alternate window by window; every window ends in a device
synchronise; the per-step median and the min..max spread over the windows are reported.
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

from tests import point_raster_ref as PR  # noqa: E402
from tests.helpers import canonical_views, mesh_arrays  # noqa: E402
from torch_renderer_amd import Meshes, Pointclouds  # noqa: E402
from torch_renderer_amd import points_renderer as PRn  # noqa: E402
from torch_renderer_amd.cameras import PerspectiveCameras  # noqa: E402
from torch_renderer_amd.ops import sample_points_from_meshes  # noqa: E402

DEV = "cuda:0"


def setup(P, N, H, W, radius, K):
    v, f, _ = mesh_arrays("cow")
    torch.manual_seed(0)
    pts = sample_points_from_meshes(Meshes([v.to(DEV)], [f.to(DEV)]), P)[0].contiguous().requires_grad_(True)
    feats = torch.rand(P, 3, device=DEV).requires_grad_(True)
    R, T, intr, (_, _, Kcv) = canonical_views(v, N, H, W)
    cams = PerspectiveCameras(focal_length=((float(Kcv[0, 0]), float(Kcv[1, 1])),),
                              principal_point=((float(Kcv[0, 2]), float(Kcv[1, 2])),), in_ndc=False,
                              image_size=torch.tensor([[H, W]]), device=DEV)
    rs = PRn.PointsRasterizationSettings(image_size=(H, W), radius=radius, points_per_pixel=K)
    ren = PRn.PointsRenderer(PRn.PointsRasterizer(cams, rs), PRn.AlphaCompositor(background_color=(0.0, 0.0, 0.0)))
    pc = Pointclouds([pts]).extend(N)
    return ren, pc, pts, feats, R.to(DEV), T.to(DEV), intr.to(DEV)


def torch_composition(pts, feats, R, T, intr, H, W, radius, K):
    """The same image from torch ops: N * HW * P distances, mask, topk, gather, alpha compositing."""
    ndc = PR.project_ref(pts, R, T, intr)                                        # (N,P,3)
    xf, yf = PR.pixel_centres(H, W)
    xf, yf = torch.from_numpy(xf).to(DEV), torch.from_numpy(yf).to(DEV)
    dx = ndc[:, None, None, :, 0] - xf[None, None, :, None]
    dy = ndc[:, None, None, :, 1] - yf[None, :, None, None]
    d2 = dx * dx + dy * dy                                                       # (N,H,W,P)
    z = ndc[:, None, None, :, 2].expand_as(d2)
    zk = torch.where((d2 < radius * radius) & (z >= 0), z, torch.full_like(z, float("inf")))
    zs, idx = torch.topk(zk, K, dim=-1, largest=False)
    filled = torch.isfinite(zs)
    a = torch.where(filled, 1.0 - torch.gather(d2, -1, idx) / (radius * radius), torch.zeros_like(zs))
    Tr = torch.cumprod(torch.cat([torch.ones_like(a[..., :1]), 1.0 - a[..., :-1]], -1), -1)
    return (feats[idx] * (a * Tr)[..., None]).sum(-2)


def run(versions, windows, warmup=3):
    for fn, _ in versions.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in versions}
    for _ in range(windows):
        for k, (fn, n) in versions.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / n)
    return {k: {"ms_per_step_median": statistics.median(ts), "ms_per_step_min": min(ts), "ms_per_step_max": max(ts),
                "windows": len(ts), "steps_per_window": versions[k][1]} for k, ts in times.items()}


def steps_of(image_of, leaves):
    def fwd():
        with torch.no_grad():
            return image_of()

    def fwd_bwd():
        for t in leaves:
            t.grad = None
        image_of().sum().backward()

    return fwd, fwd_bwd


def library_point(P, N, H, W, radius, K, steps, windows, backward=True):
    ren, pc, pts, feats, R, T, _ = setup(P, N, H, W, radius, K)
    fwd, fwd_bwd = steps_of(lambda: ren(pc, features=[feats], R=R, T=T), (pts, feats))
    v = {"forward": (fwd, steps)}
    if backward:
        v["forward_backward"] = (fwd_bwd, steps)
    r = run(v, windows)
    with torch.no_grad():
        frag = ren.rasterizer(pc, R=R, T=T)
    r.update(P=P, N=N, H=H, W=W, radius=radius, K=K,
             filled_slots_per_pixel=(frag.idx >= 0).float().sum(-1).mean().item(),
             coarse_tests=N * ((H + 15) // 16) * ((W + 15) // 16) * P)
    r["forward_ns_per_point_per_view"] = r["forward"]["ms_per_step_median"] * 1e6 / (P * N)
    return r


def torch_point(P, N, H, W, radius, K, steps, windows):
    ren, pc, pts, feats, R, T, intr = setup(P, N, H, W, radius, K)
    lib = lambda: ren(pc, features=[feats], R=R, T=T)  # noqa: E731
    tor = lambda: torch_composition(pts, feats, R, T, intr, H, W, radius, K)  # noqa: E731
    with torch.no_grad():
        diff = (lib() - tor()).abs().max().item()
    lf, lfb = steps_of(lib, (pts, feats))
    tf, tfb = steps_of(tor, (pts, feats))
    r = run({"kernels_forward": (lf, steps), "torch_forward": (tf, max(steps // 2, 2)),
             "kernels_forward_backward": (lfb, steps), "torch_forward_backward": (tfb, max(steps // 2, 2))}, windows)
    r.update(P=P, N=N, H=H, W=W, radius=radius, K=K, max_abs_image_diff=diff,
             torch_over_kernels_forward=r["torch_forward"]["ms_per_step_median"] /
             r["kernels_forward"]["ms_per_step_median"],
             torch_over_kernels_forward_backward=r["torch_forward_backward"]["ms_per_step_median"] /
             r["kernels_forward_backward"]["ms_per_step_median"])
    r["kernels_faster_than_torch"] = r["torch_over_kernels_forward"] > 1.0 and \
        r["torch_over_kernels_forward_backward"] > 1.0
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_raster_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("point_raster_bench: needs the GPU (no CPU timing)")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "library": [], "sweep": []}

    def show(tag, r, keys):
        print(tag + ": " + ", ".join(f"{k} {r[k]['ms_per_step_median']:.3f} ms [{r[k]['ms_per_step_min']:.3f}.."
                                     f"{r[k]['ms_per_step_max']:.3f}]" for k in keys), flush=True)

    for radius, K in ((0.01, 8), (0.003, 10)):
        r = library_point(20000, 64, 512, 512, radius, K, a.steps, a.windows)
        out["library"].append(r)
        show(f"(a) P = 20000, N = 64, 512x512, radius {radius}, K = {K}", r, ("forward", "forward_backward"))
    r = out["torch_composition"] = torch_point(5000, 8, 128, 128, 0.01, 8, a.steps, a.windows)
    show("(b) P = 5000, N = 8, 128x128, radius 0.01, K = 8", r,
         ("kernels_forward", "torch_forward", "kernels_forward_backward", "torch_forward_backward"))
    print(f"    torch / kernels: forward {r['torch_over_kernels_forward']:.2f}x, forward + backward "
          f"{r['torch_over_kernels_forward_backward']:.2f}x, max |image diff| {r['max_abs_image_diff']:.2e}", flush=True)
    for P in (1000, 4000, 16000, 64000, 256000, 1000000):
        r = library_point(P, 8, 512, 512, 0.01, 8, max(a.steps // 2, 2), max(a.windows // 2, 3), backward=False)
        out["sweep"].append(r)
        print(f"(c) P = {P}, N = 8: forward {r['forward']['ms_per_step_median']:.3f} ms = "
              f"{r['forward_ns_per_point_per_view']:.2f} ns per (point, view)", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
