"""ball_query (ops.ball_query, csrc/mr_ballquery.hip) against the same result composed from torch ops on the same GPU
(pairwise squared distances -> mask -> cumulative count -> the first K indices -> gather, which materialises several
(N, P1, P2) tensors) and, where K <= 32, against what a caller did before: knn_points followed by a radius mask (the
K nearest inside the radius, not the first K). Forward and forward + backward, in microseconds per step.

    python tools/ball_query_bench.py [--windows 7] [--out profiles/ball_query_bench.json]

Shapes, in the unit cube: 32 x 512 centroids x 4,096 points at K = 32, radius 0.2 (a PointNet++-style grouping);
300 x 2,000 x 400 at K = 16 (the scripts' batch); one scan of 20,000 points against itself at K = 16 with a radius
that gives a median of about K hits (an outlier filter), and the same scan with a radius that gives almost none (no
query ever fills: the scan never stops early). Every shape runs in a child process of its own under a time limit; the
run stops at the first child that fails. Inside a child the versions alternate window by window after a warm-up of
all (tools/knn_bench.py's loop), and the per-step median and the min..max spread over the windows are reported, with
each version's kernel launches per step, the launch geometry (kernels.ball_query_geometry), the hits per query, and
how many indices differ between the composition and the kernel.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from knn_bench import run  # noqa: E402  (the window loop and the launch count)

# (name, N, P1, P2, K, radius, queries are the targets, steps per window of the kernels, of the composition, seconds)
POINTS = [("grouping", 32, 512, 4096, 32, 0.2, False, 50, 5, 240),
          ("scripts batch", 300, 2000, 400, 16, 0.2, False, 50, 5, 240),
          ("outlier filter, about K hits", 1, 20000, 20000, 16, 0.06, True, 20, 3, 300),
          ("outlier filter, almost no hits", 1, 20000, 20000, 16, 0.005, True, 20, 3, 300)]
DEV = "cuda:0"


def composed(p1, p2, K, radius):
    """(dists, idx) of ball_query from torch ops, without a host read: the search carries no gradient, the gather
    does. A hit's slot is its cumulative count - 1; everything else is scattered into a spare slot K and cut off."""
    import torch

    from torch_renderer_amd.ops import masked_gather

    with torch.no_grad():
        r = torch.tensor(radius, dtype=torch.float32, device=p1.device)
        dx = p1[:, :, None, 0] - p2[:, None, :, 0]
        dy = p1[:, :, None, 1] - p2[:, None, :, 1]
        dz = p1[:, :, None, 2] - p2[:, None, :, 2]
        hit = ((dx * dx + dy * dy) + dz * dz) < r * r
        count = hit.cumsum(-1)
        slot = torch.where(hit & (count <= K), count - 1, K)
        idx = torch.full(p1.shape[:2] + (K + 1,), -1, dtype=torch.int64, device=p1.device)
        j = torch.arange(p2.shape[1], device=p1.device).expand_as(slot)
        idx.scatter_(2, slot, j)
        idx = idx[..., :K].contiguous()
    nn = masked_gather(p2, idx)
    d = ((p1[:, :, None] - nn) ** 2).sum(-1)
    return torch.where(idx >= 0, d, torch.zeros_like(d)), idx


def knn_masked(p1, p2, K, radius):
    """What a caller did before ball_query: the K nearest, then those outside the radius masked out."""
    import torch

    from torch_renderer_amd.ops import knn_points

    o = knn_points(p1, p2, K=K)
    inside = o.dists < radius * radius
    return torch.where(inside, o.dists, torch.zeros_like(o.dists)), torch.where(inside, o.idx, -1)


def bench_point(i, windows):
    import torch

    from torch_renderer_amd import kernels
    from torch_renderer_amd.ops import ball_query

    name, N, P1, P2, K, radius, same, nk, nt, _ = POINTS[i]
    g = torch.Generator().manual_seed(i)
    p2 = torch.rand(N, P2, 3, generator=g).to(DEV).requires_grad_(True)
    p1 = (p2.detach().clone() if same else torch.rand(N, P1, 3, generator=g).to(DEV)).requires_grad_(True)
    a, b = p1.detach(), p2.detach()
    qpg, splits, chunk = kernels.ball_query_geometry(N, P1, P2, K)
    point = {"point": f"{name}: {N} x {P1} x {P2}, K = {K}, radius {radius}", "N": N, "P1": P1, "P2": P2, "K": K,
             "radius": radius, "geometry": {"queries_per_group": qpg, "splits": splits, "lds_chunk": chunk},
             "distance_evaluations_of_a_full_scan": N * P1 * P2}

    ik = ball_query(a, b, K=K, radius=radius, return_nn=False).idx
    dt, it = composed(a, b, K, radius)
    differ = ik != it
    hits = (kernels.ball_query(a, b, K=P2 if P2 <= 4096 else 512, radius=radius)[1] >= 0).sum(-1).flatten().float()
    point["neighbours"] = {"indices": ik.numel(), "differ_from_the_composition": int(differ.sum()),
                           "hits_per_query_median": hits.median().item(), "hits_per_query_min": hits.min().item(),
                           "hits_per_query_max_counted_up_to_512_above_4096_targets": hits.max().item(),
                           "queries_with_K_or_more_hits": int((hits >= K).sum()), "queries": hits.numel()}
    nk_idx = knn_masked(a, b, K, radius)[1]
    point["neighbours"]["same_set_as_knn_then_mask_queries"] = int(
        (nk_idx.sort(-1).values == ik.sort(-1).values).all(-1).sum())

    def k_fwd():
        ball_query(a, b, K=K, radius=radius, return_nn=False)

    def t_fwd():
        composed(a, b, K, radius)

    def n_fwd():
        knn_masked(a, b, K, radius)

    def k_both():
        p1.grad = p2.grad = None
        ball_query(p1, p2, K=K, radius=radius, return_nn=False).dists.sum().backward()

    def t_both():
        p1.grad = p2.grad = None
        composed(p1, p2, K, radius)[0].sum().backward()

    def n_both():
        p1.grad = p2.grad = None
        knn_masked(p1, p2, K, radius)[0].sum().backward()

    k_both()
    gk = p1.grad.clone()
    t_both()
    point["grad_rel_diff_kernels_vs_torch"] = (gk - p1.grad).abs().max().item() / max(p1.grad.abs().max().item(), 1e-30)
    for mode, kf, tf, nf in (("forward", k_fwd, t_fwd, n_fwd), ("forward_backward", k_both, t_both, n_both)):
        r = run({"kernels": (kf, nk), "torch": (tf, nt), "knn_then_mask": (nf, nk)}, windows)
        r["torch_over_kernels"] = r["torch"]["us_per_step_median"] / r["kernels"]["us_per_step_median"]
        r["knn_then_mask_over_kernels"] = r["knn_then_mask"]["us_per_step_median"] / r["kernels"]["us_per_step_median"]
        point[mode] = r
    return point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ball_query_bench.json"))
    ap.add_argument("--point", type=int, default=None, help="run one shape in this process and print its JSON")
    a = ap.parse_args()
    if a.point is not None:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("ball_query_bench: needs the GPU (no CPU timing)")
        r = bench_point(a.point, a.windows)
        r["device"], r["torch_version"] = torch.cuda.get_device_name(0), torch.__version__
        print("BALL_BENCH_POINT " + json.dumps(r), flush=True)
        return
    out = {"points": []}
    for i, p in enumerate(POINTS):  # a fresh child per shape, each under its own time limit
        cmd = ["timeout", "-k", "10", str(p[-1]), sys.executable, os.path.abspath(__file__), "--point", str(i),
               "--windows", str(a.windows)]
        res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [l for l in res.stdout.splitlines() if l.startswith("BALL_BENCH_POINT ")]
        if res.returncode != 0 or not lines:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"ball_query_bench: shape {i} ended with status {res.returncode}; nothing further is started")
        r = json.loads(lines[-1][len("BALL_BENCH_POINT "):])
        out["device"], out["torch"] = r.pop("device"), r.pop("torch_version")
        out["points"].append(r)
        for mode in ("forward", "forward_backward"):
            k, t, n = r[mode]["kernels"], r[mode]["torch"], r[mode]["knn_then_mask"]
            print(f"{r['point']} {mode}: kernels {k['us_per_step_median']:.1f} us/step [{k['us_per_step_min']:.1f}.."
                  f"{k['us_per_step_max']:.1f}], torch {t['us_per_step_median']:.1f} [{t['us_per_step_min']:.1f}.."
                  f"{t['us_per_step_max']:.1f}] ({r[mode]['torch_over_kernels']:.2f}x), knn_points + mask "
                  f"{n['us_per_step_median']:.1f} [{n['us_per_step_min']:.1f}..{n['us_per_step_max']:.1f}] "
                  f"({r[mode]['knn_then_mask_over_kernels']:.2f}x), launches {k['kernel_launches_per_step']} / "
                  f"{t['kernel_launches_per_step']} / {n['kernel_launches_per_step']}", flush=True)
        nb = r["neighbours"]
        print(f"{r['point']}: {nb['differ_from_the_composition']} of {nb['indices']} indices differ from the "
              f"composition; hits per query median {nb['hits_per_query_median']:.0f}; splits "
              f"{r['geometry']['splits']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
