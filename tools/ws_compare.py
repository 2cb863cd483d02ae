"""Every mr_*_workspace query of two builds of the library over one grid of arguments; prints the table and
exits non-zero when a value differs (a refactor of the host code must leave every size alone).

    python tools/ws_compare.py OLD.so NEW.so > table.txt

The grid reaches one view and 64 (several bands of tile rows per view, and one), images from 8x8 to a tile grid
past MR_VIEW_TMAX (the count -> scan path), F = 0 .. 81,920, max_faces_per_bin 0 / 100, K = 2 / 50 and
P = 1 .. 20,000. Without a GPU the library sizes the bands for 256 CUs."""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_renderer_amd import _lib  # noqa: E402

NS, SIZES, FS, MFPB, KS, PS = (1, 64), (8, 64, 512, 1024, 2048), (0, 1, 5856, 81920), (0, 100), (2, 50), (1, 1000, 20000)


def queries(L):
    for N, S, F, m in itertools.product(NS, SIZES, FS, MFPB):
        yield f"rasterize_meshes N={N} Ftot={N * F} {S}x{S} mfpb={m}", L.mr_rasterize_meshes_workspace(N, N * F, S, S, m)
        yield f"rasterize_meshes_world N={N} F={F} {S}x{S} mfpb={m}", L.mr_rasterize_meshes_world_workspace(N, F, S, S, m)
        yield f"render N={N} F={F} {S}x{S} mfpb={m}", L.mr_render_workspace(N, F, S, S, m)
        yield f"render_meshes N={N} F={N * F} {S}x{S} mfpb={m}", L.mr_render_workspace_meshes(N, N * F, S, S, m)
        for K in KS:
            yield f"soft_silhouette N={N} F={F} {S}x{S} K={K} mfpb={m}", L.mr_soft_silhouette_workspace(N, F, S, S, K, m)
    for N, S, F in itertools.product(NS, SIZES, FS):
        yield f"render_backward N={N} V={F // 2 + 2} F={F} {S}x{S}", L.mr_render_backward_workspace(N, F // 2 + 2, F, S, S)
        yield f"pose_loss npix={N * S * S}", L.mr_pose_loss_workspace(N * S * S)
    for F in FS:
        yield f"shade_fragments F={F}", L.mr_shade_fragments_workspace(F)
        yield f"shade_fragments_backward V={F // 2 + 2} F={F}", L.mr_shade_fragments_backward_workspace(F // 2 + 2, F)
        yield f"mesh_priors V={F // 2 + 2} E={3 * F // 2} P={3 * F // 2}", L.mr_mesh_priors_workspace(F // 2 + 2, 3 * F // 2, 3 * F // 2)
        yield f"sample_points_backward V={F // 2 + 2}", L.mr_sample_points_backward_workspace(F // 2 + 2)
    for N, P1, P2 in itertools.product(NS, PS, PS):
        yield f"nearest_points N={N} P1={P1} P2={P2}", L.mr_nearest_points_workspace(N, P1, P2)
        yield f"chamfer N={N} P1={P1} P2={P2}", L.mr_chamfer_workspace(N, P1, P2)
        yield f"chamfer_backward N={N} P1={P1} P2={P2}", L.mr_chamfer_backward_workspace(N, P1, P2)


def main(old, new):
    a, b = list(queries(_lib.load(old))), list(queries(_lib.load(new)))
    bad = 0
    print(f"# query | {os.path.basename(old)} | {os.path.basename(new)} | verdict")
    for (name, x), (_, y) in zip(a, b):
        bad += x != y
        print(f"{name} | {x} | {y} | {'equal' if x == y else 'DIFFERENT'}")
    print(f"# {len(a)} queries, {bad} different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
