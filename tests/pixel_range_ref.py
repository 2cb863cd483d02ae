"""numpy restatements shared by the pixel-range tests: pix_to_ndc in float32 with the kernels' operation order,
and the face-to-tile rule (ndc_range_to_pix -> 8x8 tiles) with a free slack, for counting list entries."""
import numpy as np

F32 = np.float32
TILE = 8


def ndc_range(S1, S2):
    """pix_to_ndc's `range` (float32): 2 along the short side, 2 * S1 / S2 along the long one."""
    r = F32(2.0)
    if S1 > S2:
        r = F32(F32(S1) * r) / F32(S2)
    return F32(r)


def centre_ndc(p, S1, S2):
    """NDC of the centre of output pixel p along the axis of S1 pixels (col_ndc / row_ndc: pix_to_ndc(S1 - 1 - p,
    S1, S2)), every operation rounded to float32 in the kernels' order (no FMA). p may lie off the image."""
    r = ndc_range(S1, S2)
    off = F32(r / F32(2.0))
    i = (S1 - 1 - np.asarray(p)).astype(F32)
    return (-off + (r * i + off) / F32(S1)).astype(F32)


def centres(S1, S2):
    return centre_ndc(np.arange(S1), S1, S2)


def pitch(S1, S2):
    """One pixel in NDC."""
    return float(ndc_range(S1, S2)) / S1


def pixel_range(lo, hi, S1, S2, slack=0.05, tight=True):
    """The rule in float64 (arrays lo, hi of padded NDC bounds): pixel centre p sits at NDC ((S1 - 1) / 2 - p) *
    pitch, so the box spans pf0 = (S1 - 1) / 2 - hi / pitch .. pf1 = (S1 - 1) / 2 - lo / pitch; widened by `slack`
    px, rounded inward (tight) or outward (the rule before it), clamped to the image. p0 > p1: empty."""
    pt = pitch(S1, S2)
    half = (S1 - 1) / 2.0
    pf0 = np.clip(half - np.asarray(hi, np.float64) / pt - slack, -2.0, S1 + 1.0)
    pf1 = np.clip(half - np.asarray(lo, np.float64) / pt + slack, -2.0, S1 + 1.0)
    p0 = (np.ceil(pf0) if tight else np.floor(pf0)).astype(np.int64)
    p1 = (np.floor(pf1) if tight else np.ceil(pf1)).astype(np.int64)
    return np.maximum(p0, 0), np.minimum(p1, S1 - 1)


def tile_counts(fv, valid, H, W, slack=0.05, tight=True, pad=0.0):
    """(list entries, non-empty tiles) of one view: fv (F, 3, 3) NDC corners (x, y, z), valid (F,) bool."""
    x, y = fv[:, :, 0].astype(np.float64), fv[:, :, 1].astype(np.float64)
    cx0, cx1 = pixel_range(x.min(1) - pad, x.max(1) + pad, W, H, slack, tight)
    cy0, cy1 = pixel_range(y.min(1) - pad, y.max(1) + pad, H, W, slack, tight)
    ok = valid & (cx0 <= cx1) & (cy0 <= cy1)
    TX, TY = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    hist = np.zeros((TY, TX), dtype=np.int64)
    for a0, a1, b0, b1 in zip(cx0[ok] // TILE, cx1[ok] // TILE, cy0[ok] // TILE, cy1[ok] // TILE):
        hist[b0:b1 + 1, a0:a1 + 1] += 1
    return int(hist.sum()), int((hist > 0).sum())
