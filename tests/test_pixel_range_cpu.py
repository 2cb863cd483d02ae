"""mr_pixel_range (the kernels' ndc_range_to_pix compiled for the host: the rule behind the binning's tile
rectangles and the rasters' candidate rectangles) fuzzed against a float32 numpy restatement of pix_to_ndc and
eval_face's bbox test. No GPU.

For every box the range must be
  * a superset: every pixel whose centre the exact test keeps (not (x > hi or x < lo), float32) lies in p0 .. p1;
  * tight: every pixel in p0 .. p1 has its centre within 0.06 px of the box (the rule's 0.05 px slack plus the
    inverse map's error) — the outward floor / ceil rounding this replaced lists pixels up to 1 px away;
  * empty (p0 > p1) for a box that lies off the image.
Bounds: 0.06 px = the 0.05 px widening + 0.01 px for the float32 inverse, whose error is ~S * 2^-24 * a few
< 2e-3 px at S = 4096 (NDC values near 1 have a 6e-8 ulp, one pixel is >= 4.9e-4 NDC)."""
import ctypes

import numpy as np
import pytest

from tests.pixel_range_ref import F32, centres, ndc_range
from torch_renderer_amd import _lib

SIDES = [(16, 16), (60, 100), (100, 60), (37, 211), (512, 512), (2048, 512), (512, 2048), (4096, 4096)]
PADS = [0.0, float(np.sqrt(F32(9.21e-4)))]


@pytest.fixture(scope="module")
def lib():
    import os

    if not os.path.exists(_lib.LIB_PATH):
        from torch_renderer_amd import _build

        _build.build()
    return _lib.load()


def pixel_ranges(lib, lo, hi, S1, S2):
    p0, p1 = ctypes.c_int32(), ctypes.c_int32()
    out = np.empty((len(lo), 2), dtype=np.int64)
    for k in range(len(lo)):
        assert lib.mr_pixel_range(float(lo[k]), float(hi[k]), S1, S2, ctypes.byref(p0), ctypes.byref(p1)) == 0
        out[k] = p0.value, p1.value
    return out[:, 0], out[:, 1]


def boxes(S1, S2, rng, n=160):
    """(xmin, xmax) float32 pairs: edges on pixel centres, 1 ulp and 1e-7 .. 1e-3 NDC either side of them, a few
    fractions of a pixel around the rule's slack, and random; 1 - 3 px and wider; some hanging off the image."""
    c = centres(S1, S2)
    pitch = float(ndc_range(S1, S2)) / S1
    a = rng.integers(0, S1, n)
    b = np.clip(a + rng.integers(0, 4, n) * (rng.random(n) < 0.8) + rng.integers(0, S1, n) * (rng.random(n) < 0.1), 0,
                S1 - 1)
    lo0, hi0 = c[b], c[a]  # NDC decreases with the pixel index
    out = [(lo0, hi0)]
    inf = F32(np.inf)
    out.append((np.nextafter(lo0, inf), np.nextafter(hi0, -inf)))
    out.append((np.nextafter(lo0, -inf), np.nextafter(hi0, inf)))
    out.append((np.nextafter(lo0, inf), np.nextafter(hi0, inf)))
    for d in (1e-7, 1e-6, 1e-5, 1e-4, 1e-3):
        for s0, s1 in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            out.append(((lo0 + F32(s0 * d)).astype(F32), (hi0 + F32(s1 * d)).astype(F32)))
    for d in (0.04, 0.049, 0.051, 0.06, 0.5):  # fractions of a pixel: around the 0.05 px slack, and between centres
        for s0, s1 in ((1, -1), (-1, 1)):
            out.append(((lo0 + F32(s0 * d * pitch)).astype(F32), (hi0 + F32(s1 * d * pitch)).astype(F32)))
    x = (rng.random((2, 4 * n)) * (S1 + 4) - 2.5).astype(np.float64)  # continuous pixel coordinates, off both ends
    x.sort(axis=0)
    x[1] = np.where(rng.random(4 * n) < 0.7, np.minimum(x[1], x[0] + 3.0 * rng.random(4 * n)), x[1])
    half = (S1 - 1) / 2.0
    out.append((((half - x[1]) * pitch).astype(F32), ((half - x[0]) * pitch).astype(F32)))
    lo = np.concatenate([o[0] for o in out])
    hi = np.concatenate([o[1] for o in out])
    keep = lo <= hi
    return lo[keep], hi[keep]


@pytest.mark.parametrize("S1,S2", sorted(set(SIDES + [(b, a) for a, b in SIDES])))
@pytest.mark.parametrize("pad", PADS)
def test_range_is_a_tight_superset_of_the_exact_test(lib, S1, S2, pad):
    rng = np.random.default_rng(1000 * S1 + S2)
    xmin, xmax = boxes(S1, S2, rng)
    lo = (xmin - F32(pad)).astype(F32)  # as eval_face and the rectangles' callers form them
    hi = (xmax + F32(pad)).astype(F32)
    p0, p1 = pixel_ranges(lib, lo, hi, S1, S2)
    c = centres(S1, S2)
    p = np.arange(S1)
    kept = ~((c[None, :] > hi[:, None]) | (c[None, :] < lo[:, None]))
    inside = (p[None, :] >= p0[:, None]) & (p[None, :] <= p1[:, None])
    assert kept.any(), "degenerate fuzz: no box keeps a pixel"
    if pad == 0.0:  # (a pad of several pixels leaves no box between two centres)
        assert (~kept.any(axis=1)).any(), "degenerate fuzz: no box keeps nothing"
    missed = kept & ~inside
    assert not missed.any(), f"{int(missed.sum())} kept pixels outside the range, first box {np.argwhere(missed)[0]}"
    tol = 0.06 * float(ndc_range(S1, S2)) / S1
    c64 = c.astype(np.float64)[None, :]
    near = (c64 >= lo.astype(np.float64)[:, None] - tol) & (c64 <= hi.astype(np.float64)[:, None] + tol)
    loose = inside & ~near
    assert not loose.any(), f"{int(loose.sum())} listed pixels farther than 0.06 px from their box"
    # the range never leaves the image
    ne = p0 <= p1
    assert (p0[ne] >= 0).all() and (p1[ne] <= S1 - 1).all()


@pytest.mark.parametrize("S1,S2", SIDES)
@pytest.mark.parametrize("pad", PADS)
def test_boxes_off_the_image_give_an_empty_range(lib, S1, S2, pad):
    c = centres(S1, S2)
    pitch = float(ndc_range(S1, S2)) / S1
    rng = np.random.default_rng(7)
    gap = (0.1 + 3.0 * rng.random(64)) * pitch  # clear of the last centre by 0.1 px or more, pad included
    width = np.concatenate([rng.random(32) * 4 * pitch, 10.0 ** rng.uniform(-3, 3, 32)])
    # past pixel 0 (larger NDC) and past pixel S1 - 1 (smaller NDC)
    lo_a = float(c[0]) + pad + gap
    hi_b = float(c[-1]) - pad - gap
    xmin = np.concatenate([lo_a, hi_b - width]).astype(F32)
    xmax = np.concatenate([lo_a + width, hi_b]).astype(F32)
    lo = (xmin - F32(pad)).astype(F32)
    hi = (xmax + F32(pad)).astype(F32)
    assert not (~((c[None, :] > hi[:, None]) | (c[None, :] < lo[:, None]))).any()  # the exact test keeps nothing
    p0, p1 = pixel_ranges(lib, lo, hi, S1, S2)
    assert (p0 > p1).all(), f"{int((p0 <= p1).sum())} off-image boxes got a pixel range"


def test_bad_arguments(lib):
    p = ctypes.c_int32()
    assert lib.mr_pixel_range(0.0, 0.1, 16, 16, None, ctypes.byref(p)) == 1
    assert lib.mr_pixel_range(0.0, 0.1, 0, 16, ctypes.byref(p), ctypes.byref(p)) == 1
