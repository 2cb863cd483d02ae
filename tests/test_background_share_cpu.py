"""mr_binning_background_pixels (host only, no GPU): the pixels whose background the per-view binning launch
writes. bench.py's byte model reads it, and the launch sizes its share (``fill_first``) from the same
computation, in whole chunks: 64 lanes x 4 pixels when W % 4 == 0, else 64 pixels. So for every shape the
answer lies in [0, N H W] and is a whole number of chunks, or all N H W pixels (the last chunk of a view may
be partial). The grid includes the shapes of tests/test_gpu_background_partition.py."""
import itertools

import pytest

from torch_renderer_amd import _lib

SHAPES = [(8, 8), (20, 36), (7, 9), (64, 64), (96, 96), (128, 128), (512, 512), (30, 50), (1024, 1024)]
VIEWS = [1, 2, 3, 17, 20, 64, 264, 300]
FACES = [1, 80, 5856, 81920]


@pytest.mark.parametrize("mode", [0, 1])
def test_background_share_is_whole_chunks_within_the_image(mode):
    lib = _lib.load()
    seen_some = seen_none = False
    for (H, W), N, F in itertools.product(SHAPES, VIEWS, FACES):
        px = int(lib.mr_binning_background_pixels(N, F, H, W, mode))
        total = N * H * W
        chunk = 256 if W % 4 == 0 else 64
        assert 0 <= px <= total, (N, F, H, W, mode, px)
        assert px % chunk == 0 or px == total, (N, F, H, W, mode, px)
        seen_some |= px > 0
        seen_none |= px == 0
    assert seen_some and seen_none  # the grid reaches both sides: a share, and no spare workgroup (or no per-view binning)
    assert lib.mr_binning_background_pixels(0, 80, 64, 64, mode) == 0
    assert lib.mr_binning_background_pixels(4, 80, 0, 64, mode) == 0
