"""Exact references for the frame build (pyramid, 5x5 Sobel, the two frame statistics) in plain numpy.

Nothing here imports the CPU restatement (oracle/) or the library: the restatement repeats the reference's serial fp32
accumulation of the two means (src/frame.cpp:223-245) and is itself 4e-5 .. 8e-5 away from the exact gradient mean on a
full-size image, so it cannot carry a 1e-6 comparison.  Here every integer is exact (int64) and the one floating-point sum is
math.fsum (correctly rounded)."""
import math
from collections import namedtuple

import numpy as np

GRAD_MEAN_LO, GRAD_MEAN_HI = np.float32(7), np.float32(20)       # the clamp of src/frame.cpp:242-245

# The small shapes of test_frame_geometry_gpu.py / test_frame_ref_cpu.py: (W, H) -> (pyramid branch, (w, h) of levels 1..4).
# Each is the smallest that reaches its case (the Sobel wavefront tile is 64 x 60, four tiles per block, 15-row strips):
SMALL_SHAPES = {
    # all-fast Sobel body: partial second tile row (rows 60-63), strips with ys >= H, one tile per block with three idle
    # waves; halfSample's SSE rounding three times (widths 64, 32, 16), then scalar
    (64, 64): ("half", [(32, 32), (16, 16), (8, 8), (4, 4)]),
    # 3 x 3 tiles = 3 blocks, the last with one live wave; interior mask across tile borders; right border mid-tile on levels 1, 2
    (192, 128): ("half", [(96, 64), (48, 32), (24, 16), (12, 8)]),
    # scalar rounding from level 1 on; 10- and 5-wide levels in k_pyramid's 2- and 1-byte stores; has_right false at x = 76
    (80, 96): ("half", [(40, 48), (20, 24), (10, 12), (5, 6)]),
    # all-fast Sobel body on a cv::resize pyramid (height not a multiple of 16); k_copy_level0 for device sources
    (64, 72): ("resize", [(32, 36), (16, 18), (8, 9), (4, 4)]),
    # general Sobel body: dword rows on level 0, byte path on levels 1 and 2 (odd width 17); bilinear step 17x19 -> 8x10
    (68, 76): ("resize", [(34, 38), (17, 19), (8, 10), (4, 5)]),
    # byte path with a clipped last lane (widths 50 and 25); bilinear step 25x17 -> 12x8
    (100, 68): ("resize", [(50, 34), (25, 17), (12, 8), (6, 4)]),
}
TEXTURES = {"k4": 4, "k16": 16, "k24": 24, "noise": None}       # name -> k of texture()
UNCLAMPED = ("k16", "k24")                                        # the textures whose gradient mean is inside (7, 20)


def texture_seed(w, h, name):
    return 1000 * w + h + 7 * list(TEXTURES).index(name)


FrameStatsExact = namedtuple("FrameStatsExact", "integral_image grad_mean unclamped width height")


def sobel5_exact(img):
    """cv::Sobel(CV_16S, ksize 5, BORDER_REPLICATE) as a direct 5x5 convolution in int64: derivative [-1 -2 0 2 1] (x) smoothing
    [1 4 6 4 1].  Returns (gx, gy) as int16 (|g| <= 16 * 6 * 255 = 24480)."""
    kd, ks = (-1, -2, 0, 2, 1), (1, 4, 6, 4, 1)
    img = np.asarray(img)
    h, w = img.shape
    p = np.pad(img.astype(np.int64), 2, mode="edge")
    gx = np.zeros((h, w), np.int64)
    gy = np.zeros((h, w), np.int64)
    for j in range(5):
        for i in range(5):
            win = p[j:j + h, i:i + w]
            gx += (ks[j] * kd[i]) * win
            gy += (kd[j] * ks[i]) * win
    assert max(np.abs(gx).max(), np.abs(gy).max()) <= 24480
    return gx.astype(np.int16), gy.astype(np.int16)


def _quads(img):
    h, w = img.shape
    v = np.asarray(img)[:h // 2 * 2, :w // 2 * 2].astype(np.int64)
    return v[0::2, 0::2], v[0::2, 1::2], v[1::2, 0::2], v[1::2, 1::2]    # a b / c d


def half_sample_exact(img, sse):
    """hso::halfSample (src/vikit/vision.cpp).  sse (the input width is a multiple of 16): _mm_avg_epu8 of the two rows, then
    _mm_avg_epu16 of the column pair, round-half-up both times; else the scalar loop, (a + b + c + d) / 4 truncated."""
    a, b, c, d = _quads(img)
    if sse:
        out = (((a + c + 1) >> 1) + ((b + d + 1) >> 1) + 1) >> 1
    else:
        out = (a + b + c + d) >> 2
    return out.astype(np.uint8)


def area2x2_exact(img):
    """cv::resize by exactly 2 in both directions (INTER_LINEAR is redirected to INTER_AREA's 2x2 path): (a + b + c + d + 2) >> 2"""
    a, b, c, d = _quads(img)
    return ((a + b + c + d + 2) >> 2).astype(np.uint8)


def stats_exact(img0):
    """integralImage_ and gradMean_ of a level-0 image over rows and columns [16, size - 16).

    integral_image = float32(exact integer sum / cnt): one fp64 division (both operands exact), one rounding.
    grad_mean: sqrt(float64(gx^2 + gy^2)) per pixel (the square sum is an exact integer < 2^31), math.fsum, / cnt, rounded to
    float32, / 30 in float32, clamped to [7, 20] in float32.  unclamped = mean / 30 as a float64, before any of that rounding."""
    img0 = np.asarray(img0)
    h, w = img0.shape
    cnt = (w - 32) * (h - 32)
    assert cnt > 0
    int_sum = int(img0[16:h - 16, 16:w - 16].astype(np.int64).sum())
    gx, gy = sobel5_exact(img0)
    gx = gx[16:h - 16, 16:w - 16].astype(np.int64)
    gy = gy[16:h - 16, 16:w - 16].astype(np.int64)
    mag_sum = math.fsum(np.sqrt((gx * gx + gy * gy).astype(np.float64)).ravel().tolist())
    gm = np.float32(mag_sum / cnt) / np.float32(30)
    assert gm.dtype == np.float32
    gm = min(max(gm, GRAD_MEAN_LO), GRAD_MEAN_HI)
    return FrameStatsExact(np.float32(int_sum / cnt), np.float32(gm), mag_sum / cnt / 30.0, w, h)


def texture(w, h, k, seed):
    """uint8(120 + U{-k..k} + x * 37 // w - y * 23 // h): noise of amplitude k on a shallow ramp.  The unclamped gradient mean
    follows k (about 0.68 k at the shapes the tests use): k = 4 clamps to 7, k = 12 .. 24 stays inside (7, 20).
    k = None: full-range noise U{0..255} (about 80, clamps to 20)."""
    rng = np.random.default_rng(seed)
    if k is None:
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    return (120 + rng.integers(-k, k + 1, (h, w)) + xs * 37 // w - ys * 23 // h).astype(np.uint8)
