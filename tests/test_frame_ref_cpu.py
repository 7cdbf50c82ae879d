"""Ties the CPU restatement (oracle/) to the exact references of frame_ref.py where test_frame_geometry_gpu.py leans on it
(pyramid levels), and states what the restatement's statistics are: the reference's serial fp32 loop, bit for bit — which is
why the device's gradient mean is compared with frame_ref.stats_exact and not with it.

Outcome of the bit-for-bit check of hso_or_frame_stats against a numpy-float32 restatement of src/frame.cpp:223-245 (one
np.float32 accumulator, row-major, every operation of sqrt(gx*gx + gy*gy) rounded to float32): equal at every small shape and
texture.  The parity build of the restatement uses -ffp-contract=off, so gx*gx + gy*gy is not contracted into a multiply-add."""
import numpy as np
import pytest

import frame_ref
from frame_ref import SMALL_SHAPES, TEXTURES, area2x2_exact, half_sample_exact, sobel5_exact, stats_exact, texture, texture_seed

SHAPES = list(SMALL_SHAPES)
IDS = ["%dx%d" % s for s in SHAPES]


def _img(size, name):
    return texture(size[0], size[1], TEXTURES[name], texture_seed(size[0], size[1], name))


@pytest.mark.parametrize("size", SHAPES, ids=IDS)
def test_oracle_sobel_equals_direct_convolution(orc, size):
    for name in ("k16", "noise"):
        lv = orc.create_pyramid(_img(size, name))
        for l in range(3):
            ox, oy = orc.sobel5(lv[l])
            ex, ey = sobel5_exact(lv[l])
            assert ox.dtype == ex.dtype and np.array_equal(ox, ex) and np.array_equal(oy, ey), (name, l)


def test_sobel_exact_on_hand_made_images():
    """the direct convolution itself: a horizontal ramp has gx = 2 * sum(|kd| / 2 * distance) * sum(ks) = 8 * 16 * slope inside
    and no gy; a single bright pixel reproduces the flipped kernel"""
    ramp = np.tile(np.arange(20, dtype=np.uint8) * 3, (12, 1))
    gx, gy = sobel5_exact(ramp)
    assert not gy.any() and (gx[:, 2:-2] == 8 * 16 * 3).all()
    assert (gx[:, 0] == (2 * 1 + 1 * 2) * 3 * 16).all()          # replicated left edge: taps at x = 1, 2 only
    dot = np.zeros((9, 9), np.uint8)
    dot[4, 4] = 1
    gx, gy = sobel5_exact(dot)
    kd, ks = np.array([-1, -2, 0, 2, 1]), np.array([1, 4, 6, 4, 1])
    assert np.array_equal(gx[2:7, 2:7], np.outer(ks, -kd)) and np.array_equal(gy[2:7, 2:7], np.outer(-kd, ks))


@pytest.mark.parametrize("size", SHAPES, ids=IDS)
def test_oracle_pyramid_levels(orc, size):
    branch, dims = SMALL_SHAPES[size]
    w, h = size
    assert branch == ("half" if w % 16 == 0 and h % 16 == 0 else "resize")
    for name in ("k16", "noise"):
        img = _img(size, name)
        lv = orc.create_pyramid(img)
        assert [l.shape for l in lv] == [(h, w)] + [(lh, lw) for lw, lh in dims]
        assert np.array_equal(lv[0], img)
        n_checked = 0
        for l in range(1, 5):
            pw, ph = lv[l - 1].shape[1], lv[l - 1].shape[0]
            if branch == "half":
                assert np.array_equal(lv[l], half_sample_exact(lv[l - 1], pw % 16 == 0)), (name, l)
                n_checked += 1
            elif (2 * lv[l].shape[1], 2 * lv[l].shape[0]) == (pw, ph):
                assert np.array_equal(lv[l], area2x2_exact(lv[l - 1])), (name, l)
                n_checked += 1
        assert n_checked >= (4 if branch == "half" else 2)         # every resize shape has at least levels 1 and 2 exact


def test_the_two_half_sample_roundings_differ():
    """a + b + c + d = 1: the SSE form rounds up twice (1), the scalar form truncates (0), the area form rounds once (0)"""
    img = np.zeros((2, 16), np.uint8)
    img[0, 0] = 1
    assert half_sample_exact(img, True)[0, 0] == 1 and half_sample_exact(img, False)[0, 0] == 0 and area2x2_exact(img)[0, 0] == 0
    img[1, 1] = 1
    assert half_sample_exact(img, True)[0, 0] == 1 and half_sample_exact(img, False)[0, 0] == 0 and area2x2_exact(img)[0, 0] == 1


def _serial_fp32_stats(img0, gx0, gy0):
    """src/frame.cpp:223-245 in numpy float32: one accumulator per sum, row-major, every operation rounded to float32"""
    h, w = img0.shape
    gx = gx0[16:h - 16, 16:w - 16].astype(np.float32)
    gy = gy0[16:h - 16, 16:w - 16].astype(np.float32)
    terms = np.sqrt(gx * gx + gy * gy)                              # float32 products, float32 sum, float32 root
    assert terms.dtype == np.float32
    px = img0[16:h - 16, 16:w - 16].astype(np.float32)
    grad_sum, int_sum, n = np.float32(0), np.float32(0), 0
    for t, p in zip(terms.ravel(), px.ravel()):
        grad_sum = grad_sum + t
        int_sum = int_sum + p
        n += 1
    gm = grad_sum / np.float32(n)
    gm = gm / np.float32(30)
    gm = min(max(gm, np.float32(7)), np.float32(20))
    return np.float32(int_sum / np.float32(n)), np.float32(gm)


@pytest.mark.parametrize("size", SHAPES, ids=IDS)
@pytest.mark.parametrize("name", list(TEXTURES))
def test_oracle_statistics_are_the_serial_fp32_loop(orc, size, name):
    img = _img(size, name)
    gx, gy = orc.sobel5(img)
    so = orc.frame_stats(img, gx, gy)
    ii, gm = _serial_fp32_stats(img, gx, gy)
    assert np.float32(so.integral_image).tobytes() == ii.tobytes()
    assert np.float32(so.grad_mean).tobytes() == gm.tobytes()
    assert (so.width, so.height) == size
    # ... and at these pixel counts (<= 15360 terms) the serial sum is still close to the exact one: n * 2^-24 in the worst case
    ex = stats_exact(img)
    n = (size[0] - 32) * (size[1] - 32)
    assert abs(float(gm) - float(ex.grad_mean)) <= n * 2.0 ** -24 * float(ex.grad_mean)
    assert abs(float(ii) - float(ex.integral_image)) <= n * 2.0 ** -24 * float(ex.integral_image)


@pytest.mark.parametrize("size", SHAPES, ids=IDS)
def test_textures_land_in_all_three_clamp_regimes(size):
    lo, mid, hi = (stats_exact(_img(size, name)) for name in ("k4", "k16", "noise"))
    assert lo.unclamped < 7 and lo.grad_mean == np.float32(7)
    assert 7.5 < mid.unclamped < 19.5 and float(mid.grad_mean) == pytest.approx(mid.unclamped, rel=2e-7)
    assert hi.unclamped > 20 and hi.grad_mean == np.float32(20)
    k24 = stats_exact(_img(size, "k24"))
    assert 7.5 < k24.unclamped < 19.5 and k24.grad_mean > mid.grad_mean
    for st in (lo, mid, hi):
        assert st.integral_image.dtype == np.float32 and st.grad_mean.dtype == np.float32
        assert (st.width, st.height) == size


def test_stats_exact_on_a_closed_form():
    """a horizontal ramp of slope 3: |grad| = 384 at every interior pixel, mean intensity = the ramp's centre"""
    ramp = np.tile((np.arange(80) * 3).astype(np.uint8), (72, 1))
    st = stats_exact(ramp)
    assert st.unclamped == pytest.approx(384 / 30, rel=1e-15) and st.grad_mean == np.float32(np.float32(384) / np.float32(30))
    assert st.integral_image == np.float32(3 * (16 + 63) / 2)
    flat = stats_exact(np.full((64, 64), 93, np.uint8))
    assert flat.unclamped == 0 and flat.grad_mean == np.float32(7) and flat.integral_image == np.float32(93)
    assert frame_ref.FrameStatsExact._fields == ("integral_image", "grad_mean", "unclamped", "width", "height")
