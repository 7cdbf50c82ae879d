"""The shared per-call work area (ctx->d_batch, hso_batch_reserve) across a regrowth: what the call that grew it returns, and
what the calls after it return, equal bit for bit what a fresh context returns for the same call.

A step = upload from host images, then read everything back: the five levels, the six gradient images
(hso_gpu_frame_download_sobel; in a lazy context its first call of a context is the first to reserve the area: 8 bytes, i.e.
hso_grown(8) = 1 MiB + 12), the returned statistics, and the on-the-fly taps of levels 0..2 (hso_gpu_debug_sobel_taps).  The
taps are the read-back that is staged in the work area: 2 * 4 * W * H * 2 bytes per level, 64 KiB at 64x64 and 4.9 MB at
640x480 level 0.  So in the order 64x64, 640x480, 64x64 the second step's level-0 taps regrow the area (4.9 MB > 1 MiB + 12, or
> hso_grown(64 KiB) = 1.1 MB in an eager context, whose gradient download reserves nothing), its level-1 and -2 taps and the
whole third step run in the regrown one.  192x128 (0.39 MB) would not regrow it.

No capacity is read: only results are compared."""
import numpy as np
import pytest

from frame_ref import half_sample_exact, sobel5_exact, stats_exact, texture
from hso_amd import capi

pytestmark = pytest.mark.gpu

SMALL, LARGE = (64, 64), (640, 480)          # (width, height)
ORDER = [SMALL, LARGE, SMALL]


def _images(size, step, n):
    w, h = size
    return [texture(w, h, 16, 7000 + 100 * step + 10 * k + w) for k in range(n)]


def _context(mode):
    ctx = capi.Context(0)
    if mode == "eager":
        ctx.configure(eager_gradients=True)
    return ctx


def _read_back(ctx, fid, size):
    """everything a step reads of one frame, as bytes"""
    w, h = size
    out = [ctx.frame_level(fid, l, w, h).tobytes() for l in range(5)]
    for l in range(3):
        out += [g.tobytes() for g in ctx.frame_sobel(fid, l, w, h)]
    for l in range(3):
        out += [g.tobytes() for g in ctx.debug_sobel_taps(fid, l, w, h)]
    return out


def _step_single(ctx, size, step):
    img = _images(size, step, 1)[0]
    st = ctx.frame_upload(10 + step, img)
    return [bytes(st)] + _read_back(ctx, 10 + step, size)


def _detection(ctx, ids):
    return [np.ascontiguousarray(a).tobytes() for a in ctx.detect_candidates(ids)]


def _step_batch(ctx, size, step, detect_first):
    """three frames in one hso_gpu_frame_upload_batch; detect_first: one candidate detection on a 64x64 frame before it"""
    out = []
    if detect_first:
        ctx.frame_upload(90 + step, _images(SMALL, 50 + step, 1)[0])
        out += _detection(ctx, [90 + step])
    ids = [20 + 3 * step + k for k in range(3)]
    out += [bytes(st) for st in ctx.frame_upload_batch(ids, imgs=_images(size, step, 3))]
    for fid in ids:
        out += _read_back(ctx, fid, size)
    out += _detection(ctx, ids[:1])          # the same area, another entry point, after whatever growth the step caused
    return out


def _fresh(mode, step_fn, *args):
    ctx = _context(mode)
    try:
        return step_fn(ctx, *args)
    finally:
        ctx.close()


def _exact_64(img):
    """levels (halfSample: rounding averages while the input width is a multiple of 16, the truncating loop from 8 wide on),
    the six gradient images and integral_image of a 64x64 image, from frame_ref's exact forms"""
    levels = [img]
    for l in range(1, 5):
        levels.append(half_sample_exact(levels[-1], sse=levels[-1].shape[1] % 16 == 0))
    out = [lv.tobytes() for lv in levels]
    for l in range(3):
        out += [g.tobytes() for g in sobel5_exact(levels[l])]
    return out, stats_exact(img).integral_image


@pytest.mark.parametrize("mode", ["lazy", "eager"])
def test_regrowth_in_one_context(mode):
    ctx = _context(mode)
    try:
        for step, size in enumerate(ORDER):
            got = _step_single(ctx, size, step)
            want = _fresh(mode, _step_single, size, step)
            assert len(got) == len(want) == 1 + 5 + 6 + 6
            for k, (a, b) in enumerate(zip(got, want)):
                assert a == b, (mode, step, size, "field %d differs from the fresh context's" % k)
            if size == SMALL:
                exact, integral = _exact_64(_images(size, step, 1)[0])
                assert got[1:1 + 5 + 6] == exact, (mode, step)
                st = capi.FrameStats.from_buffer_copy(got[0])
                assert np.float32(st.integral_image).tobytes() == integral.tobytes(), (mode, step)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", ["lazy", "eager"])
def test_regrowth_across_entry_points(mode):
    ctx = _context(mode)
    try:
        for step, size in enumerate(ORDER):
            got = _step_batch(ctx, size, step, step == 1)
            want = _fresh(mode, _step_batch, size, step, step == 1)
            assert len(got) == len(want)
            for k, (a, b) in enumerate(zip(got, want)):
                assert a == b, (mode, step, size, "field %d differs from the fresh context's" % k)
    finally:
        ctx.close()
