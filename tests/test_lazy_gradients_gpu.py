"""Lazy gradient images: a frame upload builds pyramid + statistics only; the Sobel images of levels 0..2 appear when an entry
point that reads them densely names the frame (hso_frame_require_gradients), and Matcher::checkNormal forms its four taps from the
level's pixels (sobel5_taps4).  Everything here is an equality of bits: against hso_gpu_frame_download_sobel, and against a
second context configured with eager_gradients = 1 (today's one-pass build, in the same binary).

Sizes: 64x64 takes the halfSample pyramid and the all-fast Sobel kernel; 68x76 the cv::resize pyramid, whose level 1 is 34 wide
(not a multiple of 4: the general Sobel kernel) and level 2 17x19."""
import math

import numpy as np
import pytest

from hso_amd import capi, synth

SIZES = [(64, 64), (68, 76)]          # (width, height)
PX_ERROR_ANGLE = math.atan(1.0 / (2.0 * 480.6)) * 2.0


def _images(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return {"random": np.random.default_rng(1000 * w + h).integers(0, 256, (h, w), dtype=np.uint8),
            "checker": ((((xs // 3) + (ys // 3)) & 1) * 255).astype(np.uint8),
            "constant": np.full((h, w), 93, np.uint8)}


@pytest.fixture(scope="module")
def images():
    return {s: _images(*s) for s in SIZES}


@pytest.fixture(scope="module")
def lazy():
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def eager():
    ctx = capi.Context(0)
    ctx.configure(eager_gradients=True)
    yield ctx
    ctx.close()


def _release(ctx, ids):
    for i in ids:
        try:
            ctx.frame_release(i)
        except capi.HsoGpuError:
            pass


def _same_detection(a, b):
    (co_a, cc_a, eo_a, ec_a), (co_b, cc_b, eo_b, ec_b) = a, b
    return (np.array_equal(cc_a, cc_b) and np.array_equal(ec_a, ec_b) and co_a.tobytes() == co_b.tobytes()
            and eo_a.tobytes() == eo_b.tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ["random", "checker", "constant"])
def test_taps_equal_the_gradient_images(lazy, images, size, name):
    """(a) the on-the-fly taps at every pixel of levels 0..2, all four positions of the 6x6 window, against the images
    hso_gpu_frame_download_sobel returns after materialisation: bit-equal int16, borders and corners included"""
    w, h = size
    _release(lazy, [100])
    lazy.frame_upload(100, images[size][name])
    try:
        taps = [lazy.debug_sobel_taps(100, l, w, h) for l in range(3)]      # before any gradient image exists
        for l in range(3):
            gx, gy = lazy.frame_sobel(100, l, w, h)
            lh, lw = gx.shape
            for k in range(4):
                dy, dx = k >> 1, k & 1
                assert np.array_equal(taps[l][0][k][:lh - dy, :lw - dx], gx[dy:, dx:]), (l, k)
                assert np.array_equal(taps[l][1][k][:lh - dy, :lw - dx], gy[dy:, dx:]), (l, k)
            if name == "constant":
                assert not gx.any() and not gy.any()
            else:
                assert gx.any() and gy.any()
    finally:
        _release(lazy, [100])


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("path", ["single", "batch"])
def test_lazy_equals_eager(lazy, eager, images, size, path):
    """(b) statistics byte-identical after upload and still after the materialisation; all six gradient images byte-identical"""
    w, h = size
    for name, img in images[size].items():
        _release(lazy, [200]); _release(eager, [200])
        if path == "single":
            st_l, st_e = lazy.frame_upload(200, img), eager.frame_upload(200, img)
        else:
            st_l, st_e = lazy.frame_upload_batch([200], imgs=[img])[0], eager.frame_upload_batch([200], imgs=[img])[0]
        try:
            assert bytes(st_l) == bytes(st_e), name
            assert bytes(lazy.debug_frame_stats(200)) == bytes(st_e)
            for l in range(3):
                gl, ge = lazy.frame_sobel(200, l, w, h), eager.frame_sobel(200, l, w, h)
                assert gl[0].tobytes() == ge[0].tobytes() and gl[1].tobytes() == ge[1].tobytes(), (name, l)
            assert bytes(lazy.debug_frame_stats(200)) == bytes(st_e), name     # the store pass left the statistics alone
            assert bytes(eager.debug_frame_stats(200)) == bytes(st_e)
        finally:
            _release(lazy, [200]); _release(eager, [200])


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_flag_follows_the_pixels(lazy, eager, images, size):
    """(c) refresh in place, a recycled allocation and a half-ready batch: candidate detection equals the eager context's"""
    w, h = size
    A, B = images[size]["random"], images[size]["checker"]
    ids = [300, 301, 302, 303]
    _release(lazy, ids); _release(eager, ids)
    try:
        eager.frame_upload_batch([300, 301], imgs=[B, A])
        want_B, want_A = eager.detect_candidates([300]), eager.detect_candidates([301])
        assert want_B[3].sum() > 0 and want_A[1].sum() > 0        # edgelets on the checkerboard, corners in the noise
        # X = 300 carries A with its gradient images, then is refreshed in place with B
        lazy.frame_upload_batch([300], imgs=[A])
        lazy.frame_sobel(300, 0, w, h)
        lazy.frame_upload_batch([300], imgs=[B])
        assert _same_detection(lazy.detect_candidates([300]), want_B)
        # its allocation (gradient images of B) goes back to the free list and comes out again for a new id with A
        lazy.frame_release(300)
        lazy.frame_upload(301, A)
        assert _same_detection(lazy.detect_candidates([301]), want_A)
        # one batch, one frame ready (302, through the download) and one not (303)
        lazy.frame_upload_batch([302, 303], imgs=[B, A])
        lazy.frame_sobel(302, 1, w, h)
        eager.frame_upload_batch([302, 303], imgs=[B, A])
        assert _same_detection(lazy.detect_candidates([302, 303]), eager.detect_candidates([302, 303]))
        assert _same_detection(lazy.detect_candidates([303, 302, 303]), eager.detect_candidates([303, 302, 303]))
    finally:
        _release(lazy, ids); _release(eager, ids)


@pytest.fixture(scope="module")
def scene(orc):
    d = synth.config2_pair(200, trans_frac=0.05)
    rp, cp = orc.create_pyramid(d["ref"]), orc.create_pyramid(d["cur"])
    sob = [orc.sobel5(cp[l]) for l in range(3)]
    gx0, gy0 = orc.sobel5(rp[0])
    return d, rp, cp, sob, gx0, gy0


@pytest.mark.gpu
def test_consumers_do_not_read_gradient_images(lazy, eager, orc, cam, scene):
    """(d) align and seed observation on frames that never had gradient images of their own (their allocations carry another
    image's): results equal the eager context's bit for bit, and edgelets did reach checkNormal in both calls"""
    d, rp, cp, sob, gx0, gy0 = scene
    ids = [400, 401, 402, 403]
    _release(lazy, ids); _release(eager, ids)
    try:
        # two allocations with the gradient images of other pictures, back on the free list
        lazy.frame_upload_batch([402, 403], imgs=[np.ascontiguousarray(d["ref"][::-1, ::-1]), np.ascontiguousarray(255 - d["cur"])])
        h, w = d["ref"].shape
        lazy.frame_sobel(402, 0, w, h); lazy.frame_sobel(403, 0, w, h)
        lazy.frame_release(402); lazy.frame_release(403)
        for ctx in (lazy, eager):
            ctx.frame_upload(400, d["ref"]); ctx.frame_upload(401, d["cur"])

        jobs = synth.align_jobs(d, 300, 400, gx=gx0, gy=gy0, seed=21)
        got_l, got_e = lazy.align_batch(cam, 401, jobs), eager.align_batch(cam, 401, jobs)
        assert b"".join(bytes(g) for g in got_l) == b"".join(bytes(g) for g in got_e)
        # an edgelet job whose LK converged went through checkNormal: every stage but "reference on the border" / "not converged"
        reached = [i for i, (j, g) in enumerate(zip(jobs, got_l)) if j.type == capi.FTR_EDGELET and g.stage not in (1, 2)]
        assert len(reached) > 0 and any(got_l[i].success for i in reached)
        n_cpu = 0
        for i in reached[:20]:                          # ... and the restatement evaluates the check's comparison for such jobs
            orc.margins_reset()
            orc.find_match_direct(cam, jobs[i], rp, cp, sob)
            n_cpu += orc.margins().normal < 1e299
        assert n_cpu > 0

        seeds, T_cur, feats = synth.seeds_for_pair(d, 300, 400, gx=gx0, gy=gy0)
        so_l = lazy.seed_observe(cam, 401, T_cur, 1.05, PX_ERROR_ANGLE, seeds)
        so_e = eager.seed_observe(cam, 401, T_cur, 1.05, PX_ERROR_ANGLE, seeds)
        assert b"".join(bytes(g) for g in so_l) == b"".join(bytes(g) for g in so_e)
        # an edgelet seed that was updated passed refineAlignment's checkNormal
        reached = [i for i, (s, g) in enumerate(zip(seeds, so_l)) if s.type == capi.FTR_EDGELET and g.result == 1]
        assert len(reached) > 0
        n_cpu = 0
        for i in reached[:20]:
            orc.margins_reset()
            orc.seed_observe(cam, seeds[i], T_cur, 1.05, PX_ERROR_ANGLE, rp, cp, sob)
            n_cpu += orc.margins().normal < 1e299
        assert n_cpu > 0
    finally:
        _release(lazy, ids); _release(eager, ids)
