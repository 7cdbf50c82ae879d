"""hso_gpu_klt_track_multi: the two-view initialisation's KLT for many frame pairs in one device call, and the engine's use of it
(Bank::initialise: one call per step for all sequences in their second stage).

What is checked, all of it exact (the kernels are integer arithmetic up to the per-point iteration, whose statements are the single
call's): a batch equals its pairs passed one by one, byte for byte; the image kernels (four pixels per lane, dword loads where
alignment allows, byte path on row tails) equal the restatement's pyrDown / Scharr at sizes whose levels leave 2- and 3-pixel
tails and have an odd height; argument errors are answered before anything reaches the device; a bank of four sequences started
from images equals its solo runs, issues ONE KLT call per step for all sequences in stage 2, and a traced sequence's klt_track
records replay through the single call."""
import ctypes as C

import numpy as np
import pytest

from hso_amd import capi, synth, vo

pytestmark = pytest.mark.gpu

E_INVALID, E_NOFRAME = -1, -2


def _census():
    out = np.zeros(8, np.int64)
    capi.load().hso_gpu_debug_census(out.ctypes.data_as(C.c_void_p), 8)
    return out


def _texture_images(w, h, seed, shifts):
    """synth's analytic texture sampled on grids shifted by (dx, dy): the same scene moving sideways"""
    sc = synth.Scene(dict(synth.EUROC, width=w, height=h), seed=seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    return [np.clip(np.rint(sc.texture(xs + dx, ys + dy)), 0, 255).astype(np.uint8) for dx, dy in shifts]


def _points(w, h, n, seed, border):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(border, w - border, n), rng.uniform(border, h - border, n)], 1).astype(np.float32)


def _upload(ctx, ids_imgs):
    for fid, img in ids_imgs:
        ctx.frame_upload(fid, img)


def _release(ctx, ids):
    for fid in ids:
        ctx.frame_release(fid)


def _batch_equals_singles(ctx, pairs, prev, init):
    got = ctx.klt_track_multi(pairs, prev, init)
    for fp, fc, first, n in pairs:
        one = ctx.klt_track_multi([(fp, fc, 0, n)], prev[first:first + n], init[first:first + n])
        assert one.tobytes() == got[first:first + n].tobytes(), (fp, fc, first, n)
        if n:
            single = ctx.klt_track(fp, fc, prev[first:first + n], init[first:first + n])   # the single call is the same batch of one
            assert single.tobytes() == one.tobytes()
    return got


def test_batch_equals_singles_byte_for_byte_at_188x150(gpu_ctx):
    w, h = 188, 150                                          # levels 188x150, 94x75, 47x38
    assert capi.load().hso_gpu_klt_levels(w, h, 30, 4) == 2
    im = _texture_images(w, h, 611, [(0, 0), (2.3, -1.1), (4.1, 0.7)])
    ids = [89001, 89002, 89003]
    _upload(gpu_ctx, zip(ids, im))
    try:
        # rows 0..299: pair 2; rows 300..336: pair 0; pair 1 owns nothing.  The ranges come in non-ascending order of `first`,
        # and pair 2's previous frame is pair 0's current one.
        pairs = [(ids[0], ids[1], 300, 37), (ids[1], ids[0], 300, 0), (ids[1], ids[2], 0, 300)]
        prev = np.zeros((337, 2), np.float32)
        prev[:300] = _points(w, h, 300, 5, 1)
        prev[300:] = _points(w, h, 37, 6, 1)
        # windows (30x30) that hang over every edge and both pairs of corners
        prev[:8] = [(0.5, 0.5), (w - 1.5, 0.5), (0.5, h - 1.5), (w - 1.5, h - 1.5), (w / 2, 1.0), (w / 2, h - 2.0), (1.0, h / 2), (w - 2.0, h / 2)]
        prev[300:304] = [(3.0, 4.0), (w - 4.0, 3.5), (2.5, h - 3.0), (w - 3.5, h - 4.5)]
        rng = np.random.default_rng(9)
        init = prev + rng.uniform(-3, 3, prev.shape).astype(np.float32)
        got = _batch_equals_singles(gpu_ctx, pairs, prev, init)
        tracked = (got["status"] & capi.KLT_TRACKED) != 0
        assert tracked[:300].mean() > 0.5 and tracked[300:].mean() > 0.5, (tracked[:300].mean(), tracked[300:].mean())   # the tracker did run
        # the work area has its size now: one more call = one upload, one download, one wait
        c0 = _census()
        again = gpu_ctx.klt_track_multi(pairs, prev, init)
        c1 = _census()
        assert again.tobytes() == got.tobytes()
        assert c1[0] - c0[0] == 2 and c1[3] - c0[3] == 1 and c1[5] == c0[5], (c1 - c0)
        # rows nobody owns come back zero
        gap = gpu_ctx.klt_track_multi([(ids[0], ids[1], 10, 5)], prev[:20], init[:20])
        assert not gap[:10].tobytes().strip(b"\0") and not gap[15:].tobytes().strip(b"\0")
        assert gap[10:15].tobytes() == gpu_ctx.klt_track(ids[0], ids[1], prev[10:15], init[10:15]).tobytes()
    finally:
        _release(gpu_ctx, ids)


def test_batch_equals_singles_at_the_euroc_size(gpu_ctx):
    w, h = 752, 480
    assert capi.load().hso_gpu_klt_levels(w, h, 30, 4) == 3  # four levels
    im = _texture_images(w, h, 612, [(0, 0), (3.2, 1.4), (-2.0, 2.5), (1.0, -3.0)])
    ids = [89011, 89012, 89013, 89014]
    _upload(gpu_ctx, zip(ids, im))
    try:
        pairs = [(ids[0], ids[1], 0, 200), (ids[2], ids[3], 200, 200)]
        prev = _points(w, h, 400, 15, 4)
        init = prev + np.random.default_rng(16).uniform(-3, 3, prev.shape).astype(np.float32)
        got = _batch_equals_singles(gpu_ctx, pairs, prev, init)
        assert ((got["status"] & capi.KLT_TRACKED) != 0).mean() > 0.8
    finally:
        _release(gpu_ctx, ids)


@pytest.mark.parametrize("size", [(188, 150), (64, 64)])
def test_image_kernels_equal_the_restatement(orc, gpu_ctx, size):
    w, h = size
    last = orc.klt_levels(w, h)
    assert last == {(188, 150): 2, (64, 64): 1}[size]
    img = _texture_images(w, h, 613, [(0, 0)])[0]
    gpu_ctx.frame_upload(89021, img)
    try:
        lvl = img
        for level in range(last + 1):
            if level:
                lvl = orc.pyr_down(lvl)
            g_img, g_der = gpu_ctx.klt_debug_level(89021, level, w, h)
            assert g_img.shape == lvl.shape and np.array_equal(g_img, lvl), level
            assert np.array_equal(g_der, orc.scharr_deriv(lvl)), level
    finally:
        gpu_ctx.frame_release(89021)


def test_argument_errors_come_before_any_launch(gpu_ctx):
    lib = capi.load()
    im = _texture_images(188, 150, 614, [(0, 0), (1, 1)])
    other = _texture_images(64, 64, 615, [(0, 0)])[0]
    ids = [89031, 89032, 89033]
    _upload(gpu_ctx, zip(ids, im + [other]))
    try:
        px = _points(188, 150, 20, 3, 10)
        out = np.zeros(20, capi.KLT_RESULT_DTYPE)

        def call(pairs, n_total=20, params=None):
            tab = np.zeros(max(len(pairs), 1), capi.KLT_PAIR_DTYPE)
            for i, p in enumerate(pairs):
                tab[i] = p
            params = params or capi.KltParams()
            c0 = _census()
            rc = lib.hso_gpu_klt_track_multi(gpu_ctx.h, capi._ptr(tab), len(pairs), capi._ptr(px), capi._ptr(px), n_total, C.byref(params), capi._ptr(out))
            c1 = _census()
            return rc, (c1 - c0)[[0, 3, 5]]                      # copies, waits, memsets the call made

        cases = {
            "overlapping ranges": (call([(ids[0], ids[1], 0, 12), (ids[0], ids[1], 11, 9)]), E_INVALID),
            "a range past n_total": (call([(ids[0], ids[1], 0, 10), (ids[0], ids[1], 10, 11)]), E_INVALID),
            "a negative count": (call([(ids[0], ids[1], 0, -1)]), E_INVALID),
            "frames of two sizes": (call([(ids[0], ids[1], 0, 10), (ids[2], ids[2], 10, 10)]), E_INVALID),
            "a missing frame": (call([(ids[0], ids[1], 0, 10), (ids[0], 89039, 10, 10)]), E_NOFRAME),
            "a missing frame of a pair without rows": (call([(ids[0], ids[1], 0, 10), (89039, ids[0], 10, 0)]), E_NOFRAME),
            "a window of 40": (call([(ids[0], ids[1], 0, 20)], params=capi.KltParams(win_size=40)), E_INVALID),
        }
        for what, ((rc, work), want) in cases.items():
            assert rc == want, (what, rc)
            assert not work.any(), (what, work)                 # the upload precedes the first launch: no copy, nothing launched
        rc, work = call([], n_total=0)
        assert rc == 0 and not work.any()                       # n_pairs = 0: OK, and nothing to do
        rc, work = call([(ids[0], ids[1], 0, 20)])              # the call the cases were variations of is a good one
        assert rc == 0 and work[0] == 2
    finally:
        _release(gpu_ctx, ids)


def test_bank_started_from_images_tracks_all_its_sequences_in_one_call(gpu_ctx, tmp_path):
    """Four sequences started with multi.start() (the sequences and step sizes of tests/test_multi_gpu.py's two-sequence test, two
    more seeds): every status record equals the solo run's; per step, all sequences in stage 2 share ONE KLT call; one traced
    sequence's klt_track records replay through hso_gpu_klt_track bit for bit.

    Kind [9] of the call counts also holds the detector calls and the depth filter's previous-frame pass, which sequences in
    stage 1 and 3 issue.  So the growth is asserted exactly — one call, as many items as sequences in stage 2 — for the steps in
    which at least two sequences are in stage 2 and no sequence is in another stage, and for the remaining steps with at least
    two in stage 2 the condition that follows from it whatever else was called (every call carries at least one item): items
    exceed calls by at least the stage-2 sequences less one."""
    spec = dict(synth.EUROC, texture_om=((0.004, 0.05), (0.05, 0.6)))
    cam = synth.camera(spec)
    steps = [(0.05, 0.015, 0.01), (0.07, 0.01, 0.015)]
    n_seq, n_frames = 4, 22
    seqs = [synth.sequence(n_frames, spec=spec, seed=4100 + 13 * k, step=steps[k % 2], rot_deg_per_frame=(0.05, -0.1, 0.03)) for k in range(n_seq)]
    solo = []
    for S in seqs:
        odo = vo.VisualOdometry(cam, 200)
        odo.start()
        solo.append([bytes(odo.add_image(im, float(k))) for k, im in enumerate(S["images"])])
        odo.close()
    traced = 2
    trace = str(tmp_path / "klt_trace.bin")
    multi = vo.MultiVisualOdometry(cam, n_seq, 200)
    multi.start()
    multi.trace(traced, trace)
    got = [[] for _ in range(n_seq)]
    exact_steps = shared_steps = 0
    for k in range(n_frames):
        stage = [multi.status(q).stage for q in range(n_seq)]
        n2 = sum(1 for s in stage if s == 2)
        c0 = multi.call_counts()["other"]
        multi.add_images([S["images"][k] for S in seqs], [float(k)] * n_seq)
        c1 = multi.call_counts()["other"]
        d_calls, d_items = c1[0] - c0[0], c1[1] - c0[1]
        if n2 >= 2:
            shared_steps += 1
            print("step %d: stages %s, kind [9] grew by %d calls / %d items" % (k, stage, d_calls, d_items))
            assert d_items - d_calls >= n2 - 1, (k, stage, d_calls, d_items)
            if n2 == n_seq:
                exact_steps += 1
                assert (d_calls, d_items) == (1, n2), (k, stage, d_calls, d_items)
        for q in range(n_seq):
            got[q].append(bytes(multi.status(q)))
    multi.trace(traced, None)
    final = [multi.status(q).stage for q in range(n_seq)]
    multi.close()
    assert final == [3] * n_seq and exact_steps >= 2 and shared_steps >= exact_steps, (final, exact_steps, shared_steps)
    for q in range(n_seq):
        for k, (a, b) in enumerate(zip(got[q], solo[q])):
            assert a == b, "sequence %d frame %d differs from its solo run" % (q, k)
    # ---- the traced sequence's KLT records through the single call (frame id = sequence << 32 | image index)
    recs = [r for call, r in vo.read_trace(trace) if call == "klt_track"]
    init_at = next(k for k, b in enumerate(got[traced]) if vo.VoStatus.from_buffer_copy(b).stage == 3)
    assert len(recs) == init_at                                 # frames 1 .. init_at ran the second stage
    for r in recs:
        fp, fc = int(vo.scalar(r, "prev_frame_id")), int(vo.scalar(r, "cur_frame_id"))
        assert fp >> 32 == traced and fc >> 32 == traced
        a = np.frombuffer(r["px_prev"], np.float32).reshape(-1, 2); b = np.frombuffer(r["px_init"], np.float32).reshape(-1, 2)
        _upload(gpu_ctx, [(89041, seqs[traced]["images"][fp & 0xffffffff]), (89042, seqs[traced]["images"][fc & 0xffffffff])])
        try:
            res = gpu_ctx.klt_track(89041, 89042, a, b, capi.KltParams.from_buffer_copy(r["params"]))
        finally:
            _release(gpu_ctx, [89041, 89042])
        assert len(a) > 100 and res.tobytes() == r["result"]
