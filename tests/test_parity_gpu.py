"""GPU parity tests: the HIP path, called through the C-ABI (include/hso_gpu.h), against
the CPU restatement (oracle/) on the same seeded inputs.

Bar:
  bit-exact  — pyramid levels, Sobel images, reference patch cache, visibility masks,
               |residual| multisets, MAD thresholds, term / saturation counts, LM
               iteration counts and accept/reject sequences;
  tolerance  — H: 1e-5 * max|H| (the oracle itself accumulates H in 3-tier fp32);
               b: 1e-6 relative; E: 2e-4 relative against the oracle's serial fp32 sum
               (CoarseTracker.cpp:272; tens of thousands of fp32 adds) and 2e-6 against
               the fp64 sum of the same fp32 terms;
               pose: rotation <= 1e-6 rad, translation <= 1e-6 * scene depth (4 m);
               frame means: 2e-5 relative against the oracle's serial fp32 sums over 3e5 pixels — on the
               noise-plus-ramp and rendered images only, whose gradient mean is far above the clamp
               (both sides return 20.0: the assert covers the intensity mean and the clamp, nothing
               else); on the unclamped texture images: integral_image bit-equal and grad_mean 1e-6
               relative against frame_ref.stats_exact (exact integers, math.fsum), not the oracle.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from frame_ref import stats_exact, texture
from hso_amd import capi, synth

pytestmark = pytest.mark.gpu

H_TOL, B_TOL, E_TOL, E64_TOL = 1e-5, 1e-6, 2e-4, 2e-6


def upload_pair(ctx, d, ids):
    for i in ids:
        try:
            ctx.frame_release(i)
        except capi.HsoGpuError:
            pass
    return ctx.frame_upload(ids[0], d["ref"]), ctx.frame_upload(ids[1], d["cur"])


def pose_err(r_gpu, r_cpu):
    qg, tg = r_gpu.T_cur_ref.to_arrays()
    qc, tc = r_cpu.T_cur_ref.to_arrays()
    if qg @ qc < 0:
        qg = -qg
    return 2 * np.linalg.norm(qg - qc), np.linalg.norm(tg - tc)


# ------------------------------------------------------------------ frames
@pytest.mark.parametrize("spec", [synth.ICL_NUIM, synth.EUROC], ids=["640x480", "752x480"])
def test_frame_pyramid_sobel_stats(gpu_ctx, orc, spec):
    rng = np.random.default_rng(11)
    w, h = spec["width"], spec["height"]
    # random noise + smooth ramp: exercises both halfSample roundings (EuRoC: L0->L1 SSE2, then scalar)
    img = np.clip(rng.integers(0, 256, (h, w)) * 0.5 + np.linspace(0, 127, w)[None, :], 0, 255).astype(np.uint8)
    try:
        gpu_ctx.frame_release(900)
    except capi.HsoGpuError:
        pass
    st = gpu_ctx.frame_upload(900, img)
    lv = orc.create_pyramid(img)
    for l in range(5):
        assert np.array_equal(gpu_ctx.frame_level(900, l, w, h), lv[l]), "pyramid level %d" % l
    for l in range(3):
        gx, gy = gpu_ctx.frame_sobel(900, l, w, h)
        ox, oy = orc.sobel5(lv[l])
        assert np.array_equal(gx, ox) and np.array_equal(gy, oy), "sobel level %d" % l
    so = orc.frame_stats(lv[0], *orc.sobel5(lv[0]))
    assert st.integral_image == pytest.approx(so.integral_image, rel=2e-5)
    assert st.grad_mean == pytest.approx(so.grad_mean, rel=2e-5)
    assert (st.width, st.height) == (w, h)
    gpu_ctx.frame_release(900)
    # a second image whose gradient mean is NOT clamped (the one above: about 41, both sides return 20.0), against exact arithmetic
    tex = texture(w, h, 16, 1000 * w + h)
    ex = stats_exact(tex)
    assert 7.5 < ex.unclamped < 19.5
    st2 = gpu_ctx.frame_upload(900, tex)
    try:
        _assert_stats_exact(st2, ex)
        _assert_stats_exact(gpu_ctx.debug_frame_stats(900), ex)
        # No rel=2e-5 device-versus-oracle assert here: the oracle repeats the reference's serial fp32 sum over 2.8e5 / 3.2e5
        # terms and is itself 8.0e-5 (640x480) / 7.0e-5 (752x480) away from the exact gradient mean of this image, 1.4e-5 /
        # 1.3e-5 from the exact intensity mean (_oracle_distance below computes both); a perfect kernel would fail it.
        d_grad, d_int = _oracle_distance(orc, tex, ex)
        assert 2e-5 < d_grad < 1e-3 and d_int < 1e-3
    finally:
        gpu_ctx.frame_release(900)


def _release_if_resident(ctx, frame_id):
    try:
        ctx.frame_release(frame_id)
    except capi.HsoGpuError:
        pass


def _assert_stats_exact(st, ex):
    """device statistics of an unclamped image against frame_ref.stats_exact: the intensity mean bit for bit (exact integer sum,
    one fp64 division, one rounding on both sides), the gradient mean to 1e-6 (test_frame_geometry_gpu.py derives < 4e-7)"""
    assert 7.5 < ex.unclamped < 19.5
    assert np.float32(st.integral_image).tobytes() == ex.integral_image.tobytes(), (st.integral_image, ex.integral_image)
    dev = abs(st.grad_mean - float(ex.grad_mean)) / float(ex.grad_mean)
    print("grad_mean deviation %dx%d: %.3e" % (ex.width, ex.height, dev))
    assert dev <= 1e-6, (st.grad_mean, float(ex.grad_mean), dev)
    assert (st.width, st.height) == (ex.width, ex.height)


def _oracle_distance(orc, img, ex):
    """relative distance of the oracle's (serial fp32) statistics to the exact ones: (gradient mean, intensity mean).  A random
    walk of n = 3e5 .. 7e5 roundings of 2^-24 each predicts some 1e-5 .. 1e-4; the worst case n * 2^-24 is 0.02 .. 0.04."""
    so = orc.frame_stats(img, *orc.sobel5(img))
    d_grad = abs(so.grad_mean - float(ex.grad_mean)) / float(ex.grad_mean)
    d_int = abs(so.integral_image - float(ex.integral_image)) / float(ex.integral_image)
    print("oracle-to-exact distance %dx%d: grad_mean %.3e, integral_image %.3e" % (ex.width, ex.height, d_grad, d_int))
    return d_grad, d_int


def test_frame_batch_equals_single_and_device_source(gpu_ctx, orc):
    import torch
    rng = np.random.default_rng(12)
    imgs = [rng.integers(0, 256, (480, 640), dtype=np.uint8) for _ in range(5)]
    ids = list(range(910, 915))
    for i in ids:
        try:
            gpu_ctx.frame_release(i)
        except capi.HsoGpuError:
            pass
    st_b = gpu_ctx.frame_upload_batch(ids, imgs=imgs)
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    ids2 = list(range(920, 925))
    for i in ids2:
        try:
            gpu_ctx.frame_release(i)
        except capi.HsoGpuError:
            pass
    st_d = gpu_ctx.frame_upload_batch(ids2, device_ptrs=[t.data_ptr() for t in dev], width=640, height=480)
    for k, im in enumerate(imgs):
        lv = orc.create_pyramid(im)
        for l in range(5):
            assert np.array_equal(gpu_ctx.frame_level(ids[k], l, 640, 480), lv[l])
            assert np.array_equal(gpu_ctx.frame_level(ids2[k], l, 640, 480), lv[l])
        assert st_b[k].integral_image == st_d[k].integral_image and st_b[k].grad_mean == st_d[k].grad_mean
    # refresh in place: same id, new content
    gpu_ctx.frame_upload_batch(ids[:1], imgs=[imgs[3]])
    assert np.array_equal(gpu_ctx.frame_level(ids[0], 2, 640, 480), orc.create_pyramid(imgs[3])[2])
    for i in ids + ids2:
        gpu_ctx.frame_release(i)


def test_frame_errors(gpu_ctx):
    with pytest.raises(capi.HsoGpuError):
        gpu_ctx.frame_upload(930, np.zeros((736, 922), np.uint8))       # width not a multiple of 4
    with pytest.raises(capi.HsoGpuError):
        gpu_ctx.frame_upload(930, np.zeros((48, 64), np.uint8))         # smaller than 64x64
    gpu_ctx.frame_upload(931, np.zeros((64, 64), np.uint8))
    with pytest.raises(capi.HsoGpuError):
        gpu_ctx.frame_upload(931, np.zeros((64, 64), np.uint8))          # already resident
    gpu_ctx.frame_release(931)
    with pytest.raises(capi.HsoGpuError):
        gpu_ctx.frame_release(931)
    with pytest.raises(capi.HsoGpuError):
        gpu_ctx.frame_level(931, 0, 64, 64)


# ------------------------------------------------------------------ tracker: per call
@pytest.mark.parametrize("inv", [0, 1], ids=["forward", "inverse_comp"])
@pytest.mark.parametrize("n_key", ["pair2000", "pair200"])
def test_tracker_eval_parity(gpu_ctx, orc, cam, request, inv, n_key):
    d = request.getfixturevalue(n_key)
    st_r, st_c = upload_pair(gpu_ctx, d, (1, 2))
    rp, cp = orc.create_pyramid(d["ref"]), orc.create_pyramid(d["cur"])
    a0 = float(np.float32(st_c.integral_image / st_r.integral_image))
    p = capi.TrackParams(inv, 4, 1, 50)
    job = gpu_ctx.make_job(1, 2, d["feats"], capi.SE3.identity(), a0)
    tr = orc.Tracker(cam, p, rp, cp, d["feats"])
    rng = np.random.default_rng(3)
    for level in (4, 3, 2, 1):
        tr.set_level(level)
        for T, a in ((capi.SE3.identity(), a0), (orc.se3_exp(rng.normal(0, 2e-3, 6)), 1.02)):
            n, hu, ou, errs = tr.select(T, a, True)
            eo = tr.eval(T, a)
            orp, ovis = tr.cache()
            for rep in range(2):  # twice: results must not depend on timing
                go, grp, gvis, gerr = gpu_ctx.tracker_eval(cam, p, job, level, T, a, want_cache=True, want_errors=True)
                assert np.array_equal(grp, orp), "reference patch cache, level %d" % level
                assert np.array_equal(gvis, ovis)
                assert go.n_select == n and go.n_visible == int(ovis.sum())
                assert np.array_equal(np.sort(gerr[:n]), np.sort(errs)), "|residual| multiset"
                assert (go.huber, go.outlier) == (hu, ou), "MAD thresholds must be bit-identical"
                assert (go.n_terms, go.n_saturated) == (eo.n_terms, eo.n_saturated)
                Ho, Hg = np.array(eo.H[:]), np.array(go.H[:])
                assert np.abs(Ho - Hg).max() <= H_TOL * np.abs(Ho).max()
                bo, bg = np.array(eo.b[:]), np.array(go.b[:])
                assert np.abs(bo - bg).max() <= B_TOL * np.abs(bo).max()
                assert go.energy == pytest.approx(eo.energy, rel=E_TOL)
                assert go.energy_sum == pytest.approx(tr.energy_f64(), rel=E64_TOL)
        # caller-supplied thresholds (the LM loop's steady state)
        tr.set_thresholds(7.5, 22.5)
        eo = tr.eval(capi.SE3.identity(), a0)
        go, _, _, _ = gpu_ctx.tracker_eval(cam, p, job, level, capi.SE3.identity(), a0, huber=7.5, outlier=22.5)
        assert (go.n_terms, go.n_saturated) == (eo.n_terms, eo.n_saturated)
        # thousands of saturated terms add the same max_energy: the reference's serial fp32
        # sum drifts by ~4e-4 here, so only the fp64 sum of the same terms is a tight check
        assert go.energy == pytest.approx(eo.energy, rel=2e-3)
        assert go.energy_sum == pytest.approx(tr.energy_f64(), rel=E64_TOL)


def test_tracker_eval_euroc_radtan(gpu_ctx, orc):
    """752x480 with the EuRoC radtan model: odd level widths (47 at L4), distorted world2cam."""
    d = synth.config2_pair(500, spec=synth.EUROC, seed=99)
    camE = synth.camera(synth.EUROC)
    st_r, st_c = upload_pair(gpu_ctx, d, (3, 4))
    rp, cp = orc.create_pyramid(d["ref"]), orc.create_pyramid(d["cur"])
    p = capi.TrackParams(0, 4, 1, 50)
    job = gpu_ctx.make_job(3, 4, d["feats"], capi.SE3.identity(), 1.0)
    tr = orc.Tracker(camE, p, rp, cp, d["feats"])
    for level in (4, 1):
        tr.set_level(level)
        n, hu, ou, _ = tr.select(capi.SE3.identity(), 1.0)
        eo = tr.eval(capi.SE3.identity(), 1.0)
        go, _, _, _ = gpu_ctx.tracker_eval(camE, p, job, level, capi.SE3.identity(), 1.0)
        assert (go.huber, go.outlier, go.n_select) == (hu, ou, n)
        assert (go.n_terms, go.n_saturated) == (eo.n_terms, eo.n_saturated)
        assert np.abs(np.array(eo.H[:]) - np.array(go.H[:])).max() <= H_TOL * np.abs(np.array(eo.H[:])).max()
    ro = tr.run(capi.SE3.identity(), 1.0)
    rg = gpu_ctx.coarse_track_batch(camE, p, [job])[0]
    assert list(rg.iters) == list(ro.iters) and list(rg.accept_mask) == list(ro.accept_mask)
    rot, tra = pose_err(rg, ro)
    assert rot <= 1e-6 and tra <= 4e-6


ACCEPT_TOL_ROT, ACCEPT_TOL_TRANS = 5e-5, 2e-4    # BASELINE.md "stated tolerance": frames whose accept sequence differs from the serial-sum restatement's


@pytest.mark.parametrize("shape,n_scenes", [("euroc", 64), ("vga", 16)])
def test_accept_decisions_over_many_scenes(gpu_ctx, orc, shape, n_scenes):
    """Many distinct scenes x 4 motion-model starts each (256 frames at the metric's shape, 64 at BASELINE configs[1]'s).  The
    device sums the (bit-identical) fp32 energy terms in a fixed tree, the reference serially in fp32 (CoarseTracker.cpp:272,413),
    so an accept decision (:143) whose two energies lie within that serial sum's rounding noise can differ.  Asserted per frame:
      * the device reproduces the restatement that decides on the fp64 sum of the same terms (iterations, accept sequence, pose to
        1e-7) in at least 95 % of the frames (measured: 254 of 256 at 752x480, 62 of 64 at 640x480; in the others an accept test between two energies that agree to
        1e-8 flips, and the pose stays within the bound below);
      * where its accept sequence equals the serial-sum restatement's (the reference's arithmetic), the pose agrees to 1e-6 rad /
        4e-6 m; where it differs, the pose still agrees within
        5e-5 rad / 2e-4 m (both runs reach the same minimum along different iteration sequences; SURVEY App. C's end-to-end
        bound is 1e-4);
      * such frames are at most 15 % (measured: 8-12 %)."""
    spec = synth.EUROC if shape == "euroc" else synth.ICL_NUIM
    camS = synth.camera(spec)
    p = capi.TrackParams(0, 4, 1, 50)
    rng = np.random.default_rng(5)
    n_frames, n_diff, n_diff64, worst = 0, 0, 0, [0.0, 0.0]
    for k in range(n_scenes):
        d = synth.config2_pair(600, spec=spec, seed=4000 + 13 * k, exposure=float(rng.uniform(0.92, 1.08)),
                               trans_frac=float(rng.uniform(0.012, 0.028)), rot_deg=float(rng.uniform(0.3, 0.7)))
        upload_pair(gpu_ctx, d, (3, 4))
        rp, cp = orc.create_pyramid(d["ref"]), orc.create_pyramid(d["cur"])
        starts = [(capi.SE3.from_arrays(synth.rotvec_to_quat(rng.normal(0, np.deg2rad(0.05), 3)), rng.uniform(0.5, 1.2) * np.array(d["t_true"])),
                   float(np.float32(rng.uniform(0.95, 1.05)))) for _ in range(4)]
        got = gpu_ctx.coarse_track_batch(camS, p, [gpu_ctx.make_job(3, 4, d["feats"], T0, a0) for T0, a0 in starts])
        for (T0, a0), rg in zip(starts, got):
            ro = orc.Tracker(camS, p, rp, cp, d["feats"]).run(T0, a0)
            t64 = orc.Tracker(camS, p, rp, cp, d["feats"]); t64.decide_on_f64_sum(True)
            r64 = t64.run(T0, a0)
            n_frames += 1
            rot, tra = pose_err(rg, r64)
            if list(rg.iters) == list(r64.iters) and list(rg.accept_mask) == list(r64.accept_mask):
                assert rot <= 1e-7 and tra <= 4e-7, "scene %d" % k
            else:
                # the device's fp32 terms equal the restatement's to ~1e-9 of their sum, not bit for bit (tests above: E64_TOL):
                # an accept test between two energies closer than that — the last, negligible step of a level — can still flip
                n_diff64 += 1
                assert rot <= ACCEPT_TOL_ROT and tra <= ACCEPT_TOL_TRANS, ("scene %d vs f64-sum" % k, rot, tra)
            rot, tra = pose_err(rg, ro)
            if list(rg.iters) == list(ro.iters) and list(rg.accept_mask) == list(ro.accept_mask):
                assert rot <= 1e-6 and tra <= 4e-6, "scene %d" % k
            else:
                n_diff += 1
                assert rot <= ACCEPT_TOL_ROT and tra <= ACCEPT_TOL_TRANS, ("scene %d" % k, rot, tra)
                worst = [max(worst[0], rot), max(worst[1], tra)]
    print("%s: %d frames, %d with a different accept sequence (%.1f %%), worst pose gap among them %.2e rad / %.2e m; %d differ from the fp64-sum form" % (
        shape, n_frames, n_diff, 100.0 * n_diff / n_frames, worst[0], worst[1], n_diff64))
    assert n_diff <= 0.15 * n_frames
    assert n_diff64 <= n_frames // 20


def test_tracker_large_table_and_fov_camera(gpu_ctx, orc, cam):
    """3000 features (more rounds per thread than the benchmark shape, keys in memory on every
    level) and the FOV / ATAN camera model of the TUM-mono configuration (camera.cpp:196-221)."""
    d = synth.config2_pair(3000, seed=77)
    upload_pair(gpu_ctx, d, (7, 8))
    rp, cp = orc.create_pyramid(d["ref"]), orc.create_pyramid(d["cur"])
    p = capi.TrackParams(0, 4, 1, 50)
    job = gpu_ctx.make_job(7, 8, d["feats"], capi.SE3.identity(), 1.0)
    ro = orc.Tracker(cam, p, rp, cp, d["feats"]).run(capi.SE3.identity(), 1.0)
    rg = gpu_ctx.coarse_track_batch(cam, p, [job])[0]
    assert list(rg.iters) == list(ro.iters) and list(rg.accept_mask) == list(ro.accept_mask)
    assert list(rg.n_select) == list(ro.n_select) and rg.huber[4] == ro.huber[4]
    assert (rg.n_tracked, rg.n_terms_last, rg.n_saturated_last) == (ro.n_tracked, ro.n_terms_last, ro.n_saturated_last)
    rot, tra = pose_err(rg, ro)
    assert rot <= 1e-6 and tra <= 4e-6
    # FOV camera: the bearings come from a pinhole scene, so this is a parity case, not a tracking case
    camF = capi.make_camera(capi.CAM_FOV, 640, 480, 300.0, 300.0, 319.5, 239.5, d=(0.9, 0, 0, 0, 0), distortion=1)
    tr = orc.Tracker(camF, p, rp, cp, d["feats"][:1500])
    jobF = gpu_ctx.make_job(7, 8, d["feats"][:1500], capi.SE3.identity(), 1.0)
    for level in (3, 1):
        tr.set_level(level)
        n, hu, ou, _ = tr.select(capi.SE3.identity(), 1.0)
        eo = tr.eval(capi.SE3.identity(), 1.0)
        go, _, _, _ = gpu_ctx.tracker_eval(camF, p, jobF, level, capi.SE3.identity(), 1.0)
        assert (go.huber, go.outlier, go.n_select) == (hu, ou, n) and n > 1000
        assert (go.n_terms, go.n_saturated) == (eo.n_terms, eo.n_saturated)
        assert np.abs(np.array(eo.H[:]) - np.array(go.H[:])).max() <= H_TOL * np.abs(np.array(eo.H[:])).max()


# ------------------------------------------------------------------ tracker: full run
@pytest.mark.parametrize("inv", [0, 1], ids=["forward", "inverse_comp"])
def test_coarse_track_run_parity(gpu_ctx, orc, cam, pair2000, inv):
    d = pair2000
    st_r, st_c = upload_pair(gpu_ctx, d, (1, 2))
    rp, cp = orc.create_pyramid(d["ref"]), orc.create_pyramid(d["cur"])
    a0 = float(np.float32(st_c.integral_image / st_r.integral_image))
    p = capi.TrackParams(inv, 4, 1, 50)
    ro = orc.Tracker(cam, p, rp, cp, d["feats"]).run(capi.SE3.identity(), a0)
    job = gpu_ctx.make_job(1, 2, d["feats"], capi.SE3.identity(), a0)
    rg = gpu_ctx.coarse_track_batch(cam, p, [job])[0]
    assert rg.status == 0
    assert list(rg.iters) == list(ro.iters), "LM iteration counts per level"
    assert list(rg.accept_mask) == list(ro.accept_mask), "accept/reject sequences"
    assert list(rg.n_eval) == list(ro.n_eval) and list(rg.n_select) == list(ro.n_select)
    assert list(rg.huber) == list(ro.huber) and list(rg.outlier) == list(ro.outlier)
    assert (rg.n_tracked, rg.n_terms_last, rg.n_saturated_last) == (ro.n_tracked, ro.n_terms_last, ro.n_saturated_last)
    rot, tra = pose_err(rg, ro)
    assert rot <= 1e-6 and tra <= 4e-6, (rot, tra)
    assert rg.exposure_rat == pytest.approx(ro.exposure_rat, abs=2e-6)
    for l in (4, 3, 2, 1):
        assert rg.energy[l] == pytest.approx(ro.energy[l], rel=1e-4)
    # and it found the scene's true motion
    q, t = rg.T_cur_ref.to_arrays()
    assert np.linalg.norm(q - d["q_true"]) < 2e-4 and np.linalg.norm(t - d["t_true"]) < 2e-3


def test_coarse_track_batch_is_deterministic_and_order_free(gpu_ctx, orc, cam, pair2000, pair200):
    """Independent jobs in one launch: every job equals its solo result, bit for bit,
    whatever the batch composition (fixed reduction trees, no atomics on floats)."""
    st = upload_pair(gpu_ctx, pair2000, (1, 2))
    st2 = upload_pair(gpu_ctx, pair200, (5, 6))
    p = capi.TrackParams(0, 4, 1, 50)
    jA = gpu_ctx.make_job(1, 2, pair2000["feats"], capi.SE3.identity(), 1.0)
    jB = gpu_ctx.make_job(5, 6, pair200["feats"], capi.SE3.identity(), 1.0)
    jC = gpu_ctx.make_job(1, 2, pair2000["feats"][:700], capi.SE3.identity(), 1.04)
    # the one-workgroup-per-job shapes (a solo call would otherwise take the cooperative shape: tests/test_track_coop_gpu.py)
    from conftest import track_env
    with track_env(gpu_ctx, "one_wg"):
        solo = [gpu_ctx.coarse_track_batch(cam, p, [j])[0] for j in (jA, jB, jC)]
        batch = gpu_ctx.coarse_track_batch(cam, p, [jA, jB, jC] * 40)
    for i, r in enumerate(batch):
        s = solo[i % 3]
        assert bytes(r) == bytes(s), "job %d differs from its solo run" % i
    # small-N job vs oracle (S > 1 lane groups per feature)
    rp, cp = orc.create_pyramid(pair200["ref"]), orc.create_pyramid(pair200["cur"])
    ro = orc.Tracker(cam, p, rp, cp, pair200["feats"]).run(capi.SE3.identity(), 1.0)
    assert list(solo[1].iters) == list(ro.iters) and list(solo[1].accept_mask) == list(ro.accept_mask)
    rot, tra = pose_err(solo[1], ro)
    assert rot <= 1e-6 and tra <= 4e-6


@pytest.mark.parametrize("inv", [0, 1], ids=["forward", "inverse_comp"])
def test_coarse_track_large_batch_takes_the_two_launch_path(gpu_ctx, orc, cam, pair2000, pair200, inv):
    """A batch that fills the chip at least twice runs levels 4..2 on two 256-thread workgroups per CU and level 1 on one
    512-thread workgroup (hso_tracker.hip: track_launch): a different split of the same sums, so every job must still equal
    the CPU restatement's decisions and pose, equal its twins bit for bit, and agree with the one-launch path to rounding."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    upload_pair(gpu_ctx, pair2000, (1, 2)); upload_pair(gpu_ctx, pair200, (5, 6))
    p = capi.TrackParams(inv, 4, 1, 50)
    T0 = capi.SE3.from_arrays(synth.rotvec_to_quat(0.6 * np.deg2rad(0.5) * np.array([0.2, -0.7, 0.4])), 0.7 * np.array(pair2000["t_true"]))
    jobs = [gpu_ctx.make_job(1, 2, pair2000["feats"], T0, 1.04), gpu_ctx.make_job(5, 6, pair200["feats"], capi.SE3.identity(), 1.0),
            gpu_ctx.make_job(1, 2, pair2000["feats"][:900], capi.SE3.identity(), 1.0)]
    n = 2 * n_cu + 7
    batch = gpu_ctx.coarse_track_batch(cam, p, [jobs[i % 3] for i in range(n)])
    from conftest import track_env
    with track_env(gpu_ctx, "one_wg"):
        solo = [gpu_ctx.coarse_track_batch(cam, p, [j])[0] for j in jobs]         # one launch, 512 threads
    rp, cp = orc.create_pyramid(pair2000["ref"]), orc.create_pyramid(pair2000["cur"])
    ro = orc.Tracker(cam, p, rp, cp, pair2000["feats"]).run(T0, 1.04)
    for i, r in enumerate(batch):
        assert bytes(r) == bytes(batch[i % 3]), "job %d differs from its twin" % i
        assert r.status == 0 and list(r.iters) == list(solo[i % 3].iters) and list(r.accept_mask) == list(solo[i % 3].accept_mask)
        rot, tra = pose_err(r, solo[i % 3])
        assert rot <= 1e-6 and tra <= 4e-6
        assert list(r.huber) == pytest.approx(list(solo[i % 3].huber), rel=1e-5) and r.huber[4] == solo[i % 3].huber[4]
    r = batch[0]
    assert list(r.iters) == list(ro.iters) and list(r.accept_mask) == list(ro.accept_mask) and list(r.n_eval) == list(ro.n_eval)
    assert (r.n_tracked, r.n_terms_last, r.n_saturated_last) == (ro.n_tracked, ro.n_terms_last, ro.n_saturated_last)
    rot, tra = pose_err(r, ro)
    assert rot <= 1e-6 and tra <= 4e-6


def test_coarse_track_edge_cases(gpu_ctx, orc, cam, pair200):
    d = pair200
    upload_pair(gpu_ctx, d, (5, 6))
    rp, cp = orc.create_pyramid(d["ref"]), orc.create_pyramid(d["cur"])
    p = capi.TrackParams(0, 4, 1, 50)
    # empty feature table (CoarseTracker.cpp:53-54)
    r = gpu_ctx.coarse_track_batch(cam, p, [gpu_ctx.make_job(5, 6, d["feats"][:0], capi.SE3.identity(), 1.25)])[0]
    assert r.n_tracked == 0 and r.exposure_rat == 1.25 and list(r.T_cur_ref.q) == [0, 0, 0, 1]
    # no feature has a point: < 30 terms -> thresholds (5.2, 100), zero step, one iteration per level
    f = d["feats"].copy(); f["dist"] = -1
    r = gpu_ctx.coarse_track_batch(cam, p, [gpu_ctx.make_job(5, 6, f, capi.SE3.identity(), 1.0)])[0]
    ro = orc.Tracker(cam, p, rp, cp, f).run(capi.SE3.identity(), 1.0)
    assert list(r.iters) == list(ro.iters) == [0, 1, 1, 1, 1]
    assert r.huber[4] == np.float32(5.2) and r.outlier[4] == 100 and r.n_tracked == 0
    # ragged: features at the border / half invalid / far-off initial pose
    f = synth.Scene().features(np.array([0, 0, 0, 1.0]), np.zeros(3), 333, seed=5, margin=1, frac_invalid=0.5)
    T_bad = orc.se3_exp([0.3, -0.2, 0.1, 0.02, -0.03, 0.01])
    job = gpu_ctx.make_job(5, 6, f, T_bad, 0.8)
    r = gpu_ctx.coarse_track_batch(cam, p, [job])[0]
    ro = orc.Tracker(cam, p, rp, cp, f).run(T_bad, 0.8)
    assert list(r.iters) == list(ro.iters) and list(r.accept_mask) == list(ro.accept_mask)
    assert list(r.n_select) == list(ro.n_select) and r.huber[4] == ro.huber[4]
    # ~170 valid features and a poor start: the coarse levels' normal equations are
    # ill-conditioned, so the 1e-7 H differences grow to ~1e-6 in the pose handed to the next
    # level and its medians move in the 5th digit; decisions and counts still agree
    assert np.allclose(list(r.huber), list(ro.huber), rtol=1e-3)
    rot, tra = pose_err(r, ro)
    assert rot <= 1e-4 and tra <= 1e-3
    # relocalisation schedule: levels 4..0, 15 iterations (frame_handler_mono.cpp:366); level 0 does not
    # fit in LDS and takes the global-memory tap path
    p0 = capi.TrackParams(0, 4, 0, 15)
    r = gpu_ctx.coarse_track_batch(cam, p0, [gpu_ctx.make_job(5, 6, d["feats"], capi.SE3.identity(), 1.0)])[0]
    ro = orc.Tracker(cam, p0, rp, cp, d["feats"]).run(capi.SE3.identity(), 1.0)
    assert list(r.iters) == list(ro.iters) and list(r.accept_mask) == list(ro.accept_mask)
    assert r.huber[4] == ro.huber[4] and np.allclose(list(r.huber), list(ro.huber), rtol=1e-4)
    rot, tra = pose_err(r, ro)
    assert rot <= 1e-6 and tra <= 4e-6
    # errors: frame not resident, bad levels
    with pytest.raises(capi.HsoGpuError):
        gpu_ctx.coarse_track_batch(cam, p, [gpu_ctx.make_job(5, 777, d["feats"], capi.SE3.identity(), 1.0)])
    with pytest.raises(capi.HsoGpuError):
        gpu_ctx.coarse_track_batch(cam, capi.TrackParams(0, 5, 1, 50), [gpu_ctx.make_job(5, 6, d["feats"], capi.SE3.identity(), 1.0)])


def test_make_depth_ref_parity(gpu_ctx, orc):
    rng = np.random.default_rng(8)
    poses = [orc.se3_exp(rng.normal(0, 0.2, 6)) for _ in range(6)]
    T_ref = orc.se3_exp(rng.normal(0, 0.2, 6))
    n = 3000
    din = np.zeros(n, capi.DEPTH_REF_IN_DTYPE)
    din["has_point"] = rng.integers(0, 2, n)
    din["host_pose"] = rng.integers(0, 6, n)
    f = rng.normal(size=(n, 3)); f[:, 2] = np.abs(f[:, 2]) + 1
    din["host_f"] = f / np.linalg.norm(f, axis=1, keepdims=True)
    din["idist"] = rng.uniform(0.1, 1, n)
    din["idist"][:50] = -0.5
    og = gpu_ctx.make_depth_ref(din, poses, T_ref)
    oc = orc.make_depth_ref(din, poses, T_ref)
    assert np.array_equal(og == -1, oc == -1)
    assert np.allclose(og, oc, rtol=1e-14, atol=0)


def test_tracker_against_committed_golden(gpu_ctx):
    """HIP path vs tests/golden/tracker_small.json (no oracle call in this test)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mk", os.path.join(GOLDEN, "make_tracker_golden.py"))
    mk = importlib.util.module_from_spec(spec); spec.loader.exec_module(mk)
    g = json.load(open(os.path.join(GOLDEN, "tracker_small.json")))
    d = mk.case()
    cam = synth.camera(mk.SPEC)
    st_r, st_c = upload_pair(gpu_ctx, d, (7, 8))
    assert st_r.integral_image == pytest.approx(g["stats"][0], rel=2e-5)
    a0 = float(np.float32(g["stats"][2] / g["stats"][0]))
    for inv in (0, 1):
        r = gpu_ctx.coarse_track_batch(cam, capi.TrackParams(inv, 4, 1, 50),
                                       [gpu_ctx.make_job(7, 8, d["feats"], capi.SE3.identity(), a0)])[0]
        e = g["runs"][str(inv)]
        assert list(r.iters) == e["iters"] and [int(x) for x in r.accept_mask] == e["accept"]
        # the top level's thresholds depend only on the inputs: bit-exact; lower levels start from
        # the previous level's LM result (equal to ~1e-9), so their medians may move by float ulps
        assert float(r.huber[4]) == e["huber"][4] and list(r.n_select) == e["n_select"]
        assert np.allclose([float(x) for x in r.huber], e["huber"], rtol=1e-5)
        assert np.allclose(r.T_cur_ref.q[:], e["q"], atol=5e-7) and np.allclose(r.T_cur_ref.t[:], e["t"], atol=4e-6)
        assert r.n_tracked == e["n_tracked"]


# ------------------------------------------------------------------ size-independent properties
def test_full_size_properties(gpu_ctx, cam, pair2000):
    """At BASELINE's full size (640x480, N=2000): tracking ref against itself is a fixed point;
    the estimate is invariant to feature order; exposure scales out."""
    d = pair2000
    upload_pair(gpu_ctx, d, (1, 2))
    p = capi.TrackParams(0, 4, 1, 50)
    # (1) identical images: zero residual -> identity pose, exposure 1, no accepted motion
    r = gpu_ctx.coarse_track_batch(cam, p, [gpu_ctx.make_job(1, 1, d["feats"], capi.SE3.identity(), 1.0)])[0]
    assert np.allclose(r.T_cur_ref.q[:], [0, 0, 0, 1], atol=1e-9) and np.allclose(r.T_cur_ref.t[:], 0, atol=1e-8)
    assert abs(r.exposure_rat - 1) < 1e-6
    # (2) permuting the feature table changes only summation order
    perm = np.random.default_rng(0).permutation(len(d["feats"]))
    rA = gpu_ctx.coarse_track_batch(cam, p, [gpu_ctx.make_job(1, 2, d["feats"], capi.SE3.identity(), 1.0)])[0]
    rB = gpu_ctx.coarse_track_batch(cam, p, [gpu_ctx.make_job(1, 2, d["feats"][perm], capi.SE3.identity(), 1.0)])[0]
    assert list(rA.huber) == list(rB.huber) and list(rA.n_select) == list(rB.n_select)
    rot, tra = pose_err(rA, rB)
    assert rot <= 1e-6 and tra <= 4e-6
    # (3) the converged pose does not depend on the initial exposure guess
    rC = gpu_ctx.coarse_track_batch(cam, p, [gpu_ctx.make_job(1, 2, d["feats"], capi.SE3.identity(), 1.08)])[0]
    rot, tra = pose_err(rA, rC)
    assert rot <= 2e-5 and tra <= 2e-4 and abs(rA.exposure_rat - rC.exposure_rat) < 1e-4


# ------------------------------------------------------------------ cv::resize pyramid branch (TUM-mono 920x736)
TUM_MONO = dict(model=capi.CAM_PINHOLE, width=920, height=736, fx=0.349153 * 920 * 1.4, fy=0.436593 * 736 * 1.4, cx=459.5, cy=367.5)


def test_resize_branch_frame_and_tracker(gpu_ctx, orc):
    """A level-0 size that is not a multiple of 16: cv::resize pyramid (level 4 is 58x46, level 2 is
    230 wide = not a multiple of 4), Sobel, stats, the tracker on all levels and FAST-9."""
    d = synth.config2_pair(700, spec=TUM_MONO, seed=55)
    camT = synth.camera(TUM_MONO)
    w, h = 920, 736
    for i in (910, 911):
        try:
            gpu_ctx.frame_release(i)
        except capi.HsoGpuError:
            pass
    st_r, st_c = gpu_ctx.frame_upload(910, d["ref"]), gpu_ctx.frame_upload(911, d["cur"])
    try:
        rp, cp = orc.create_pyramid(d["ref"]), orc.create_pyramid(d["cur"])
        assert [l.shape for l in cp] == [(736, 920), (368, 460), (184, 230), (92, 115), (46, 58)]
        for l in range(5):
            assert np.array_equal(gpu_ctx.frame_level(911, l, w, h), cp[l]), "pyramid level %d" % l
        for l in range(3):
            gx, gy = gpu_ctx.frame_sobel(911, l, w, h)
            ox, oy = orc.sobel5(cp[l])
            assert np.array_equal(gx, ox) and np.array_equal(gy, oy), "sobel level %d" % l
        so = orc.frame_stats(cp[0], *orc.sobel5(cp[0]))
        # the reference sums 6.2e5 pixels serially in fp32 (frame.cpp:223-236): its own rounding
        # error grows with the pixel count; the device sum is an exact integer
        assert st_c.integral_image == pytest.approx(so.integral_image, rel=1e-4)
        ex_c = stats_exact(d["cur"])
        assert np.float32(st_c.integral_image).tobytes() == ex_c.integral_image.tobytes()
        assert st_c.grad_mean == pytest.approx(so.grad_mean, rel=1e-4)
        assert ex_c.unclamped > 20 and st_c.grad_mean == 20.0       # the rendered image is clamped (about 50): 20.0 against 20.0
        # an image whose gradient mean is not clamped, against exact arithmetic (the oracle's serial sum is 6.4e-5 away from it
        # on this image, 1.7e-5 on the intensity mean: no device-versus-oracle assert)
        tex = texture(w, h, 16, 1000 * w + h)
        ex = stats_exact(tex)
        assert 7.5 < ex.unclamped < 19.5
        _release_if_resident(gpu_ctx, 912)
        st_t = gpu_ctx.frame_upload(912, tex)
        try:
            _assert_stats_exact(st_t, ex)
            _assert_stats_exact(gpu_ctx.debug_frame_stats(912), ex)
            d_grad, d_int = _oracle_distance(orc, tex, ex)
            assert 2e-5 < d_grad < 1e-3 and d_int < 1e-3
        finally:
            gpu_ctx.frame_release(912)
        # tracker: per-level evaluation parity and the full run
        p = capi.TrackParams(0, 4, 1, 50)
        job = gpu_ctx.make_job(910, 911, d["feats"], capi.SE3.identity(), 1.0)
        tr = orc.Tracker(camT, p, rp, cp, d["feats"])
        for level in (4, 2):
            tr.set_level(level)
            n, hu, ou, _ = tr.select(capi.SE3.identity(), 1.0)
            eo = tr.eval(capi.SE3.identity(), 1.0)
            go, _, _, _ = gpu_ctx.tracker_eval(camT, p, job, level, capi.SE3.identity(), 1.0)
            assert (go.huber, go.outlier, go.n_select) == (hu, ou, n)
            assert (go.n_terms, go.n_saturated) == (eo.n_terms, eo.n_saturated)
        ro = tr.run(capi.SE3.identity(), 1.0)
        rg = gpu_ctx.coarse_track_batch(camT, p, [job])[0]
        assert list(rg.iters) == list(ro.iters) and list(rg.accept_mask) == list(ro.accept_mask)
        rot, tra = pose_err(rg, ro)
        assert rot <= 1e-6 and tra <= 4e-6
        # FAST-9 on the odd-sized levels
        levels, counts = gpu_ctx.fast_detect(911, n_levels=3, threshold=15, border=8, cap=60000)
        for L in range(3):
            want, n = orc.fast_detect_level(cp[L], 15, border=8)
            assert counts[L] == n and n > 20
            assert levels[L].tobytes() == want.tobytes()
    finally:
        gpu_ctx.frame_release(910); gpu_ctx.frame_release(911)


@pytest.mark.gpu
def test_frame_upload_resized_tum_mono(gpu_ctx, orc):
    """ImageReader::readImage's cv::resize to the downscaled camera size (1280x1024 -> 920x736, the
    size test/cameras/tum_mono_vo_*.txt yields) on the device, then the cv::resize pyramid."""
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:1024, 0:1280]
    img = (128 + 60 * np.sin(xx * 0.031) * np.cos(yy * 0.017) + rng.normal(0, 6, (1024, 1280))).clip(0, 255).astype(np.uint8)
    st = gpu_ctx.frame_upload_resized(9620, img, 920, 736)
    try:
        want0 = orc.resize_linear(img, 920, 736)
        pyr = orc.create_pyramid(want0)
        for L in range(5):
            got = gpu_ctx.frame_level(9620, L, 920, 736)
            assert got.shape == pyr[L].shape and (got == pyr[L]).all(), L
        gx, gy = orc.sobel5(np.ascontiguousarray(pyr[0]))
        ggx, ggy = gpu_ctx.frame_sobel(9620, 0, 920, 736)
        assert (ggx == gx).all() and (ggy == gy).all()
        assert st.width == 920 and st.height == 736
        # integer down-scales take the area-fast path; equal sizes are a plain upload
        half = img[:512, :640]
        st2 = gpu_ctx.frame_upload_resized(9621, half, 320, 256)
        assert (gpu_ctx.frame_level(9621, 0, 320, 256) == orc.resize_linear(half, 320, 256)).all()
        gpu_ctx.frame_release(9621)
        gpu_ctx.frame_upload_resized(9621, half, 640, 512)
        assert (gpu_ctx.frame_level(9621, 0, 640, 512) == half).all()
        gpu_ctx.frame_release(9621)
        with pytest.raises(capi.HsoGpuError):
            gpu_ctx.frame_upload_resized(9621, half, 322, 256)          # width % 4
    finally:
        gpu_ctx.frame_release(9620)
