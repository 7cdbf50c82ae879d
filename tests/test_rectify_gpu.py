"""Image rectification on the device (hso_amd/csrc/hso_rectify.hip) against its host definition hso_gpu_rectify_host and the numpy
restatement tests/rectify_ref.py, byte for byte; the batch entry, the map upload, the resize in front, the error codes; the
engine with hso_vo_options.rectify against the same engine fed host-rectified images, bit for bit; run_sequence on a stand-in
folder with the wide TUM camera file."""
import ctypes as C
import os

import numpy as np
import pytest

import rectify_ref as ref
from conftest import ROOT
from hso_amd import capi, formats, synth, vo

pytestmark = pytest.mark.gpu


def _stats(st):
    return (st.integral_image, st.grad_mean, st.width, st.height)


def _cases():
    """name -> (w, h, xy, frac): the hand-made map at both small shapes, the border camera, one Equidistant camera at 752x480, TUM wide"""
    out = {}
    for w, h in ((64, 64), (68, 66)):
        out["handmade_%dx%d" % (w, h)] = (w, h) + ref.handmade_map(w, h, seed=w)
    for name, cam in (("border_68x66", ref.border_camera()), ("equidistant_752x480", ref.equidistant_752()), ("tum_wide_920x736", ref.tum_wide())):
        out[name] = (cam.width, cam.height) + ref.build_map(cam)
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.fixture()
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", ["handmade_64x64", "handmade_68x66", "border_68x66", "equidistant_752x480", "tum_wide_920x736"])
def test_kernel_equals_host_definition(ctx, cases, name):
    w, h, xy, frac = cases[name]
    img = np.random.default_rng(3).integers(0, 256, (h, w), dtype=np.uint8)
    want = capi.rectify_host(xy, frac, img)
    assert np.array_equal(want, ref.remap(xy, frac, img))
    m = ctx.rectify_map_create(xy=xy, frac=frac)
    st = ctx.frame_upload_rectified(1, img, m)
    got = ctx.frame_level(1, 0, w, h)
    assert np.array_equal(got, want), "%d bytes differ, first at %s" % (int((got != want).sum()), np.argwhere(got != want)[:3].tolist())
    # everything behind level 0 is the plain frame build of the rectified image
    st_plain = ctx.frame_upload(2, want)
    assert _stats(st) == _stats(st_plain)
    assert np.array_equal(ctx.frame_level(1, 1, w, h), ctx.frame_level(2, 1, w, h))
    # the all-255 image: no weight sum overflows, no byte exceeds 255, four live taps give 255 back
    flat = np.full((h, w), 255, np.uint8)
    ctx.frame_upload_rectified(3, flat, m)
    assert np.array_equal(ctx.frame_level(3, 0, w, h), capi.rectify_host(xy, frac, flat))
    # a device image takes the same path
    import torch
    d_img = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    ctx.frame_upload_rectified(4, None, m, device_ptr=d_img.data_ptr(), width=w, height=h)
    assert np.array_equal(ctx.frame_level(4, 0, w, h), want)


def test_map_upload_reads_back(ctx):
    cam = ref.border_camera()
    xy, frac = capi.rectify_build_map(cam)
    m = ctx.rectify_map_create(cam=cam)
    xy_d, frac_d = ctx.rectify_map_read(m, cam.width, cam.height)
    assert np.array_equal(xy_d, xy) and np.array_equal(frac_d, frac)
    assert np.array_equal(xy, ref.build_map(cam)[0]) and np.array_equal(frac, ref.build_map(cam)[1])
    m2 = ctx.rectify_map_create(xy=xy[:, :64].copy(), frac=frac[:, :64].copy())     # a second map lives beside the first
    assert m2 != m
    assert np.array_equal(ctx.rectify_map_read(m, cam.width, cam.height)[0], xy)
    assert np.array_equal(ctx.rectify_map_read(m2, 64, cam.height)[1], frac[:, :64])


@pytest.mark.parametrize("name", ["border_68x66", "equidistant_752x480"])
def test_batch_equals_single_frames(ctx, cases, name):
    import torch
    w, h, xy, frac = cases[name]
    m = ctx.rectify_map_create(xy=xy, frac=frac)
    rng = np.random.default_rng(8)
    imgs = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(9)]
    single, single_st = [], []
    for i, im in enumerate(imgs):
        single_st.append(_stats(ctx.frame_upload_rectified(1000 + i, im, m)))
        single.append(ctx.frame_level(1000 + i, 0, w, h))
        assert np.array_equal(single[i], capi.rectify_host(xy, frac, im))
    next_id = 1
    for n in (1, 3, 9):                      # 9 = two full groups of frames per lane and a partial one
        for on_device in (False, True):
            ids = list(range(next_id, next_id + n))
            next_id += n
            if on_device:
                d = [torch.from_numpy(im).cuda() for im in imgs[:n]]
                torch.cuda.synchronize()
                st = ctx.frame_upload_batch_rectified(ids, m, device_ptrs=[t.data_ptr() for t in d])
            else:
                st = ctx.frame_upload_batch_rectified(ids, m, imgs=imgs[:n])
            for i, fid in enumerate(ids):
                assert np.array_equal(ctx.frame_level(fid, 0, w, h), single[i]), (n, on_device, i)
                assert np.array_equal(ctx.frame_level(fid, 2, w, h), ctx.frame_level(1000 + i, 2, w, h))
                assert _stats(st[i]) == single_st[i]
    # device images without statistics: the asynchronous form
    d = [torch.from_numpy(im).cuda() for im in imgs]
    torch.cuda.synchronize()
    ids = list(range(500, 509))
    assert ctx.frame_upload_batch_rectified(ids, m, device_ptrs=[t.data_ptr() for t in d], want_stats=False) is None
    ctx.synchronize()
    for i, fid in enumerate(ids):
        assert np.array_equal(ctx.frame_level(fid, 0, w, h), single[i])
        assert _stats(ctx.debug_frame_stats(fid)) == single_st[i]
    # refreshing resident ids in place, mixed with a new one
    ctx.frame_upload_batch_rectified([500, 777, 501], m, imgs=[imgs[4], imgs[5], imgs[6]])
    for fid, i in ((500, 4), (777, 5), (501, 6), (502, 2)):
        assert np.array_equal(ctx.frame_level(fid, 0, w, h), single[i])
    # a bad entry in the middle leaves nothing new resident, and what was resident as it was
    idsb = np.array([9001, 9002, 9003], np.int64)
    ptrs = np.array([imgs[0].ctypes.data, 0, imgs[2].ctypes.data], np.uint64)
    rc = ctx.lib.hso_gpu_frame_upload_batch_rectified(ctx.h, capi._ptr(idsb), capi._ptr(ptrs), 3, m, 0, None)
    assert rc == capi.E_INVALID
    out = np.zeros((h, w), np.uint8)
    for fid in (9001, 9002, 9003):
        assert ctx.lib.hso_gpu_frame_download_level(ctx.h, fid, 0, capi._ptr(out), None, None) == -2     # HSO_E_NOFRAME
    idsb = np.array([9001, 9001], np.int64)                                                                # a new id twice
    ptrs = np.array([imgs[0].ctypes.data, imgs[1].ctypes.data], np.uint64)
    assert ctx.lib.hso_gpu_frame_upload_batch_rectified(ctx.h, capi._ptr(idsb), capi._ptr(ptrs), 2, m, 0, None) == capi.E_INVALID
    assert ctx.lib.hso_gpu_frame_download_level(ctx.h, 9001, 0, capi._ptr(out), None, None) == -2
    assert np.array_equal(ctx.frame_level(500, 0, w, h), single[4])


def test_resize_in_front(ctx, cases):
    w, h, xy, frac = cases["tum_wide_920x736"]
    big = np.random.default_rng(21).integers(0, 256, (1024, 1280), dtype=np.uint8)
    m = ctx.rectify_map_create(cam=ref.tum_wide())
    ctx.frame_upload_resized(1, big, w, h)
    want = capi.rectify_host(xy, frac, ctx.frame_level(1, 0, w, h))
    st = ctx.frame_upload_rectified(2, big, m)
    assert (st.width, st.height) == (w, h)
    assert np.array_equal(ctx.frame_level(2, 0, w, h), want)


def test_error_codes(ctx, cases):
    w, h, xy, frac = cases["border_68x66"]
    lib, P = ctx.lib, capi._ptr
    mid = C.c_int32(-7)
    img = np.zeros((h, w), np.uint8)
    st = capi.FrameStats()
    # map creation: cameras the reference does not rectify, NULL arguments, the size rules of the uploads
    pin = capi.make_camera(capi.CAM_PINHOLE, 640, 480, 480, 480, 320, 240)
    fov_d = capi.make_camera(capi.CAM_FOV, 640, 480, 300, 300, 320, 240, d=[0.9], distortion=1)
    assert lib.hso_gpu_rectify_map_create(ctx.h, C.byref(pin), C.byref(mid)) == capi.E_INVALID
    assert lib.hso_gpu_rectify_map_create(ctx.h, C.byref(fov_d), C.byref(mid)) == capi.E_INVALID
    assert lib.hso_gpu_rectify_map_create(ctx.h, None, C.byref(mid)) == capi.E_INVALID
    assert lib.hso_gpu_rectify_map_create(ctx.h, C.byref(ref.border_camera()), None) == capi.E_INVALID
    assert lib.hso_gpu_rectify_map_create(None, C.byref(ref.border_camera()), C.byref(mid)) == capi.E_INVALID
    odd = capi.make_camera(capi.CAM_EQUIDISTANT, 66, 66, 30, 30, 33, 33, d=[0.1, 0, 0, 0], distortion=0)       # width % 4
    small = capi.make_camera(capi.CAM_EQUIDISTANT, 64, 60, 30, 30, 32, 30, d=[0.1, 0, 0, 0], distortion=0)     # < 64
    assert lib.hso_gpu_rectify_map_create(ctx.h, C.byref(odd), C.byref(mid)) == capi.E_INVALID
    assert lib.hso_gpu_rectify_map_create(ctx.h, C.byref(small), C.byref(mid)) == capi.E_INVALID
    assert lib.hso_gpu_rectify_map_create_tables(ctx.h, w, h, None, P(frac), C.byref(mid)) == capi.E_INVALID
    assert lib.hso_gpu_rectify_map_create_tables(ctx.h, w, h, P(xy), None, C.byref(mid)) == capi.E_INVALID
    assert lib.hso_gpu_rectify_map_create_tables(ctx.h, w, h, P(xy), P(frac), None) == capi.E_INVALID
    assert lib.hso_gpu_rectify_map_create_tables(ctx.h, 66, h, P(xy), P(frac), C.byref(mid)) == capi.E_INVALID
    assert lib.hso_gpu_rectify_map_create_tables(ctx.h, 64, 60, P(xy), P(frac), C.byref(mid)) == capi.E_INVALID
    assert mid.value == -7
    m = ctx.rectify_map_create(xy=xy, frac=frac)
    # unknown map, NULL image, bad sizes, a resident id
    for bad in (-1, m + 1, 12345):
        assert lib.hso_gpu_frame_upload_rectified(ctx.h, 1, P(img), w, h, bad, 0, C.byref(st)) == capi.E_INVALID
        assert lib.hso_gpu_rectify_map_destroy(ctx.h, bad) == capi.E_INVALID
        assert lib.hso_gpu_rectify_map_read(ctx.h, bad, P(xy), P(frac)) == capi.E_INVALID
    assert lib.hso_gpu_frame_upload_rectified(ctx.h, 1, None, w, h, m, 0, C.byref(st)) == capi.E_INVALID
    assert lib.hso_gpu_frame_upload_rectified(ctx.h, 1, P(img), 0, h, m, 0, C.byref(st)) == capi.E_INVALID
    assert lib.hso_gpu_frame_upload_rectified(None, 1, P(img), w, h, m, 0, C.byref(st)) == capi.E_INVALID
    assert lib.hso_gpu_rectify_map_read(ctx.h, m, None, P(frac)) == capi.E_INVALID
    ctx.frame_upload_rectified(1, img, m)
    assert lib.hso_gpu_frame_upload_rectified(ctx.h, 1, P(img), w, h, m, 0, C.byref(st)) == capi.E_INVALID     # already resident
    # batch: NULL arguments, n <= 0, a resident frame of another size than the map
    ids = np.array([5], np.int64)
    ptrs = np.array([img.ctypes.data], np.uint64)
    assert lib.hso_gpu_frame_upload_batch_rectified(ctx.h, None, P(ptrs), 1, m, 0, None) == capi.E_INVALID
    assert lib.hso_gpu_frame_upload_batch_rectified(ctx.h, P(ids), None, 1, m, 0, None) == capi.E_INVALID
    assert lib.hso_gpu_frame_upload_batch_rectified(ctx.h, P(ids), P(ptrs), 0, m, 0, None) == capi.E_INVALID
    assert lib.hso_gpu_frame_upload_batch_rectified(ctx.h, P(ids), P(ptrs), 1, m + 1, 0, None) == capi.E_INVALID
    ctx.frame_upload(6, np.zeros((64, 64), np.uint8))
    ids6 = np.array([6], np.int64)
    assert lib.hso_gpu_frame_upload_batch_rectified(ctx.h, P(ids6), P(ptrs), 1, m, 0, None) == capi.E_INVALID
    # a destroyed map is unknown from then on; the frames made through it stay
    ctx.rectify_map_destroy(m)
    assert lib.hso_gpu_rectify_map_destroy(ctx.h, m) == capi.E_INVALID
    assert lib.hso_gpu_frame_upload_rectified(ctx.h, 2, P(img), w, h, m, 0, C.byref(st)) == capi.E_INVALID
    assert lib.hso_gpu_frame_upload_batch_rectified(ctx.h, P(ids), P(ptrs), 1, m, 0, None) == capi.E_INVALID
    assert ctx.frame_level(1, 0, w, h).shape == (h, w)
    assert b"map" in lib.hso_gpu_last_error(ctx.h)


# ------------------------------------------------------------------------------------------------ engine
K_MILD = (-0.01, 0.003, -0.001, 0.0002)
EQUI_SPEC = dict(model=capi.CAM_PINHOLE, width=752, height=480, fx=458.654, fy=457.296, cx=367.215, cy=248.375)   # the rectified geometry


def _raw_frame(args):
    """the image an Equidistant camera with K_MILD sees: the pinhole rendering of the scene, sampled where each raw pixel's ray goes"""
    seed, q, t, k = args
    sc = synth.Scene(EQUI_SPEC, seed)
    ys, xs = np.mgrid[0:sc.h, 0:sc.w].astype(np.float64)
    mx, my = (xs - sc.cx) / sc.fx, (ys - sc.cy) / sc.fy
    rd = np.sqrt(mx * mx + my * my)                      # = theta_d
    th = rd.copy()
    for _ in range(6):                                   # Newton on theta (1 + k0 th^2 + k1 th^4 + k2 th^6 + k3 th^8) = theta_d
        t2 = th * th
        f = th * (1 + t2 * (K_MILD[0] + t2 * (K_MILD[1] + t2 * (K_MILD[2] + t2 * K_MILD[3])))) - rd
        df = 1 + t2 * (3 * K_MILD[0] + t2 * (5 * K_MILD[1] + t2 * (7 * K_MILD[2] + t2 * 9 * K_MILD[3])))
        th = th - f / df
    s = np.where(rd > 1e-9, np.tan(th) / np.maximum(rd, 1e-9), 1.0)
    xu, yu = sc.cx + sc.fx * mx * s, sc.cy + sc.fy * my * s
    x0, y0 = sc.pixels0_of(np.asarray(q), np.asarray(t), xu, yu, iters=5)
    img = sc.texture(x0, y0) + np.random.default_rng(seed + 100 + k).normal(0, 0.5, x0.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def raw_sequences():
    """two short raw sequences (different scenes and motions), their host-rectified twins, and the first frames' depth images"""
    import multiprocessing as mp
    cam = capi.make_camera(capi.CAM_EQUIDISTANT, 752, 480, EQUI_SPEC["fx"], EQUI_SPEC["fy"], EQUI_SPEC["cx"], EQUI_SPEC["cy"], d=list(K_MILD), distortion=0)
    xy, frac = capi.rectify_build_map(cam)
    jobs, metas = [], []
    for seed, n, step, rot in ((2024, 5, (0.016, 0.005, 0.007), (0.05, -0.12, 0.03)), (2041, 4, (0.02, 0.004, 0.006), (0.04, -0.1, 0.03))):
        for k in range(n):
            jobs.append((seed, list(synth.rotvec_to_quat(np.deg2rad(np.array(rot)) * k)), list(np.array(step) * k), k))
        metas.append((seed, n))
    with mp.get_context("fork").Pool(min(9, len(jobs))) as pool:
        images = pool.map(_raw_frame, jobs, chunksize=1)
    out, at = [], 0
    for seed, n in metas:
        raw = images[at:at + n]
        at += n
        sc = synth.Scene(EQUI_SPEC, seed)
        ys, xs = np.mgrid[0:sc.h, 0:sc.w].astype(np.float64)
        out.append(dict(raw=raw, rect=[capi.rectify_host(xy, frac, im) for im in raw], depth0=sc.points0(xs, ys)[..., 2].astype(np.float32)))
    return cam, out


def _solo(cam, images, depth0, rectify):
    odo = vo.VisualOdometry(cam, 120)
    if rectify:
        odo.set_options(rectify=True)
    odo.set_first_frame(images[0], depth0, 0.0)
    sts = [bytes(odo.status())] + [bytes(odo.add_image(im, float(k))) for k, im in enumerate(images[1:], 1)]
    kfs = [(a, bytes(b), c) for a, b, c in odo.keyframes()]
    odo.close()
    return sts, kfs


def test_engine_rectify_equals_host_rectified_images(raw_sequences):
    cam, seqs = raw_sequences
    S = seqs[0]
    assert not np.array_equal(S["raw"][0], S["rect"][0])
    on = _solo(cam, S["raw"], S["depth0"], True)
    off = _solo(cam, S["rect"], S["depth0"], False)
    last = vo.VoStatus.from_buffer_copy(on[0][-1])
    assert last.n_tracked > 0 and last.stage == 3, (last.n_tracked, last.stage)
    assert on == off          # every status record (poses included) and every keyframe pose, to the bit
    raw_unrectified = _solo(cam, S["raw"], S["depth0"], False)
    assert raw_unrectified != on


def test_engine_rectify_bank_of_three(raw_sequences):
    cam, seqs = raw_sequences
    runs = [(seqs[0], 5), (seqs[1], 4), (seqs[0], 3)]        # different lengths: sequences sit steps out
    got = {}
    for rectify in (True, False):
        key = "raw" if rectify else "rect"
        bank = vo.MultiVisualOdometry(cam, 3, 120)
        if rectify:
            bank.set_options(rectify=True)
        bank.set_first_frames([s[key][0] for s, _ in runs], [s["depth0"] for s, _ in runs])
        rec = [[bytes(bank.status(i))] for i in range(3)]
        for k in range(1, 5):
            bank.add_images([s[key][k] if k < n else None for s, n in runs], [float(k)] * 3)
            for i, (s, n) in enumerate(runs):
                if k < n:
                    rec[i].append(bytes(bank.status(i)))
        got[key] = (rec, [[(a, bytes(b), c) for a, b, c in bank.keyframes(i)] for i in range(3)])
        bank.close()
    for i in range(3):
        assert vo.VoStatus.from_buffer_copy(got["raw"][0][i][-1]).n_tracked > 0
    assert got["raw"] == got["rect"]
    # ... and a sequence in the bank is the sequence alone
    assert got["raw"][0][0] == _solo(cam, seqs[0]["raw"], seqs[0]["depth0"], True)[0]


def test_engine_refuses_rectify_for_cameras_the_reference_does_not_rectify():
    odo = vo.VisualOdometry(synth.camera(synth.EUROC), 120)
    o = vo.VoOptions(C.sizeof(vo.VoOptions))
    o.rectify = 1
    assert odo.lib.hso_vo_set_options(odo.h, C.byref(o)) == capi.E_INVALID
    o.rectify = 0
    assert odo.lib.hso_vo_set_options(odo.h, C.byref(o)) == 0          # the handle stays usable
    odo.close()


def test_run_sequence_rectifies_with_the_wide_tum_camera_file(tmp_path):
    """a stand-in folder of sensor-size images and tests/golden/cameras/tum_mono_vo_wide.txt (third line `true`): the first traced
    frame_upload record holds the resized AND rectified image (before this option existed: the merely resized one)"""
    from hso_amd import run_sequence
    cam_file = os.path.join(ROOT, "tests", "golden", "cameras", "tum_mono_vo_wide.txt")
    calib = formats.parse_calibration(cam_file)
    W, H = calib["width"], calib["height"]
    folder = tmp_path / "images"
    folder.mkdir()
    sc = synth.Scene(dict(model=capi.CAM_PINHOLE, width=1280, height=1024, fx=450.0, fy=450.0, cx=640.0, cy=512.0, texture_om=((0.004, 0.05), (0.05, 0.4))), 77)
    sensor = sc.render(np.array([0, 0, 0, 1.0]), np.zeros(3))
    formats.write_png(str(folder / "00000.png"), sensor)
    np.save(str(tmp_path / "d0.npy"), np.full((H, W), 3.0, np.float32))
    trace = str(tmp_path / "trace.bin")
    line = run_sequence.main([str(folder), "None", cam_file, "end=1", "depth0=" + str(tmp_path / "d0.npy"), "trace=" + trace,
                              "result=" + str(tmp_path / "traj.txt")], return_line=True)
    assert isinstance(line, dict) and line["frames"] == 1
    rec = next(r for name, r in vo.read_trace(trace) if name == "frame_upload")
    assert (vo.scalar(rec, "width"), vo.scalar(rec, "height")) == (W, H)
    got = np.frombuffer(rec["img"], np.uint8).reshape(H, W)
    ctx = capi.Context(0)
    ctx.frame_upload_resized(1, sensor, W, H)
    resized = ctx.frame_level(1, 0, W, H)
    ctx.close()
    want = capi.rectify_host(*capi.rectify_build_map(calib["camera"]), resized)
    assert not np.array_equal(want, resized)
    assert np.array_equal(got, want)
