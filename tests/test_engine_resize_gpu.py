"""hso_vo_options.resize: the engine fed sensor-size images (enlarged renderings) against the same engine fed what the single-frame
hso_gpu_frame_upload_resized makes of them, bit for bit in every status record and keyframe — alone, with rectify, in a bank with
a sequence sitting a step out, with device pointers; the refusal without the option; the trace record; run_sequence."""
import ctypes as C

import numpy as np
import pytest

from hso_amd import capi, formats, synth, vo

pytestmark = pytest.mark.gpu

SMALL = dict(synth.EUROC, width=384, height=256, fx=240.0, fy=240.0, cx=191.5, cy=127.5)
MOTION = dict(step=(0.02, 0.006, 0.008), rot_deg_per_frame=(0.04, -0.12, 0.03))
W, H = SMALL["width"], SMALL["height"]
N = 12
REFUSAL = "Frame: provided image has not the same size as the camera model or image is not grayscale"


def enlarge(img, tenths):
    """a sensor image for a camera-size rendering: bilinear enlargement by tenths / 10 (any enlargement serves: both sides of every
    comparison start from these bytes)"""
    h, w = img.shape
    bw, bh = (w * tenths) // 10, (h * tenths) // 10
    xs = np.clip((np.arange(bw) + 0.5) * w / bw - 0.5, 0, w - 1)
    ys = np.clip((np.arange(bh) + 0.5) * h / bh - 0.5, 0, h - 1)
    x0, y0 = np.floor(xs).astype(int), np.floor(ys).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = (xs - x0)[None, :], (ys - y0)[:, None]
    f = img.astype(np.float64)
    out = (f[y0][:, x0] * (1 - fx) + f[y0][:, x1] * fx) * (1 - fy) + (f[y1][:, x0] * (1 - fx) + f[y1][:, x1] * fx) * fy
    return np.ascontiguousarray(np.clip(np.rint(out), 0, 255).astype(np.uint8))     # row-major: the device-pointer test hands the bytes over as they lie


def make_data():
    """three short sequences; per sequence the enlarged images (1.4 x, 2 x, 1.4 x) and what the single-frame entry shrinks them to"""
    seqs = [synth.sequence(N, spec=SMALL, seed=2024 + 17 * k, workers=4, **MOTION) for k in range(3)]
    ctx = capi.Context(0)
    out = []
    for k, S in enumerate(seqs):
        big = [enlarge(im, (14, 20, 14)[k]) for im in S["images"]]
        shrunk = []
        for im in big:
            ctx.frame_upload_resized(1, im, W, H)
            shrunk.append(ctx.frame_level(1, 0, W, H))
            ctx.frame_release(1)
        out.append(dict(big=big, shrunk=shrunk, depth0=S["depth0"]))
    ctx.close()
    assert out[0]["big"][0].shape == (358, 537) and out[1]["big"][0].shape == (512, 768)
    return out


@pytest.fixture(scope="module")
def data():
    return make_data()


def _solo(cam, images, depth0, **options):
    odo = vo.VisualOdometry(cam, 120)
    if options:
        odo.set_options(**options)
    odo.set_first_frame(images[0], depth0, 0.0)
    sts = [bytes(odo.status())] + [bytes(odo.add_image(im, float(k))) for k, im in enumerate(images[1:], 1)]
    kfs = [(a, bytes(b), c) for a, b, c in odo.keyframes()]
    odo.close()
    return sts, kfs


@pytest.mark.parametrize("which", [0, 1])            # 1.4 x: the bilinear path; 2 x: the 2 x 2 decimation
def test_engine_resize_equals_preshrunk_images(data, which):
    cam = synth.camera(SMALL)
    S = data[which]
    on = _solo(cam, S["big"], S["depth0"], resize=True)
    off = _solo(cam, S["shrunk"], S["depth0"])
    last = vo.VoStatus.from_buffer_copy(on[0][-1])
    assert last.n_tracked > 0 and last.stage == 3, (last.n_tracked, last.stage)
    assert on == off          # every field of every status record and the keyframe list, to the bit
    # camera-size images take today's path with the option set
    assert _solo(cam, S["shrunk"], S["depth0"], resize=True) == off


def test_engine_resize_with_rectify(data):
    cam = capi.make_camera(capi.CAM_EQUIDISTANT, W, H, SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], d=[-0.01, 0.003, -0.001, 0.0002], distortion=0)
    S = data[0]
    on = _solo(cam, S["big"], S["depth0"], resize=True, rectify=True)
    off = _solo(cam, S["shrunk"], S["depth0"], rectify=True)
    assert on == off
    assert on != _solo(cam, S["big"], S["depth0"], resize=True)        # the map was applied


def _bank(cam, runs, key, device=False, **options):
    """runs: (sequence, first step, number of frames); a sequence whose frames are used up, or sequence 2 at step 3, sits out"""
    import torch
    bank = vo.MultiVisualOdometry(cam, len(runs), 120)
    if options:
        bank.set_options(**options)
    bank.set_first_frames([s[key][0] for s, _ in runs], [s["depth0"] for s, _ in runs])
    rec = [[bytes(bank.status(i))] for i in range(len(runs))]
    at = [1] * len(runs)
    for step in range(1, N + 1):
        imgs = []
        for i, (s, n) in enumerate(runs):
            sits_out = at[i] >= n or (i == 2 and step == 3)
            imgs.append(None if sits_out else s[key][at[i]])
        if all(im is None for im in imgs):
            break
        stamps = [float(a) for a in at]
        if device:
            d = [torch.from_numpy(im).cuda() if im is not None else None for im in imgs]
            torch.cuda.synchronize()
            shape = next(im.shape for im in imgs if im is not None)
            bank.add_images_device([t.data_ptr() if t is not None else 0 for t in d], shape[1], shape[0], stamps)
        else:
            bank.add_images(imgs, stamps)
        for i, im in enumerate(imgs):
            if im is not None:
                rec[i].append(bytes(bank.status(i)))
                at[i] += 1
    kfs = [[(a, bytes(b), c) for a, b, c in bank.keyframes(i)] for i in range(len(runs))]
    bank.close()
    return rec, kfs


def test_bank_of_three_equals_solo_runs(data):
    cam = synth.camera(SMALL)
    runs = [(data[0], N), (data[2], N - 2), (data[0], N - 1)]          # one image size per call: the 1.4 x sequences
    rec, kfs = _bank(cam, runs, "big", resize=True)
    for i, (s, n) in enumerate(runs):
        sts, k = _solo(cam, s["big"][:n], s["depth0"], resize=True)
        assert rec[i] == sts, i
        assert kfs[i] == k, i
    assert (rec, kfs) == _bank(cam, runs, "shrunk")


def test_device_pointer_images(data):
    cam = synth.camera(SMALL)
    runs = [(data[0], N), (data[2], N - 2), (data[0], N - 1)]
    assert _bank(cam, runs, "big", device=True, resize=True) == _bank(cam, runs, "shrunk")


def test_wrong_size_without_the_option_is_refused_as_before(data):
    cam = synth.camera(SMALL)
    S = data[0]
    odo = vo.VisualOdometry(cam, 120)
    big = S["big"][0]
    rc = odo.lib.hso_vo_set_first_frame(odo.h, capi._ptr(big), big.shape[1], big.shape[0], 0.0, capi._ptr(np.ascontiguousarray(S["depth0"], np.float32)), None)
    assert rc == capi.E_INVALID and odo.lib.hso_vo_last_error(odo.h).decode() == REFUSAL
    odo.set_first_frame(S["shrunk"][0], S["depth0"], 0.0)
    with pytest.raises(capi.HsoGpuError) as e:
        odo.add_image(S["big"][1], 1.0)
    assert str(e.value) == "add_image failed (-1): " + REFUSAL
    assert odo.add_image(S["shrunk"][1], 1.0).stage == 3               # the handle stays usable
    odo.close()
    bank = vo.MultiVisualOdometry(cam, 2, 120)
    with pytest.raises(capi.HsoGpuError) as e:
        bank.set_first_frames([big, big], [S["depth0"], S["depth0"]])
    assert REFUSAL in str(e.value)
    bank.close()


def test_default_is_off_and_set_options_accepts_the_word():
    o = vo.VoOptions(C.sizeof(vo.VoOptions))
    assert o.resize == 0
    odo = vo.VisualOdometry(synth.camera(SMALL), 120)
    o.resize = 1
    assert odo.lib.hso_vo_set_options(odo.h, C.byref(o)) == 0
    o.size = 24                                                        # a caller compiled before the word existed: off
    assert odo.lib.hso_vo_set_options(odo.h, C.byref(o)) == 0
    big = np.zeros((300, 400), np.uint8)
    assert odo.lib.hso_vo_add_image(odo.h, capi._ptr(big), 400, 300, 0.0) == capi.E_INVALID
    assert odo.lib.hso_vo_last_error(odo.h).decode() == REFUSAL
    odo.close()


def test_traced_frame_upload_replays(data, tmp_path):
    cam = synth.camera(SMALL)
    S = data[0]
    trace = str(tmp_path / "trace.bin")
    odo = vo.VisualOdometry(cam, 120)
    odo.set_options(resize=True)
    odo.trace(trace)
    odo.set_first_frame(S["big"][0], S["depth0"], 0.0)
    odo.add_image(S["big"][1], 1.0)
    odo.close()
    recs = [r for name, r in vo.read_trace(trace) if name == "frame_upload"]
    assert len(recs) == 2
    ctx = capi.Context(0)
    for k, rec in enumerate(recs):
        assert (vo.scalar(rec, "width"), vo.scalar(rec, "height")) == (W, H)
        img = np.frombuffer(rec["img"], np.uint8).reshape(H, W)
        assert np.array_equal(img, S["shrunk"][k])
        st = ctx.frame_upload(10 + k, img)                               # the replay
        assert bytes(st) == bytes(rec["stats"])
        st_b = ctx.frame_upload_batch_resized([20 + k], W, H, imgs=[S["big"][k]])[0]
        assert bytes(st_b) == bytes(st)
        for l in range(5):
            assert np.array_equal(ctx.frame_level(10 + k, l, W, H), ctx.frame_level(20 + k, l, W, H))
    ctx.close()


def test_run_sequence_takes_sensor_images(data, tmp_path):
    from hso_amd import run_sequence
    S = data[0]
    cam_file = tmp_path / "cam.txt"
    cam_file.write_text("Pinhole %r %r %r %r 0 0 0 0\n%d %d\n" % (SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], W, H))
    np.save(str(tmp_path / "d0.npy"), S["depth0"])
    got = {}
    for key in ("big", "shrunk"):
        folder = tmp_path / key
        folder.mkdir()
        for k, im in enumerate(S[key]):
            formats.write_png(str(folder / ("%05d.png" % k)), im)
        result = str(tmp_path / (key + ".txt"))
        line = run_sequence.main([str(folder), "None", str(cam_file), "depth0=" + str(tmp_path / "d0.npy"), "result=" + result], return_line=True)
        line = {k: v for k, v in line.items() if k not in ("frames_per_s", "result")}
        got[key] = (line, open(result).read())
    assert got["big"][0]["frames"] == N and got["big"][0]["keyframes"] >= 1 and got["big"][0]["tracking_failures"] == 0
    assert got["big"] == got["shrunk"]
