"""Image rectification without a GPU: hso_gpu_rectify_build_map and hso_gpu_rectify_host (hso_amd/csrc/hso_rectify_host.cpp, host
code behind the C-ABI) against the numpy restatement tests/rectify_ref.py, entry for entry and byte for byte — both sides call
the same libm, so the tolerance is zero — and the Equidistant branch of formats.parse_calibration."""
import ctypes as C
import os

import numpy as np
import pytest

import rectify_ref as ref
from conftest import ROOT
from hso_amd import capi, formats

CAMERAS = {
    "tum_wide_920x736": lambda: ref.tum_wide(),
    "tum_wide_64x64": lambda: ref.tum_wide(64, 64),
    "equidistant_512": ref.equidistant_512,
    "border_68x66": ref.border_camera,
}


@pytest.fixture(scope="module")
def lib():
    from hso_amd import build
    build.build()
    return capi.load()


@pytest.fixture(scope="module")
def maps(lib):
    """name -> (camera, restated xy, restated frac), computed once"""
    out = {}
    for name, make in CAMERAS.items():
        cam = make()
        out[name] = (cam,) + ref.build_map(cam)
    return out


@pytest.mark.parametrize("name", list(CAMERAS))
def test_build_map_equals_restatement(lib, maps, name):
    cam, xy_ref, frac_ref = maps[name]
    xy, frac = capi.rectify_build_map(cam)
    assert xy.shape == (cam.height, cam.width, 2) and frac.shape == (cam.height, cam.width)
    assert np.array_equal(xy, xy_ref), "xy differs in %d entries" % int((xy != xy_ref).sum())
    assert np.array_equal(frac, frac_ref), "frac differs in %d entries" % int((frac != frac_ref).sum())
    assert int(frac.max()) <= 1023


def test_real_cameras_have_no_border_pixels_and_the_border_camera_has_every_class(maps):
    for name in ("tum_wide_920x736", "equidistant_512"):
        cam, xy, _ = maps[name]
        assert not ref.classes(xy, cam.width, cam.height).any(), name
    cam, xy, _ = maps["border_68x66"]
    counts = np.bincount(ref.classes(xy, cam.width, cam.height).ravel(), minlength=3)
    print("border camera: inlier / fully outside / partial =", counts.tolist())
    assert (counts >= 100).all(), counts.tolist()


@pytest.mark.parametrize("name", list(CAMERAS))
def test_host_remap_equals_restatement_through_camera_maps(lib, maps, name):
    cam, xy, frac = maps[name]
    rng = np.random.default_rng(11)
    for img in (rng.integers(0, 256, (cam.height, cam.width), dtype=np.uint8), np.full((cam.height, cam.width), 255, np.uint8)):
        got = capi.rectify_host(xy, frac, img)
        assert np.array_equal(got, ref.remap(xy, frac, img))
    if name == "equidistant_512":   # an undistorting map of a mild lens keeps a flat image flat
        assert (got == 255).all()


@pytest.mark.parametrize("w,h", [(64, 64), (68, 66)])
def test_host_remap_handmade_map_places_every_branch(lib, w, h):
    xy, frac = ref.handmade_map(w, h, seed=w)
    cls = np.bincount(ref.classes(xy, w, h).ravel(), minlength=3)
    assert (cls >= 100).all(), cls.tolist()
    # every (sx, sy) pair of the border set is present, so every single-tap-outside combination is
    pairs = {(int(a), int(b)) for a, b in xy.reshape(-1, 2)}
    assert len(pairs) == 36
    rng = np.random.default_rng(5)
    for img in (rng.integers(0, 256, (h, w), dtype=np.uint8), np.full((h, w), 255, np.uint8)):
        got = capi.rectify_host(xy, frac, img)
        want = ref.remap(xy, frac, img)
        assert np.array_equal(got, want), "differs at %s" % np.argwhere(got != want)[:5].tolist()
    # all-255: a pixel whose four taps are inside stays 255 whatever the fraction (the weights sum to 32768), none exceeds it
    inl = ref.classes(xy, w, h) == 0
    assert (got[inl] == 255).all() and (got[ref.classes(xy, w, h) == 1] == 0).all()


def test_build_map_and_host_remap_refusals(lib):
    xy = np.zeros((64, 64, 2), np.int16)
    frac = np.zeros((64, 64), np.uint16)
    pin = capi.make_camera(capi.CAM_PINHOLE, 64, 64, 50, 50, 32, 32, d=[-0.28, 0.07, 0, 0, 0])
    fov_distorting = capi.make_camera(capi.CAM_FOV, 64, 64, 50, 50, 32, 32, d=[0.9], distortion=1)
    fov = capi.make_camera(capi.CAM_FOV, 64, 64, 50, 50, 32, 32, d=[0.9], distortion=0)
    f = lib.hso_gpu_rectify_build_map
    assert f(C.byref(pin), capi._ptr(xy), capi._ptr(frac)) == capi.E_INVALID
    assert f(C.byref(fov_distorting), capi._ptr(xy), capi._ptr(frac)) == capi.E_INVALID
    assert f(None, capi._ptr(xy), capi._ptr(frac)) == capi.E_INVALID
    assert f(C.byref(fov), None, capi._ptr(frac)) == capi.E_INVALID
    assert f(C.byref(fov), capi._ptr(xy), None) == capi.E_INVALID
    assert f(C.byref(fov), capi._ptr(xy), capi._ptr(frac)) == 0
    img = np.zeros((64, 64), np.uint8)
    out = np.zeros_like(img)
    g = lib.hso_gpu_rectify_host
    assert g(None, capi._ptr(frac), 64, 64, capi._ptr(img), capi._ptr(out)) == capi.E_INVALID
    assert g(capi._ptr(xy), capi._ptr(frac), 64, 64, None, capi._ptr(out)) == capi.E_INVALID
    assert g(capi._ptr(xy), capi._ptr(frac), 64, 64, capi._ptr(img), capi._ptr(img)) == capi.E_INVALID   # in place: cv::remap clones
    assert g(capi._ptr(xy), capi._ptr(frac), 64, 64, capi._ptr(img), capi._ptr(out)) == 0


def test_parse_calibration_equidistant():
    c = formats.parse_calibration("Equidistant 190.978 190.973 254.932 256.897 0.00348 0.000715 -0.00205 0.000203\n512 512\n")
    cam = c["camera"]
    assert c["model"] == "Equidistant" and c["undistort"] is True and (c["width"], c["height"]) == (512, 512)
    assert cam.model == capi.CAM_EQUIDISTANT and cam.distortion == 0 and (cam.width, cam.height) == (512, 512)
    assert [cam.fx, cam.fy, cam.cx, cam.cy] == [float(np.float32(v)) for v in (190.978, 190.973, 254.932, 256.897)]
    assert list(cam.d) == [float(np.float32(v)) for v in (0.00348, 0.000715, -0.00205, 0.000203)] + [0.0]
    # above 848x800 the file's size and intrinsics shrink by the pinhole branch's rule (test/test_dataset.cpp:186-196)
    line = "%s 1000 1001 640 512 0.01 0.002 0 0\n1280 1024\n"
    e, p = formats.parse_calibration(line % "Equidistant"), formats.parse_calibration(line % "Pinhole")
    assert (e["width"], e["height"]) == (p["width"], p["height"]) == (920, 736) and (e["file_width"], e["file_height"]) == (1280, 1024)
    for k in ("fx", "fy", "cx", "cy"):
        assert getattr(e["camera"], k) == getattr(p["camera"], k) and getattr(e["camera"], k) < 1000
    assert e["camera"].model == capi.CAM_EQUIDISTANT and e["undistort"] is True and p["undistort"] is False
    assert list(e["camera"].d)[:2] == [float(np.float32(0.01)), float(np.float32(0.002))]


def test_fov_fixtures_parse_as_before():
    wide = formats.parse_calibration(os.path.join(ROOT, "tests", "golden", "cameras", "tum_mono_vo_wide.txt"))
    narrow = formats.parse_calibration(os.path.join(ROOT, "tests", "golden", "cameras", "tum_mono_vo_narrow.txt"))
    assert wide["model"] == narrow["model"] == "FOV"
    assert wide["undistort"] is True and wide["camera"].distortion == 0
    assert narrow["undistort"] is False and narrow["camera"].distortion == 1
    for c in (wide, narrow):
        assert (c["width"], c["height"], c["file_width"], c["file_height"]) == (920, 736, 1280, 1024)
        assert c["camera"].model == capi.CAM_FOV
    assert wide["camera"].d[0] == float(np.float32(0.933271))
    assert abs(wide["camera"].fx - 0.349153 * 920) < 1e-3 and abs(wide["camera"].cy - 0.499021 * 736) < 1e-3
