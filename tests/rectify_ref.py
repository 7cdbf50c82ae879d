"""numpy restatement of image rectification, written from the reference (src/camera.cpp:223-265 FOVCamera::getRemap +
distortPixelFOV, :317-364 EquidistantCamera::getRemap + distortPixelEquidistant) and from OpenCV's cv::convertMaps /
cv::remap fixed-point path — not from hso_amd/csrc/hso_rectify_host.cpp, which the tests hold to it.

Types follow the reference: everything it declares `float` is float32 here, its members (fx_, cx_, omega_, d_[]) are
doubles.  camera.h:32 has `using namespace std;`, so tan / atan / sqrt on floats are the float overloads; tanf and atanf
are taken from the machine's libm through ctypes (numpy's float32 arctan may differ from libm's by an ulp, which would
move map entries); sqrt is correctly rounded either way."""
import ctypes as C
import ctypes.util

import numpy as np

from hso_amd import capi

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tanf.argtypes = _libm.atanf.argtypes = [C.c_float]
_libm.tanf.restype = _libm.atanf.restype = C.c_float
f32, f64 = np.float32, np.float64


def _atanf(a):
    """libm's atanf over a float32 array (equal inputs share one call)"""
    a = np.asarray(a, f32)
    uniq, inv = np.unique(a, return_inverse=True)
    out = np.array([_libm.atanf(float(v)) for v in uniq], f32)
    return out[inv].reshape(a.shape)


def _normalised(cam):
    u = np.arange(cam.width, dtype=f32)[None, :].astype(f64)          # float x = pixel_location[0]; then x - cx_ in double
    v = np.arange(cam.height, dtype=f32)[:, None].astype(f64)
    ix = np.broadcast_to(((u - cam.cx) / cam.fx).astype(f32), (cam.height, cam.width))
    iy = np.broadcast_to(((v - cam.cy) / cam.fy).astype(f32), (cam.height, cam.width))
    r = np.sqrt(ix * ix + iy * iy, dtype=f32)
    return ix, iy, r


def float_maps(cam):
    """map_x_float, map_y_float of getRemap"""
    ix, iy, r = _normalised(cam)
    if cam.model == capi.CAM_FOV and cam.distortion == 0:
        dist = f32(cam.d[0])
        d2t = f32(2) * f32(_libm.tanf(float(dist / f32(2))))
        one = (r == 0) | (dist == 0)
        rs = np.where(one, f32(1), r)
        with np.errstate(divide="ignore", invalid="ignore"):
            fac = np.where(one, f32(1), _atanf(rs * d2t) / (dist * rs)).astype(f32)
        mx = (cam.fx * fac.astype(f64) * ix.astype(f64) + cam.cx).astype(f32)
        my = (cam.fy * fac.astype(f64) * iy.astype(f64) + cam.cy).astype(f32)
        return mx, my
    if cam.model == capi.CAM_EQUIDISTANT:
        k = [float(x) for x in cam.d[:4]]
        theta = _atanf(r)
        t2 = theta * theta
        t4 = t2 * t2
        t6 = t4 * t2
        t8 = t4 * t4
        poly = 1 + k[0] * t2.astype(f64)
        poly = poly + k[1] * t4.astype(f64)
        poly = poly + k[2] * t6.astype(f64)
        poly = poly + k[3] * t8.astype(f64)
        thetad = (theta.astype(f64) * poly).astype(f32)
        big = r.astype(f64) > 1e-8
        scaling = np.where(big, thetad / np.where(big, r, f32(1)), f32(1)).astype(f32)
        mx = (cam.fx * ix.astype(f64) * scaling.astype(f64) + cam.cx).astype(f32)
        my = (cam.fy * iy.astype(f64) * scaling.astype(f64) + cam.cy).astype(f32)
        return mx, my
    raise ValueError("the reference does not rectify this camera")


def convert_maps(mx, my):
    """cv::convertMaps(CV_32FC1, CV_32FC1 -> CV_16SC2, CV_16UC1): cvRound rounds half to even"""
    ix = np.rint(mx * f32(32)).astype(np.int64)
    iy = np.rint(my * f32(32)).astype(np.int64)
    xy = np.stack([np.clip(ix >> 5, -32768, 32767), np.clip(iy >> 5, -32768, 32767)], axis=-1).astype(np.int16)
    frac = ((iy & 31) * 32 + (ix & 31)).astype(np.uint16)
    return xy, frac


def build_map(cam):
    return convert_maps(*float_maps(cam))


def classes(xy, w, h):
    """per pixel: 0 inlier, 1 fully outside, 2 partial (cv::remap's three branches)"""
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    inl = (sx >= 0) & (sx < w - 1) & (sy >= 0) & (sy < h - 1)
    out = (sx >= w) | (sx + 1 < 0) | (sy >= h) | (sy + 1 < 0)
    return np.where(inl, 0, np.where(out, 1, 2))


def remap(xy, frac, src):
    """cv::remap(src, ., xy, frac, INTER_LINEAR), CV_8UC1, BORDER_CONSTANT 0: weights (32-ax)(32-ay)*32 ..., taps outside read 0"""
    src = np.asarray(src, np.uint8)
    h, w = src.shape
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    f = frac.astype(np.int64) & 1023
    ax, ay = f & 31, f >> 5
    acc = np.zeros(frac.shape, np.int64)
    for dy, dx, wt in ((0, 0, (32 - ax) * (32 - ay) * 32), (0, 1, ax * (32 - ay) * 32), (1, 0, (32 - ax) * ay * 32), (1, 1, ax * ay * 32)):
        x, y = sx + dx, sy + dy
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        tap = np.where(ok, src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64), 0)
        acc += tap * wt
    assert int(acc.max(initial=0)) + 16384 < 2 ** 31
    out = (acc + 16384) >> 15
    assert int(out.max(initial=0)) <= 255
    return out.astype(np.uint8)


# ---- the cameras and maps the tests share
def tum_wide(width=920, height=736):
    """tests/golden/cameras/tum_mono_vo_wide.txt at 920x736 (as parsed), or its normalised intrinsics at another size"""
    import os
    from hso_amd import formats
    here = os.path.dirname(os.path.abspath(__file__))
    cam = formats.parse_calibration(os.path.join(here, "golden", "cameras", "tum_mono_vo_wide.txt"))["camera"]
    if (width, height) != (cam.width, cam.height):
        cam = capi.make_camera(capi.CAM_FOV, width, height, cam.fx / cam.width * width, cam.fy / cam.height * height,
                               cam.cx / cam.width * width, cam.cy / cam.height * height, d=[cam.d[0]], distortion=0)
    return cam


def equidistant_512():
    return capi.make_camera(capi.CAM_EQUIDISTANT, 512, 512, 190.978, 190.973, 254.932, 256.897, d=[0.00348, 0.000715, -0.00205, 0.000203], distortion=0)


def equidistant_752():
    return capi.make_camera(capi.CAM_EQUIDISTANT, 752, 480, 458.654, 457.296, 367.215, 248.375, d=[-0.03, 0.01, -0.004, 0.0005], distortion=0)


def border_camera():
    """strong coefficients on a small image: inlier, fully-outside and partial pixels by the hundred"""
    return capi.make_camera(capi.CAM_EQUIDISTANT, 68, 66, 30.0, 31.0, 20.25, 40.5, d=[0.6, 0.2, 0.0, 0.0], distortion=0)


def handmade_map(w, h, seed):
    """every branch and every single-tap-outside combination: sx in {-2,-1,0,W-2,W-1,W} x sy likewise x frac in
    {0, 31, 992, 1023, random}, tiled over the image in a shuffled order"""
    rng = np.random.default_rng(seed)
    xs = [-2, -1, 0, w - 2, w - 1, w]
    ys = [-2, -1, 0, h - 2, h - 1, h]
    combos = [(x, y, f) for x in xs for y in ys for f in (0, 31, 992, 1023, -1)]
    idx = np.resize(rng.permutation(len(combos)), w * h)
    rng.shuffle(idx)
    xy = np.zeros((h * w, 2), np.int16)
    frac = np.zeros(h * w, np.uint16)
    rnd = rng.integers(0, 1024, w * h)
    for i, c in enumerate(idx):
        x, y, f = combos[c]
        xy[i] = (x, y)
        frac[i] = rnd[i] if f < 0 else f
    assert w * h >= len(combos)
    return xy.reshape(h, w, 2), frac.reshape(h, w)
