"""The batched cv::resize at upload (k_resize_batch, hso_gpu_frame_upload_batch_resized) byte for byte against the CPU restatement
orc.resize_linear (oracle/hso_oracle_image.c) and against the single-frame hso_gpu_frame_upload_resized on the same image: every
branch of the definition by shape, batches against n single calls, host and device sources, the rectification behind it, the
src == dst case and the error codes."""
import ctypes as C

import numpy as np
import pytest

import rectify_ref as ref
from hso_amd import capi

pytestmark = pytest.mark.gpu

# (source w, h) -> (destination w, h)
SHAPES = {
    "area_fast": ((128, 128), (64, 64)),            # both scales exactly 2: (a + b + c + d + 2) >> 2
    "integer_3": ((192, 192), (64, 64)),            # integer scale other than 2: bilinear
    "mixed_2x3": ((128, 192), (64, 64)),            # scales 2 and 3: bilinear
    "odd_source": ((89, 91), (64, 64)),             # odd source width, fractional scale
    "upscale": ((64, 64), (96, 80)),                # left clamp, right tail, top and bottom row clamps
    "resize_pyramid": ((90, 66), (68, 76)),         # destination takes the cv::resize pyramid branch
}


def _stats(st):
    return (st.integral_image, st.grad_mean, st.width, st.height)


def _images(sw, sh, seed=5):
    rng = np.random.default_rng(seed)
    cols = np.tile(np.where(np.arange(sw) % 2 == 0, 0, 255).astype(np.uint8), (sh, 1))
    rows = np.tile(np.where(np.arange(sh) % 2 == 0, 0, 255).astype(np.uint8)[:, None], (1, sw))
    return [rng.integers(0, 256, (sh, sw), dtype=np.uint8), cols, np.ascontiguousarray(rows)]


@pytest.fixture()
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _all_levels(ctx, fid, w, h):
    return [ctx.frame_level(fid, l, w, h) for l in range(5)]


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_equals_oracle_and_single_frame_entry(ctx, orc, name):
    (sw, sh), (dw, dh) = SHAPES[name]
    imgs = _images(sw, sh)
    assert imgs[1].shape == imgs[2].shape == (sh, sw) and imgs[1][0, 1] == 255 and imgs[2][1, 0] == 255 and imgs[2][0, 1] == 0
    ids = [10, 11, 12]
    st = ctx.frame_upload_batch_resized(ids, dw, dh, imgs=imgs)
    for i, im in enumerate(imgs):
        want = orc.resize_linear(im, dw, dh)
        got = ctx.frame_level(ids[i], 0, dw, dh)
        assert np.array_equal(got, want), "%s image %d: %d bytes differ, first at %s" % (name, i, int((got != want).sum()), np.argwhere(got != want)[:3].tolist())
        st1 = ctx.frame_upload_resized(100 + i, im, dw, dh)
        single = _all_levels(ctx, 100 + i, dw, dh)
        assert np.array_equal(single[0], want)
        for l in range(1, 5):        # levels 1-4 (for 68x76: the cv::resize pyramid branch) and the statistics behind the new level 0
            assert np.array_equal(ctx.frame_level(ids[i], l, dw, dh), single[l]), (name, i, l)
        assert _stats(st[i]) == _stats(st1)


def test_tum_mono_sensor_size(ctx, orc):
    img = np.random.default_rng(21).integers(0, 256, (1024, 1280), dtype=np.uint8)
    st = ctx.frame_upload_batch_resized([1], 920, 736, imgs=[img])
    assert np.array_equal(ctx.frame_level(1, 0, 920, 736), orc.resize_linear(img, 920, 736))
    st1 = ctx.frame_upload_resized(2, img, 920, 736)
    assert _stats(st[0]) == _stats(st1)
    assert np.array_equal(ctx.frame_level(1, 4, 920, 736), ctx.frame_level(2, 4, 920, 736))


@pytest.mark.parametrize("name", ["odd_source", "area_fast"])
def test_batch_equals_single_calls(ctx, name):
    import torch
    (sw, sh), (dw, dh) = SHAPES[name]
    rng = np.random.default_rng(8)
    imgs = [rng.integers(0, 256, (sh, sw), dtype=np.uint8) for _ in range(5)]
    single, single_st = [], []
    for i, im in enumerate(imgs):
        single_st.append(_stats(ctx.frame_upload_resized(1000 + i, im, dw, dh)))
        single.append(_all_levels(ctx, 1000 + i, dw, dh))

    def same(fid, i):
        for l in range(5):
            assert np.array_equal(ctx.frame_level(fid, l, dw, dh), single[i][l]), (fid, i, l)

    next_id = 1
    for n in (1, 5):
        for on_device in (False, True):
            ids = list(range(next_id, next_id + n))
            next_id += n
            if on_device:
                d = [torch.from_numpy(im).cuda() for im in imgs[:n]]
                torch.cuda.synchronize()
                st = ctx.frame_upload_batch_resized(ids, dw, dh, device_ptrs=[t.data_ptr() for t in d], src_width=sw, src_height=sh)
            else:
                st = ctx.frame_upload_batch_resized(ids, dw, dh, imgs=imgs[:n])
            for i, fid in enumerate(ids):
                same(fid, i)
                assert _stats(st[i]) == single_st[i]
    # a device source at an odd address: nothing assumes an aligned source
    flat = torch.zeros(sw * sh + 8, dtype=torch.uint8, device="cuda")
    flat[3:3 + sw * sh] = torch.from_numpy(imgs[2].reshape(-1)).cuda()
    torch.cuda.synchronize()
    st = ctx.frame_upload_batch_resized([300], dw, dh, device_ptrs=[flat.data_ptr() + 3], src_width=sw, src_height=sh)
    same(300, 2)
    # device images without statistics: the asynchronous form
    d = [torch.from_numpy(im).cuda() for im in imgs]
    torch.cuda.synchronize()
    ids = list(range(500, 505))
    assert ctx.frame_upload_batch_resized(ids, dw, dh, device_ptrs=[t.data_ptr() for t in d], src_width=sw, src_height=sh, want_stats=False) is None
    ctx.synchronize()
    for i, fid in enumerate(ids):
        same(fid, i)
        assert _stats(ctx.debug_frame_stats(fid)) == single_st[i]
    # two resident ids refreshed in place, mixed with three new ones
    st = ctx.frame_upload_batch_resized([500, 777, 501, 778, 779], dw, dh, imgs=[imgs[4], imgs[3], imgs[2], imgs[1], imgs[0]])
    for k, (fid, i) in enumerate(((500, 4), (777, 3), (501, 2), (778, 1), (779, 0))):
        same(fid, i)
        assert _stats(st[k]) == single_st[i]
    same(502, 2)                     # a neighbour that was not named stays


def test_with_rectify_map(ctx, orc):
    """resize, then remap, as the harness orders them: a FOV-undistort map of tests/golden/cameras/tum_mono_vo_wide.txt at 92x76"""
    import torch
    cam = ref.tum_wide(92, 76)
    xy, frac = capi.rectify_build_map(cam)
    m = ctx.rectify_map_create(cam=cam)
    rng = np.random.default_rng(13)
    imgs = [rng.integers(0, 256, (107, 131), dtype=np.uint8) for _ in range(5)]
    want = [capi.rectify_host(xy, frac, orc.resize_linear(im, 92, 76)) for im in imgs]
    assert not np.array_equal(want[0], orc.resize_linear(imgs[0], 92, 76))
    st = ctx.frame_upload_batch_resized([1, 2, 3, 4, 5], 92, 76, imgs=imgs, map_id=m)
    d = [torch.from_numpy(im).cuda() for im in imgs]
    torch.cuda.synchronize()
    st_d = ctx.frame_upload_batch_resized([11, 12, 13, 14, 15], 92, 76, device_ptrs=[t.data_ptr() for t in d], src_width=131, src_height=107, map_id=m)
    for i in range(5):
        assert np.array_equal(ctx.frame_level(1 + i, 0, 92, 76), want[i]), i
        assert np.array_equal(ctx.frame_level(11 + i, 0, 92, 76), want[i]), i
        st1 = ctx.frame_upload(100 + i, want[i])
        assert _stats(st[i]) == _stats(st1) == _stats(st_d[i])
        assert np.array_equal(ctx.frame_level(1 + i, 3, 92, 76), ctx.frame_level(100 + i, 3, 92, 76))
    # the single-frame rectified entry resizes in front too: the same bytes
    ctx.frame_upload_rectified(200, imgs[0], m)
    assert np.array_equal(ctx.frame_level(200, 0, 92, 76), want[0])


def test_same_size_is_the_plain_batch(ctx):
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, (66, 68), dtype=np.uint8) for _ in range(3)]
    st = ctx.frame_upload_batch_resized([1, 2, 3], 68, 66, imgs=imgs)
    st_p = ctx.frame_upload_batch([11, 12, 13], imgs=imgs)
    for i in range(3):
        assert _stats(st[i]) == _stats(st_p[i])
        for l in range(5):
            assert np.array_equal(ctx.frame_level(1 + i, l, 68, 66), ctx.frame_level(11 + i, l, 68, 66))
    assert np.array_equal(ctx.frame_level(2, 0, 68, 66), imgs[1])
    # ... and with a map, the plain rectified batch
    cam = ref.border_camera()
    m = ctx.rectify_map_create(cam=cam)
    ctx.frame_upload_batch_resized([21, 22, 23], 68, 66, imgs=imgs, map_id=m)
    ctx.frame_upload_batch_rectified([31, 32, 33], m, imgs=imgs)
    for i in range(3):
        assert np.array_equal(ctx.frame_level(21 + i, 0, 68, 66), ctx.frame_level(31 + i, 0, 68, 66))
        assert np.array_equal(ctx.frame_level(21 + i, 0, 68, 66), capi.rectify_host(*capi.rectify_build_map(cam), imgs[i]))


def test_error_codes(ctx, orc):
    lib, P = ctx.lib, capi._ptr
    sw, sh, dw, dh = 89, 91, 64, 64
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 256, (sh, sw), dtype=np.uint8) for _ in range(3)]
    ids = np.array([1, 2, 3], np.int64)
    ptrs = np.array([im.ctypes.data for im in imgs], np.uint64)
    out = np.zeros((dh, dw), np.uint8)

    def call(ids_=ids, ptrs_=ptrs, n=3, sw_=sw, sh_=sh, dw_=dw, dh_=dh, m=-1, h=ctx.h):
        return lib.hso_gpu_frame_upload_batch_resized(h, P(ids_) if ids_ is not None else None, P(ptrs_) if ptrs_ is not None else None, n,
                                                      sw_, sh_, dw_, dh_, m, 0, None)

    def none_resident():
        for fid in (1, 2, 3):
            assert lib.hso_gpu_frame_download_level(ctx.h, fid, 0, P(out), None, None) == -2     # HSO_E_NOFRAME

    assert call(h=None) == capi.E_INVALID
    assert call(ids_=None) == capi.E_INVALID
    assert call(ptrs_=None) == capi.E_INVALID
    assert call(n=0) == capi.E_INVALID and call(n=-1) == capi.E_INVALID
    assert call(sw_=0) == capi.E_INVALID and call(sh_=-3) == capi.E_INVALID
    assert call(dw_=66) == capi.E_INVALID                                   # width % 4
    assert call(dw_=60) == capi.E_INVALID and call(dh_=63) == capi.E_INVALID     # smaller than 64x64
    assert call(m=0) == capi.E_INVALID and call(m=12345) == capi.E_INVALID       # no such map
    cam = ref.border_camera()
    m = ctx.rectify_map_create(cam=cam)                                     # 68x66
    assert call(m=m) == capi.E_INVALID                                      # a map of another size than the destination
    assert call(sw_=68, sh_=66, m=m) == capi.E_INVALID                      # ... also when the source has the map's size
    none_resident()
    assert call(ids_=np.array([1, 2, 1], np.int64)) == capi.E_INVALID       # a new id twice
    assert call(ptrs_=np.array([imgs[0].ctypes.data, 0, imgs[2].ctypes.data], np.uint64)) == capi.E_INVALID     # a null image in the middle
    none_resident()
    ctx.frame_upload(2, np.zeros((80, 96), np.uint8))
    assert call() == capi.E_INVALID                                         # a resident frame of another size
    assert b"another size" in lib.hso_gpu_last_error(ctx.h)
    for fid in (1, 3):
        assert lib.hso_gpu_frame_download_level(ctx.h, fid, 0, P(out), None, None) == -2
    assert ctx.frame_level(2, 0, 96, 80).shape == (80, 96)
    ctx.frame_release(2)
    # a valid call succeeds afterwards
    assert call() == 0
    ctx.synchronize()
    for i in range(3):
        assert np.array_equal(ctx.frame_level(1 + i, 0, dw, dh), orc.resize_linear(imgs[i], dw, dh))
