"""The frame build (k_pyramid / k_resize_level, k_sobel in its three modes and two bodies, k_frame_stats) against exact
references at the small shapes where the Sobel tiling, the narrow pyramid stores and the bilinear step meet their edges
(frame_ref.SMALL_SHAPES says what each shape reaches), with images whose gradient mean is NOT clamped.

References: pyramid levels = the CPU restatement (tied to frame_ref's roundings in test_frame_ref_cpu.py); gradient images =
frame_ref.sobel5_exact; statistics = frame_ref.stats_exact, never the restatement (its serial fp32 sum is itself 6e-5 .. 8e-5
away from the exact gradient mean at full size).

Tolerances.  integral_image: bit-equal (the device sum is an exact integer, then one fp64 division and one rounding: the
reference's operations).  grad_mean, reference clamped: exactly 7.0 / 20.0.  grad_mean, unclamped: 1e-6 relative.  Worst case
per term: int -> fp32 conversion of the exact square sum 2^-24, halved by the root; v_sqrt_f32 1 ulp = 2^-23; two fp32
additions of positive values 2 * 2^-24; all terms positive, so the sum is within 2.7e-7; the final cast and the fp32 division
by 30 add 2 * 2^-24: under 4e-7.  The fp64 accumulation is negligible.  1e-6 leaves 2.5x.

Every unclamped comparison first asserts 7.5 < unclamped < 19.5 on the reference, before the device is asked.

Largest |device - exact| / exact of grad_mean observed (k16 / k24 textures, both contexts, returned record and
debug_frame_stats, single and batched uploads), MI355X:
    64x64   0        192x128  0        80x96   0
    64x72   0        68x76    6.1e-8   100x68  0         (6.1e-8 = one float32 ulp at 15.7; 0 = the same float32)
    full size, texture k = 16 (test_parity_gpu.py): 640x480 0, 752x480 9.0e-8, 920x736 0
"""
import numpy as np
import pytest

from frame_ref import SMALL_SHAPES, TEXTURES, UNCLAMPED, sobel5_exact, stats_exact, texture, texture_seed
from hso_amd import capi

pytestmark = pytest.mark.gpu

SHAPES = list(SMALL_SHAPES)
IDS = ["%dx%d" % s for s in SHAPES]
PLUMBING = [(192, 128), (68, 76)]
PLUMBING_IDS = ["%dx%d" % s for s in PLUMBING]
GRAD_MEAN_REL = 1e-6
CONSTANT = 93


class Ref:
    def __init__(self, orc, img):
        self.img = img
        self.levels = orc.create_pyramid(img)
        self.sobel = [sobel5_exact(self.levels[l]) for l in range(3)]
        self.stats = stats_exact(img)


@pytest.fixture(scope="module")
def refs(orc):
    """every reference once: (size, texture name | "constant") -> Ref; read-only"""
    out = {}
    for (w, h) in SHAPES:
        for name, k in TEXTURES.items():
            out[(w, h), name] = Ref(orc, texture(w, h, k, texture_seed(w, h, name)))
        out[(w, h), "constant"] = Ref(orc, np.full((h, w), CONSTANT, np.uint8))
    return out


@pytest.fixture(scope="module")
def ctxs():
    lazy, eager = capi.Context(0), capi.Context(0)
    eager.configure(eager_gradients=True)
    yield {"lazy": lazy, "eager": eager}
    lazy.close(); eager.close()


def _release(ctx, ids):
    for i in ids:
        try:
            ctx.frame_release(i)
        except capi.HsoGpuError:
            pass


def _input_regime(ex, name):
    """the condition on the INPUT, from the reference alone: which clamp regime the comparison is going to be made in"""
    if name in UNCLAMPED:
        assert 7.5 < ex.unclamped < 19.5, ex.unclamped
    elif name in ("k4", "constant"):
        assert ex.unclamped < 6.5 and ex.grad_mean == np.float32(7)
    else:
        assert ex.unclamped > 20.5 and ex.grad_mean == np.float32(20)


def _check_stats(st, ex, what):
    assert (st.width, st.height) == (ex.width, ex.height), what
    assert np.float32(st.integral_image).tobytes() == ex.integral_image.tobytes(), (what, st.integral_image, ex.integral_image)
    if ex.unclamped < 7 or ex.unclamped > 20:
        assert st.grad_mean == float(ex.grad_mean) and st.grad_mean in (7.0, 20.0), (what, st.grad_mean)
        return
    assert 7.5 < ex.unclamped < 19.5
    dev = abs(st.grad_mean - float(ex.grad_mean)) / float(ex.grad_mean)
    print("grad_mean deviation %dx%d %s: %.3e (device %.9g, exact %.9g)" % (ex.width, ex.height, what, dev, st.grad_mean,
                                                                             float(ex.grad_mean)))
    assert dev <= GRAD_MEAN_REL, (what, st.grad_mean, float(ex.grad_mean), dev)


def _check_gradients(ctx, fid, ref, what):
    w, h = ref.stats.width, ref.stats.height
    for l in range(3):
        gx, gy = ctx.frame_sobel(fid, l, w, h)
        assert gx.shape == ref.sobel[l][0].shape
        assert np.array_equal(gx, ref.sobel[l][0]) and np.array_equal(gy, ref.sobel[l][1]), (what, "sobel level %d" % l)


def _check_frame(ctx, mode, fid, st, ref, what):
    """a resident frame against its reference: statistics (returned and resident; lazy: before and after the Sobel download),
    the five levels, the six gradient images"""
    w, h = ref.stats.width, ref.stats.height
    if st is not None:
        _check_stats(st, ref.stats, what + " returned")
    _check_stats(ctx.debug_frame_stats(fid), ref.stats, what + " resident")
    for l in range(5):
        assert np.array_equal(ctx.frame_level(fid, l, w, h), ref.levels[l]), (what, "pyramid level %d" % l)
    _check_gradients(ctx, fid, ref, what)
    if mode == "lazy":          # the store pass (SOB_STORE) left the partials and the record alone
        _check_stats(ctx.debug_frame_stats(fid), ref.stats, what + " resident after the Sobel download")


@pytest.mark.parametrize("name", list(TEXTURES))
@pytest.mark.parametrize("mode", ["lazy", "eager"])
@pytest.mark.parametrize("size", SHAPES, ids=IDS)
def test_frame_against_exact_references(ctxs, refs, size, mode, name):
    ctx, ref = ctxs[mode], refs[size, name]
    _input_regime(ref.stats, name)
    assert [l.shape for l in ref.levels[1:]] == [(lh, lw) for lw, lh in SMALL_SHAPES[size][1]]
    _release(ctx, [100])
    st = ctx.frame_upload(100, ref.img)
    try:
        _check_frame(ctx, mode, 100, st, ref, "%s %s" % (mode, name))
    finally:
        _release(ctx, [100])


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("mode", ["lazy", "eager"])
@pytest.mark.parametrize("size", PLUMBING, ids=PLUMBING_IDS)
def test_three_frames_in_one_batch(ctxs, refs, size, mode, source):
    """blockIdx.y into bases and part[]: no frame picks up a neighbour's partials.  Three regimes side by side (7.0, unclamped,
    20.0); each frame's record equals its single upload's byte for byte and meets the reference.  device: resident sources
    (k_pyramid's fused copy on 192x128, k_copy_level0 on the cv::resize shape)."""
    ctx = ctxs[mode]
    w, h = size
    names = ["k4", "k16", "noise"]
    for n in names:
        _input_regime(refs[size, n].stats, n)
    ids, solo = [210, 211, 212], []
    _release(ctx, ids + [213])
    try:
        for n in names:
            solo.append(bytes(ctx.frame_upload(213, refs[size, n].img)))
            ctx.frame_release(213)
        if source == "host":
            sts = ctx.frame_upload_batch(ids, imgs=[refs[size, n].img for n in names])
        else:
            import torch
            dev = [torch.from_numpy(refs[size, n].img).cuda() for n in names]
            sts = ctx.frame_upload_batch(ids, device_ptrs=[t.data_ptr() for t in dev], width=w, height=h)
        for k, n in enumerate(names):
            assert bytes(sts[k]) == solo[k], n
            assert bytes(ctx.debug_frame_stats(ids[k])) == solo[k], n
        for k, n in enumerate(names):
            _check_frame(ctx, mode, ids[k], sts[k], refs[size, n], "%s batch[%d] %s %s" % (mode, k, source, n))
        for k, n in enumerate(names):     # ... and a neighbour's Sobel download changed nobody's record
            assert bytes(ctx.debug_frame_stats(ids[k])) == solo[k], n
    finally:
        _release(ctx, ids + [213])


@pytest.mark.parametrize("mode", ["lazy", "eager"])
@pytest.mark.parametrize("size", PLUMBING, ids=PLUMBING_IDS)
def test_refresh_in_place_follows_the_pixels(ctxs, refs, size, mode):
    """noise -> k16 -> constant under one id: statistics and gradient images are the new pixels' (stale partials or stale
    gradient images would show against the reference; nothing here is compared with the other context)"""
    ctx = ctxs[mode]
    _release(ctx, [220])
    try:
        for n in ["noise", "k16", "constant"]:
            _input_regime(refs[size, n].stats, n)
            st = ctx.frame_upload_batch([220], imgs=[refs[size, n].img])[0]
            _check_frame(ctx, mode, 220, st, refs[size, n], "%s refresh to %s" % (mode, n))
        flat = refs[size, "constant"]
        assert flat.stats.integral_image == np.float32(CONSTANT) and not any(g.any() for pair in flat.sobel for g in pair)
    finally:
        _release(ctx, [220])


@pytest.mark.parametrize("mode", ["lazy", "eager"])
@pytest.mark.parametrize("size", PLUMBING, ids=PLUMBING_IDS)
def test_recycled_allocation(ctxs, refs, size, mode):
    """an allocation that held noise (partials, record and gradient images) comes back from the free list for a new id"""
    ctx = ctxs[mode]
    w, h = size
    _release(ctx, [230, 231])
    try:
        _input_regime(refs[size, "k16"].stats, "k16")
        ctx.frame_upload(230, refs[size, "noise"].img)
        ctx.frame_sobel(230, 0, w, h)
        ctx.frame_release(230)
        st = ctx.frame_upload(231, refs[size, "k16"].img)
        _check_frame(ctx, mode, 231, st, refs[size, "k16"], "%s recycled" % mode)
    finally:
        _release(ctx, [230, 231])
