"""hso_vo_options.device_select without a GPU: the option fits the struct's reserved words, the device library exports and capi
binds the two entry points behind it, and an engine linked against a device library that lacks hso_gpu_detect_select_multi
(tests/fakegpu: the reference is weak) still loads and, asked for the option, computes what it computes without it."""
import ctypes as C

from hso_amd import capi, synth, vo
from test_engine_cpu import fake, small_seq  # noqa: F401  (fixtures)


def _run(lib, S, n, max_fts, device_select):
    odo = vo.VisualOdometry(synth.camera(S["spec"]), max_fts, lib=lib)
    if device_select:
        odo.set_options(device_select=True)
    odo.set_first_frame(S["images"][0], S["depth0"], 0.0)
    out = [bytes(odo.add_image(S["images"][k], float(k))) for k in range(1, n)]
    kfs = [(a, bytes(b), c) for a, b, c in odo.keyframes()]
    odo.close()
    return out, kfs


def test_option_falls_back_when_the_device_library_lacks_the_entry(fake, small_seq):  # noqa: F811
    assert not hasattr(fake, "hso_gpu_detect_select_multi")
    on = _run(fake, small_seq, 16, 80, True)
    off = _run(fake, small_seq, 16, 80, False)
    assert len(off[1]) >= 2, "the run takes no keyframe after the first: nothing was selected"
    assert on == off


def test_options_struct_keeps_its_size():
    assert C.sizeof(vo.VoOptions) == 8 * 4
    names = [f[0] for f in vo.VoOptions._fields_]
    assert names.index("device_select") == 4 and vo.VoOptions.device_select.offset == 16
    assert vo.VoOptions.reserved.size == 3 * 4


def test_device_library_exports_and_binds_the_entries():
    from hso_amd import build
    build.build()
    lib = capi.load()
    for name in ("hso_gpu_select_octree_batch", "hso_gpu_detect_select_multi"):
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    assert callable(capi.Context.select_octree_batch) and callable(capi.Context.detect_select_multi)
    # a null context is refused before anything touches a device
    assert lib.hso_gpu_select_octree_batch(None, None, None, 0, 0, 640, 0, 480, 300, None, 0, None) == capi.E_INVALID
