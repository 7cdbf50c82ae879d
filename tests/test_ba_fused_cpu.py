"""hso_gpu_options.ba_fused / hso_vo_options.ba_fused without a GPU: the device options struct grew by one word at its end, the
engine's option took the last reserved word of its 32-byte struct, the libraries export what the bindings name, and an engine
linked against the CPU stand-in of the device library (tests/fakegpu, which has one kernel shape to offer) accepts the option and
computes what it computes without it."""
import ctypes as C

from hso_amd import capi, synth, vo
from test_engine_cpu import fake, small_seq  # noqa: F401  (fixtures)


def test_device_options_grew_by_one_word_at_the_end():
    names = [f[0] for f in capi.GpuOptions._fields_]
    assert names[-1] == "ba_fused" and names[-2] == "eager_gradients"
    assert C.sizeof(capi.GpuOptions) == 9 * 4 + 4                              # the struct of the ABI's second generation + ba_fused
    assert capi.GpuOptions.ba_fused.offset == C.sizeof(capi.GpuOptions) - 4 == capi.GpuOptions.eager_gradients.offset + 4
    assert capi.ABI_VERSION == 2
    assert "hso_gpu_ba_debug_launches" in capi.DEBUG_SYMBOLS and callable(capi.Context.ba_debug_launches)
    assert capi.BA_FUSED_ROUNDS >= 10                                          # the engine's windows (8-10 rounds) fit one launch


def test_engine_options_keep_their_size():
    assert C.sizeof(vo.VoOptions) == 32
    assert vo.VoOptions.reserved.offset == 20 and vo.VoOptions.reserved.size == 12
    o = vo.VoOptions(C.sizeof(vo.VoOptions))
    o.ba_fused = 1
    assert (o.rectify, o.resize, o.ba_fused) == (0, 0, 1)
    assert bytes(o)[28:32] == (1).to_bytes(4, "little") and bytes(o)[4:28] == bytes(24)   # the third word of the array: offset 28
    assert "hso_vo_multi_ba_launches" in vo.EXPORTED_SYMBOLS


def test_libraries_export_the_entries():
    from hso_amd import build
    build.build()
    lib = capi.load()
    assert hasattr(lib, "hso_gpu_ba_debug_launches")
    out = (C.c_int64 * 2)()
    assert lib.hso_gpu_ba_debug_launches(None, out) == capi.E_INVALID         # a null context is refused before anything touches a device
    assert lib.hso_gpu_configure(None, None) == capi.E_INVALID
    assert hasattr(vo.load(), "hso_vo_multi_ba_launches")


def _run(lib, S, n, max_fts, ba_fused):
    odo = vo.VisualOdometry(synth.camera(S["spec"]), max_fts, lib=lib)
    if ba_fused:
        o = vo.VoOptions(C.sizeof(vo.VoOptions))
        o.ba_fused = 1
        assert lib.hso_vo_set_options(odo.h, C.byref(o)) == 0
    odo.set_first_frame(S["images"][0], S["depth0"], 0.0)
    out = [bytes(odo.add_image(S["images"][k], float(k))) for k in range(1, n)]
    kfs = [(a, bytes(b), c) for a, b, c in odo.keyframes()]
    odo.close()
    return out, kfs


def test_stand_in_accepts_the_option_and_ignores_it(fake, small_seq):  # noqa: F811
    assert not hasattr(fake, "hso_gpu_ba_debug_launches")
    on = _run(fake, small_seq, 16, 80, True)
    off = _run(fake, small_seq, 16, 80, False)
    assert len(off[1]) >= 2, "the run takes no keyframe after the first: no local BA ran"
    assert on == off


def test_stand_in_bank_reports_no_launch_counter(fake, small_seq):  # noqa: F811
    bank = vo.MultiVisualOdometry(synth.camera(small_seq["spec"]), 1, 80, lib=fake)
    bank.set_options(ba_fused=True)
    out = (C.c_int64 * 2)()
    fake.hso_vo_multi_ba_launches.argtypes = [C.c_void_p, C.c_void_p]
    assert fake.hso_vo_multi_ba_launches(bank.h, out) == capi.E_UNSUPPORTED
    bank.close()
