"""hso_vo_options.resize without a GPU: the option is the second of the words the struct reserved, off by default, and an engine
linked against a device library that lacks hso_gpu_frame_upload_batch_resized (tests/fakegpu: the reference is weak) answers it
with HSO_E_UNSUPPORTED and goes on working."""
import ctypes as C

import numpy as np

from hso_amd import capi, synth, vo
from test_engine_cpu import fake, small_seq  # noqa: F401  (fixtures)

REFUSAL = "Frame: provided image has not the same size as the camera model or image is not grayscale"


def test_unsupported_against_a_device_library_without_the_entry(fake, small_seq):  # noqa: F811
    assert not hasattr(fake, "hso_gpu_frame_upload_batch_resized")
    S = small_seq
    odo = vo.VisualOdometry(synth.camera(S["spec"]), 80, lib=fake)
    o = vo.VoOptions(C.sizeof(vo.VoOptions))
    o.resize = 1
    assert fake.hso_vo_set_options(odo.h, C.byref(o)) == capi.E_UNSUPPORTED
    assert b"hso_gpu_frame_upload_batch_resized" in fake.hso_vo_last_error(odo.h)
    # nothing was set: a wrong-size image is refused as ever, and the handle runs the sequence
    big = np.zeros((S["images"][0].shape[0] * 2, S["images"][0].shape[1] * 2), np.uint8)
    assert fake.hso_vo_add_image(odo.h, capi._ptr(big), big.shape[1], big.shape[0], 0.0) == capi.E_INVALID
    assert fake.hso_vo_last_error(odo.h).decode() == REFUSAL
    o.resize = 0
    assert fake.hso_vo_set_options(odo.h, C.byref(o)) == 0
    odo.set_first_frame(S["images"][0], S["depth0"], 0.0)
    assert odo.add_image(S["images"][1], 1.0).stage == 3
    odo.close()


def test_options_struct_is_unchanged_and_names_the_word():
    assert C.sizeof(vo.VoOptions) == 8 * 4
    assert [f[0] for f in vo.VoOptions._fields_] == ["size", "sync_previous", "track_no_coop", "no_numa_pin", "device_select", "reserved"]
    assert vo.VoOptions.reserved.offset == 20 and vo.VoOptions.reserved.size == 3 * 4
    o = vo.VoOptions(C.sizeof(vo.VoOptions))
    o.resize = 1
    assert list(o.reserved) == [0, 1, 0] and o.rectify == 0                 # hso_vo_options.resize: byte 24, behind rectify
    assert bytes(o)[24:28] == (1).to_bytes(4, "little")


def test_default_is_off():
    o = vo.VoOptions(C.sizeof(vo.VoOptions))
    assert o.resize == 0 and o.rectify == 0
    import inspect
    for cls in (vo.VisualOdometry, vo.MultiVisualOdometry):
        assert inspect.signature(cls.set_options).parameters["resize"].default is False


def test_device_library_exports_and_binds_the_entry():
    from hso_amd import build
    build.build()
    lib = capi.load()
    name = "hso_gpu_frame_upload_batch_resized"
    assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
    assert callable(capi.Context.frame_upload_batch_resized)
    assert lib.hso_gpu_frame_upload_batch_resized(None, None, None, 0, 0, 0, 0, 0, -1, 0, None) == capi.E_INVALID     # before anything touches a device
