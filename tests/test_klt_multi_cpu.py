"""hso_gpu_klt_track_multi without a GPU: the built library exports and binds it and refuses a NULL context before anything touches
a device; the engine linked against tests/fakegpu (which has no such entry) still starts sequences from images through one
hso_gpu_klt_track call per sequence; and the host half of the batched call — the engine's table concatenation and the device
library's range checks — runs in a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hso_amd import capi, synth, vo

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE_LIB = os.path.join(HERE, "fakegpu", "libhso_host_fake.so")
SMALL = dict(synth.EUROC, width=384, height=256, fx=240.0, fy=240.0, cx=191.5, cy=127.5)   # tests/test_engine_cpu.py's camera


@pytest.fixture(scope="module")
def fake(orc):
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "fakegpu")])
    return vo.load_from(FAKE_LIB)


def test_library_exports_and_binds_the_batched_call():
    lib = capi.load()
    assert "hso_gpu_klt_track_multi" in capi.EXPORTED_SYMBOLS and hasattr(lib, "hso_gpu_klt_track_multi")
    assert lib.hso_gpu_klt_track_multi.argtypes is not None and len(lib.hso_gpu_klt_track_multi.argtypes) == 8
    assert capi.KLT_PAIR_DTYPE.itemsize == 24                          # hso_klt_pair: two int64, two int32
    assert callable(capi.Context.klt_track_multi)


def test_null_context_is_refused_before_anything_touches_a_device():
    lib = capi.load()
    tab = np.zeros(1, capi.KLT_PAIR_DTYPE)
    tab[0] = (1, 2, 0, 4)
    px = np.zeros((4, 2), np.float32)
    out = np.zeros(4, capi.KLT_RESULT_DTYPE)
    params = capi.KltParams()
    rc = lib.hso_gpu_klt_track_multi(None, capi._ptr(tab), 1, capi._ptr(px), capi._ptr(px), 4, C.byref(params), capi._ptr(out))
    assert rc == -1                                                    # HSO_E_INVALID
    assert lib.hso_gpu_klt_track(None, 1, 2, capi._ptr(px), capi._ptr(px), 4, C.byref(params), capi._ptr(out)) == -1


def test_engine_without_the_batched_entry_starts_from_images(fake):
    """tests/fakegpu has no hso_gpu_klt_track_multi: the engine keeps one KLT call per sequence there, and two sequences started
    from images reach stage 3; kind [9] of the call counts shows the per-sequence calls (calls == items for the KLT steps)."""
    names = subprocess.run(["nm", "-D", "--defined-only", FAKE_LIB], capture_output=True, text=True, check=True).stdout.split()
    assert "hso_gpu_klt_track" in names and "hso_gpu_klt_track_multi" not in names
    spec = dict(SMALL, texture_om=((0.004, 0.05), (0.05, 0.6)))
    cam = synth.camera(spec)
    seqs = [synth.sequence(10, spec=spec, seed=4300 + 7 * k, workers=4, step=(0.10 + 0.03 * k, 0.015, 0.01), rot_deg_per_frame=(0.05, -0.1, 0.03)) for k in range(2)]
    solo = []
    for S in seqs:
        odo = vo.VisualOdometry(cam, 120, lib=fake)
        odo.start()
        solo.append([bytes(odo.add_image(im, float(k))) for k, im in enumerate(S["images"])])
        odo.close()
    bank = vo.MultiVisualOdometry(cam, 2, 120, lib=fake)
    bank.start()
    got = [[], []]
    for k in range(10):
        stage = [bank.status(q).stage for q in range(2)]
        c0 = bank.call_counts()["other"]
        bank.add_images([S["images"][k] for S in seqs], [float(k)] * 2)
        c1 = bank.call_counts()["other"]
        if stage == [2, 2]:
            assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 2), (k, c0, c1)   # the fallback: a call per sequence
        for q in range(2):
            got[q].append(bytes(bank.status(q)))
    final = [bank.status(q).stage for q in range(2)]
    bank.close()
    assert final == [3, 3], final
    assert got == solo


def test_host_half_under_sanitizers(tmp_path):
    """tests/klt_tables_main.cpp: concatenation, slices, range checks and the per-row pair index, compiled with
    -fsanitize=address,undefined into a program of its own (nothing of it is loaded into this process)."""
    exe = str(tmp_path / "klt_tables")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "klt_tables_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-400:], out.stderr[-2000:])
