"""The map export's host side, no GPU: the PLY writer / reader of hso_amd/formats.py, the layout of the two record structs against
the binding's dtypes, the declared-implies-exported rule for the new names, and the engine over the CPU stand-in of the device
library (tests/fakegpu has no export entries): all four hso_vo* calls answer HSO_E_UNSUPPORTED and the handle stays usable."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hso_amd import capi, formats, synth, vo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SMALL = dict(synth.EUROC, width=384, height=256, fx=240.0, fy=240.0, cx=191.5, cy=127.5)


def hand_made():
    pts = np.zeros(5, capi.POINT_EXPORT_DTYPE)
    pts["pos"] = [[0.1, -2.5, 3.0], [1e-300, 1e300, -0.0], [np.pi, np.e, 1 / 3], [4, 5, 6], [-7.25, 8.5, -9.75]]
    pts["point"], pts["keyframe_id"], pts["n_obs"] = [0, 3, 9, 2 ** 31 - 1, 12], [1, 1, 2, 7, -1], [1, 2, 70000, 4, 0]
    pts["color"], pts["type"], pts["ftr_type"] = [0, 128, 255, 17, 200], [3, 4, 3, 4, 15], [0, 1, 2, 0, 1]
    seeds = np.zeros(3, capi.SEED_EXPORT_DTYPE)
    seeds["pos"] = [[1, 2, 3], [-4.5, 5.5, 6.125], [7e-9, 8e9, 9]]
    seeds["mu"], seeds["sigma2"], seeds["slot"], seeds["group"] = [0.5, 2.0, 1e-3], [1e-4, 0.25, 3.0], [0, 5, 6], [0, 1, 1]
    seeds["color"], seeds["type"], seeds["level"] = [1, 2, 3], [0, 1, 2], [0, 1, 2]
    return pts, seeds


def test_ply_round_trip_and_header(tmp_path):
    pts, seeds = hand_made()
    p, s, e = str(tmp_path / "p.ply"), str(tmp_path / "s.ply"), str(tmp_path / "e.ply")
    formats.save_ply(p, pts)
    formats.save_ply(s, seeds)
    formats.save_ply(e, pts[:0])
    head = ("ply\nformat binary_little_endian 1.0\ncomment hso_amd map export\nelement vertex %d\nproperty double x\nproperty double y\n"
            "property double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n")
    want_p = (head % 5 + "property uchar type\nproperty int n_obs\nend_header\n").encode()
    want_s = (head % 3 + "property uchar type\nproperty float sigma2\nend_header\n").encode()
    raw_p, raw_s = open(p, "rb").read(), open(s, "rb").read()
    assert raw_p[:len(want_p)] == want_p and len(raw_p) == len(want_p) + 5 * (24 + 3 + 1 + 4)
    assert raw_s[:len(want_s)] == want_s and len(raw_s) == len(want_s) + 3 * (24 + 3 + 1 + 4)
    assert raw_p[len(want_p):len(want_p) + 24] == pts["pos"][0].astype("<f8").tobytes()         # little-endian doubles, packed
    for path, rec, extra in ((p, pts, "n_obs"), (s, seeds, "sigma2")):
        v = formats.load_ply(path)
        assert v.dtype.names == ("x", "y", "z", "red", "green", "blue", "type", extra)
        assert np.stack([v["x"], v["y"], v["z"]], 1).tobytes() == rec["pos"].tobytes()           # bits, -0.0 included
        for ch in ("red", "green", "blue"):
            assert np.array_equal(v[ch], rec["color"])
        assert np.array_equal(v["type"], rec["type"]) and np.array_equal(v[extra], rec[extra])
    assert len(formats.load_ply(e)) == 0
    with pytest.raises(ValueError):
        open(e, "wb").write(raw_p[:-1])
        formats.load_ply(e)


def test_record_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of hso_point_export and hso_seed_export as a C compiler lays them out = the binding's dtypes"""
    names = {"hso_point_export": capi.POINT_EXPORT_DTYPE, "hso_seed_export": capi.SEED_EXPORT_DTYPE}
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "hso_gpu.h"', "int main(void) {"]
    for st, dt in names.items():
        src.append('printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        src += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f) for f in dt.names]
    src += ["return 0; }"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(c)])
    got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["hso_point_export"]) == capi.POINT_EXPORT_DTYPE.itemsize == 40
    assert int(got["hso_seed_export"]) == capi.SEED_EXPORT_DTYPE.itemsize == 48
    for st, dt in names.items():
        for f in dt.names:
            assert int(got["%s.%s" % (st, f)]) == dt.fields[f][1], (st, f)


def test_new_names_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "hso_gpu.h")).read() + open(os.path.join(ROOT, "include", "hso_vo.h")).read()
    dev = ["hso_gpu_seqmap_export_points", "hso_gpu_seed_table_export"]
    eng = ["hso_vo_get_map_points", "hso_vo_get_seeds", "hso_vo_multi_get_map_points", "hso_vo_multi_get_seeds"]
    for name in dev + eng:
        assert "int %s(" % name in header, name
    assert set(dev) <= set(capi.EXPORTED_SYMBOLS) and set(eng) <= set(vo.EXPORTED_SYMBOLS)
    lib, host = capi.load(), vo.load()
    assert all(hasattr(lib, n) for n in dev) and all(hasattr(host, n) for n in eng)
    # the citations the header owes its readers
    assert "src/viewer.cpp:109-136" in header and "src/depth_filter.cpp:440-460" in header


@pytest.fixture(scope="module")
def fake(orc):
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "fakegpu")])
    return vo.load_from(os.path.join(HERE, "fakegpu", "libhso_host_fake.so"))


def test_engine_without_export_entries_answers_unsupported(fake):
    S = synth.sequence(4, spec=SMALL, workers=2, step=(0.05, 0.015, 0.02), rot_deg_per_frame=(0.1, -0.3, 0.08))
    cam = synth.camera(SMALL)
    odo = vo.VisualOdometry(cam, 80, lib=fake)
    odo.set_first_frame(S["images"][0], S["depth0"], 0.0)
    odo.add_image(S["images"][1], 1.0)
    n = np.full(1, -3, np.int32)
    pts, sds = np.zeros(4, capi.POINT_EXPORT_DTYPE), np.zeros(4, capi.SEED_EXPORT_DTYPE)
    assert fake.hso_vo_get_map_points(odo.h, 0x18, 1, pts.ctypes.data, 4, n.ctypes.data) == capi.E_UNSUPPORTED
    assert fake.hso_vo_get_seeds(odo.h, sds.ctypes.data, 4, n.ctypes.data) == capi.E_UNSUPPORTED
    assert b"map export" in fake.hso_vo_last_error(odo.h)
    with pytest.raises(capi.HsoGpuError):
        odo.map_points()
    st = odo.add_image(S["images"][2], 2.0)                           # the handle is as usable as before
    assert st.stage == 3 and st.frame_id == 2
    odo.close()
    bank = vo.MultiVisualOdometry(cam, 2, 80, lib=fake)
    bank.set_first_frames([S["images"][0]] * 2, [S["depth0"]] * 2)
    begin = np.full(3, -3, np.int32)
    for k in (-1, 0, 1):
        assert fake.hso_vo_multi_get_map_points(bank.h, k, 0x18, 1, pts.ctypes.data, 4, begin.ctypes.data) == capi.E_UNSUPPORTED
        assert fake.hso_vo_multi_get_seeds(bank.h, k, sds.ctypes.data, 4, n.ctypes.data) == capi.E_UNSUPPORTED
    assert fake.hso_vo_multi_get_map_points(bank.h, 2, 0x18, 1, pts.ctypes.data, 4, begin.ctypes.data) == capi.E_INVALID
    assert n[0] == -3 and list(begin) == [-3] * 3 and not pts.tobytes().strip(b"\0")
    bank.add_images([S["images"][1]] * 2, [1.0, 1.0])
    assert bank.status(1).frame_id == 1
    bank.close()
