"""hso_vo_get_map_points / hso_vo_get_seeds and their hso_vo_multi_* forms on a rendered sequence: the exported points lie in front
of their host keyframes and project onto the pixel whose level-0 value is their colour; a sequence in either slot of a two-sequence
bank exports what it exports alone, bit for bit; run_sequence's cloud= / seeds= files read back to the same arrays."""
import numpy as np
import pytest

import map_export_ref as ref
from hso_amd import capi, formats, synth, vo

pytestmark = pytest.mark.gpu

# the small camera of the engine tests, without lens distortion: the test projects the points itself
SPEC = dict(synth.EUROC, width=384, height=256, fx=240.0, fy=240.0, cx=191.5, cy=127.5, d=(0.0, 0.0, 0.0, 0.0, 0.0))
MOTION = dict(step=(0.05, 0.015, 0.02), rot_deg_per_frame=(0.1, -0.3, 0.08))
W, H = SPEC["width"], SPEC["height"]
N, MAX_FTS = 24, 120
ROUNDING = 1e-9          # px: far above the rounding error of a recomputed projection, far below any sub-pixel feature offset


@pytest.fixture(scope="module")
def seq():
    return synth.sequence(N, spec=SPEC, workers=4, **MOTION)


@pytest.fixture(scope="module")
def solo(seq):
    """the sequence alone: the exports after the last frame, the keyframes, and which frame each keyframe id names"""
    odo = vo.VisualOdometry(synth.camera(SPEC), MAX_FTS)
    odo.set_first_frame(seq["images"][0], seq["depth0"], 0.0)
    early = odo.map_points()                                   # right after set_first_frame: valid, and the first keyframe's points
    st = odo.status()
    kf_frame = {int(st.keyframe_id): int(st.frame_id)}
    for k in range(1, N):
        st = odo.add_image(seq["images"][k], float(k))
        if st.is_keyframe:
            kf_frame[int(st.keyframe_id)] = int(st.frame_id)
    out = dict(points=odo.map_points(), all_points=odo.map_points(type_mask=0xfffe, min_obs=0), seeds=odo.seeds(), early=early,
               keyframes=odo.keyframes(), kf_frame=kf_frame, stage=odo.status().stage)
    odo.close()
    return out


def test_points_lie_on_their_colour(seq, solo):
    pts = solo["points"]
    assert solo["stage"] == 3 and len(solo["keyframes"]) >= 3 and len(pts) > 50 and len(solo["early"]) > 20
    assert (np.diff(pts["point"]) > 0).all() and set(pts["type"]) <= {3, 4} and (pts["n_obs"] >= 1).all()
    # level 0 of every keyframe as the device holds it
    ctx = capi.Context(0)
    pose, level0 = {}, {}
    for ts, T, fid in solo["keyframes"]:
        q, t = T.to_arrays()
        pose[fid] = (ref.quat_matrix(q), t)
        ctx.frame_upload(fid + 1, seq["images"][fid])
        level0[fid] = ctx.frame_level(fid + 1, 0, W, H)
    ctx.close()
    n_off = 0
    for r in pts:
        assert int(r["keyframe_id"]) in solo["kf_frame"]
        fid = solo["kf_frame"][int(r["keyframe_id"])]
        R, t = pose[fid]
        p = R @ r["pos"] + t
        assert p[2] > 0                                                   # in front of its host keyframe
        u, v = SPEC["fx"] * p[0] / p[2] + SPEC["cx"], SPEC["fy"] * p[1] / p[2] + SPEC["cy"]
        assert 0 <= u < W and 0 <= v < H
        # The detector's features sit on whole pixels, and the projection recomputed here carries fp64 rounding (about twenty
        # operations on values below 384: under 2e-12 px; 6e-14 measured), so a feature at x.0 comes back as x - 1e-13 as often as
        # not and a bare (int) lands one pixel off (241 of 2000 points did).  The pixel is the one under u + 1e-9.
        n_off += int(level0[fid][int(v + ROUNDING), int(u + ROUNDING)] != r["color"])
    print("exported points: %d, colour differs from the pixel under the projection: %d" % (len(pts), n_off))
    assert n_off == 0


def test_seeds_are_live_and_coloured(solo):
    s = solo["seeds"]
    assert len(s) > 20 and (np.diff(s["slot"]) > 0).all() and (s["group"] == 0).all()
    assert (s["mu"] > 0).all() and np.isfinite(s["pos"]).all() and len(set(s["color"])) > 4


def test_bank_slots_equal_the_solo_run(seq, solo):
    bank = vo.MultiVisualOdometry(synth.camera(SPEC), 2, MAX_FTS)
    bank.set_first_frames([seq["images"][0]] * 2, [seq["depth0"]] * 2)
    for k in range(1, N):
        bank.add_images([seq["images"][k]] * 2, [float(k)] * 2)
    both, begin = bank.map_points(-1)
    assert list(begin) == [0, len(solo["points"]), 2 * len(solo["points"])]
    for q in range(2):
        one, b = bank.map_points(q)
        assert list(b) == [0, len(one)]
        assert one.tobytes() == solo["points"].tobytes() == both[begin[q]:begin[q + 1]].tobytes()
        wide, _ = bank.map_points(q, type_mask=0xfffe, min_obs=0)
        assert wide.tobytes() == solo["all_points"].tobytes()
        s = bank.seeds(q)
        assert (s["group"] == q).all()
        for name in capi.SEED_EXPORT_DTYPE.names:
            if name not in ("group", "slot"):                             # one table serves the bank: the slots interleave
                assert s[name].tobytes() == solo["seeds"][name].tobytes(), name
    every = bank.seeds(-1)
    assert len(every) == 2 * len(solo["seeds"]) and (np.diff(every["slot"]) > 0).all()
    bank.close()


def test_run_sequence_writes_the_clouds(seq, solo, tmp_path):
    from hso_amd import run_sequence
    cam_file = tmp_path / "cam.txt"
    cam_file.write_text("Pinhole %r %r %r %r 0 0 0 0\n%d %d\n" % (SPEC["fx"], SPEC["fy"], SPEC["cx"], SPEC["cy"], W, H))
    np.save(str(tmp_path / "d0.npy"), seq["depth0"])
    folder = tmp_path / "images"
    folder.mkdir()
    for k, im in enumerate(seq["images"]):
        formats.write_png(str(folder / ("%05d.png" % k)), im)
    cloud, seeds = str(tmp_path / "out" / "cloud.ply"), str(tmp_path / "out" / "seeds.ply")
    line = run_sequence.main([str(folder), "None", str(cam_file), "depth0=" + str(tmp_path / "d0.npy"), "result=" + str(tmp_path / "kf.txt"),
                              "max_fts=%d" % MAX_FTS, "cloud=" + cloud, "seeds=" + seeds], return_line=True)
    c, s = formats.load_ply(cloud), formats.load_ply(seeds)
    assert line["n_cloud"] == len(c) == len(solo["points"]) and line["n_seeds"] == len(s) == len(solo["seeds"])
    for rec, v in ((solo["points"], c), (solo["seeds"], s)):
        assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), rec["pos"])
        assert np.array_equal(v["red"], rec["color"]) and np.array_equal(v["green"], rec["color"]) and np.array_equal(v["blue"], rec["color"])
        assert np.array_equal(v["type"], rec["type"])
    assert np.array_equal(c["n_obs"], solo["points"]["n_obs"]) and np.array_equal(s["sigma2"], solo["seeds"]["sigma2"])
    assert "sigma2" not in c.dtype.names and "n_obs" not in s.dtype.names
