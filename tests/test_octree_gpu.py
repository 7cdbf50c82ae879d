"""The oct-tree distribution on the device (hso_amd/csrc/hso_octree_dev.hip: hso_gpu_select_octree_batch, and fused behind the
detection: hso_gpu_detect_select_multi) against the host function hso_gpu_select_octree on the same keys — byte for byte: the same
keys, in the same order, the same count.  tests/test_octree.py ties the host function to the list restatement (oracle/octree_py.py).
No tolerance anywhere: the arithmetic is integer work, float comparisons and one correctly rounded float division."""
import numpy as np
import pytest

from hso_amd import capi, synth, vo

pytestmark = pytest.mark.gpu

OCCUR = capi.KP_OCCUR
KP = capi.KEYPOINT_DTYPE


def _random_keys(rng, n, width, height, n_occur=0, clustered=False):
    """the key generator of tests/test_octree.py: lattice positions, response ties, sub-pixel occupancy keys first"""
    keys = np.zeros(n + n_occur, KP)
    if clustered:
        c = rng.integers(0, 6, n + n_occur)
        cx = np.array([50, 300, 320, 600, 610, 100])[c] + rng.normal(0, 12, n + n_occur)
        cy = np.array([40, 200, 240, 440, 100, 400])[c] + rng.normal(0, 9, n + n_occur)
        keys["x"] = np.clip(cx, 0, width - 1).astype(np.int32)
        keys["y"] = np.clip(cy, 0, height - 1).astype(np.int32)
    else:
        keys["x"] = rng.integers(0, width, n + n_occur)
        keys["y"] = rng.integers(0, height, n + n_occur)
    lvl = rng.integers(0, 3, n + n_occur)
    keys["x"] = (keys["x"].astype(np.int32) >> lvl) << lvl          # level-L candidates sit on a 2^L lattice
    keys["y"] = (keys["y"].astype(np.int32) >> lvl) << lvl
    keys["level"] = lvl
    keys["species"] = rng.integers(0, 2, n + n_occur)
    keys["response"] = rng.integers(0, 40, n + n_occur) * 12.5        # ties in the response on purpose
    keys["gx"], keys["gy"] = rng.integers(-900, 900, n + n_occur), rng.integers(-900, 900, n + n_occur)
    if n_occur:
        keys["species"][:n_occur] = OCCUR                             # existing features come first
        keys["x"][:n_occur] = rng.uniform(0, width - 1, n_occur)      # sub-pixel positions
        keys["y"][:n_occur] = rng.uniform(0, height - 1, n_occur)
        keys["response"][:n_occur] = 0
        keys["level"][:n_occur] = 0
    return keys


# (n, n_occur, n_features, clustered); sets of one n_features share a call (n_features is call-wide)
CASES = [(3000, 0, 300, False), (3000, 120, 300, False), (9000, 60, 2000, False), (800, 0, 2100, False),
         (2500, 80, 300, True), (40, 5, 300, False), (1, 0, 300, False)]


@pytest.mark.parametrize("width,height", [(752, 480), (640, 480), (920, 736)])
def test_batch_equals_the_host_function(gpu_ctx, width, height):
    sets = {}
    for n, n_occur, n_features, clustered in CASES:
        rng = np.random.default_rng(n * 7 + n_occur + width)
        sets.setdefault(n_features, []).append(_random_keys(rng, n, width, height, n_occur, clustered))
    sets[300].insert(2, np.zeros(0, KP))                              # an empty set in the middle
    assert sorted(sets) == [300, 2000, 2100] and len(sets[300]) == 6
    for n_features, group in sets.items():
        got, n_out = gpu_ctx.select_octree_batch(group, width, height, n_features)
        for k, keys in enumerate(group):
            want = capi.select_octree(keys, width, height, n_features)
            assert n_out[k] == len(want), (n_features, k, len(keys), int(n_out[k]), len(want))
            assert got[k].tobytes() == want.tobytes(), (n_features, k, len(keys))
        # a set alone = the same set inside the batch
        k = 1 if len(group) > 1 else 0
        alone, n_alone = gpu_ctx.select_octree_batch([group[k]], width, height, n_features)
        assert n_alone[0] == n_out[k] and alone[0].tobytes() == got[k].tobytes()
    # the second phase really ran with a long sort (9000 keys for 2000 nodes) and the 2100 case ended short of its budget
    assert len(capi.select_octree(sets[2100][0], width, height, 2100)) < 2100


def test_hand_cases(gpu_ctx):
    same = np.zeros(5, KP)                                            # coincident keys can never be separated
    same["x"], same["y"] = 100, 100
    same["response"] = [1, 5, 3, 5, 2]
    same["gx"] = np.arange(5)                                         # tells the two response-5 keys apart
    two = np.zeros(2, KP)                                             # a corner beats an edgelet with a higher response
    two["x"], two["y"] = [10, 10], [10, 10]
    two["species"], two["response"] = [capi.KP_EDGELET, capi.KP_CORNER_HIGH], [900, 1]
    occ = np.zeros(3, KP)                                             # an occupancy key silences its node
    occ["x"], occ["y"] = [10.4, 10, 300], [10.2, 10, 300]
    occ["species"] = [OCCUR, capi.KP_CORNER_HIGH, capi.KP_CORNER_HIGH]
    bad = np.zeros(3, KP)                                             # x = 700 in a 640-wide rectangle: this set only is invalid
    bad["x"], bad["y"] = [5, 700, 300], [5, 5, 5]
    zero = np.zeros(2, KP)                                            # -0.0 and +0.0 tie: the earlier key stays
    zero["x"], zero["y"] = 50, 50
    zero["response"] = [-0.0, 0.0]
    zero["gx"] = [1, 2]
    group = [same, two, occ, bad, zero]
    got, n_out = gpu_ctx.select_octree_batch(group, 640, 480, 300)
    assert n_out.tolist() == [1, 1, 1, capi.E_INVALID, 1]
    assert got[0][0]["response"] == 5 and got[0][0]["gx"] == 1        # the second input
    assert got[1][0]["species"] == capi.KP_CORNER_HIGH
    assert got[2][0]["x"] == 300
    assert len(got[3]) == 0
    assert got[4][0]["gx"] == 1
    for k in (0, 1, 2, 4):
        assert got[k].tobytes() == capi.select_octree(group[k], 640, 480, 300).tobytes()
    # out_cap smaller than the count: the first out_cap keys and the full count
    rng = np.random.default_rng(12)
    keys = _random_keys(rng, 500, 640, 480)
    want = capi.select_octree(keys, 640, 480, 100)
    assert len(want) > 40
    got, n_out = gpu_ctx.select_octree_batch([keys, same], 640, 480, 100, out_cap=40)
    assert n_out.tolist() == [len(want), 1]
    assert got[0].tobytes() == want[:40].tobytes() and got[1][0]["gx"] == 1
    # limits and bad arguments are call-wide statuses
    with pytest.raises(capi.HsoGpuError):
        gpu_ctx.select_octree_batch([keys], 640, 480, 5000)
    with pytest.raises(capi.HsoGpuError):
        gpu_ctx.select_octree_batch([keys], 0, 480, 100)


def _assemble(occ_xy, co, cc, eo, ec, k, n_levels=3):
    """allFeturesToDistribute_ of frame k the way Bank::detect (hso_amd/host/hso_engine_kf.cpp) builds it"""
    o = np.zeros(len(occ_xy), KP)
    o["x"], o["y"], o["species"] = occ_xy[:, 0], occ_xy[:, 1], OCCUR
    parts = [o]
    for L in range(n_levels):
        c = co[k, L, :cc[k, L]]
        a = np.zeros(len(c), KP)
        a["x"], a["y"] = c["x"].astype(np.int32) << L, c["y"].astype(np.int32) << L
        a["response"], a["level"], a["species"] = c["response"], L, capi.KP_CORNER_HIGH
        e = eo[k, L, :ec[k, L]]
        b = np.zeros(len(e), KP)
        b["x"], b["y"] = e["x"].astype(np.int32) << L, e["y"].astype(np.int32) << L
        b["response"], b["level"], b["species"], b["gx"], b["gy"] = e["grad"], L, capi.KP_EDGELET, e["gx"], e["gy"]
        parts += [a, b]
    return np.concatenate(parts)


def test_fused_detection_and_selection(gpu_ctx):
    h, w = 480, 640
    rng = np.random.default_rng(5)
    imgs = [synth.config2_pair(10, seed=71)["ref"], synth.config2_pair(10, seed=72)["ref"],
            (np.kron(rng.integers(0, 2, (h // 8, w // 8)), np.ones((8, 8))) * 40 + 60).astype(np.uint8)]
    ths = [12, 5, 27]
    ids = [9860 + k for k in range(len(imgs))]
    for i, im in zip(ids, imgs):
        gpu_ctx.frame_upload(i, im)
    try:
        first = gpu_ctx.detect_candidates_multi(ids, ths, n_levels=3, corner_cap=40000, edgelet_cap=4800)
        co, cc, eo, ec = first
        assert cc[1, 0] > 150 and cc.max() > 8
        # occupancy positions: none, 150 real corner positions of the frame (its nodes are silenced), 40 random sub-pixel ones
        pick = rng.choice(cc[1, 0], 150, replace=False)
        occ = [np.zeros((0, 2), np.float32),
               np.stack([co[1, 0, pick]["x"], co[1, 0, pick]["y"]], 1).astype(np.float32),
               np.stack([rng.uniform(0, w - 1, 40), rng.uniform(0, h - 1, 40)], 1).astype(np.float32)]
        n_features = 300
        want = [capi.select_octree(_assemble(occ[k], co, cc, eo, ec, k), w, h, n_features) for k in range(3)]
        silenced = capi.select_octree(_assemble(occ[0], co, cc, eo, ec, 1), w, h, n_features)
        assert len(silenced) > len(want[1])                            # the occupancy keys of frame 1 do silence nodes
        got, n_out, gcc, gec, n_cand = gpu_ctx.detect_select_multi(ids, ths, occ, w, h, n_features, corner_cap=40000)
        assert (gcc == cc).all() and (gec == ec).all()
        assert n_cand.tolist() == [len(occ[k]) + int(cc[k].sum() + ec[k].sum()) for k in range(3)]
        for k in range(3):
            assert n_out[k] == len(want[k]) and got[k].tobytes() == want[k].tobytes(), k
        # a corner list that overflows: that frame says so, the counts are the full ones
        got8, n_out8, cc8, ec8, n_cand8 = gpu_ctx.detect_select_multi(ids, ths, occ, w, h, n_features, corner_cap=8)
        over = [bool(cc[k].max() > 8) for k in range(3)]
        assert any(over)
        assert n_out8.tolist() == [capi.E_TRUNCATED if over[k] else len(want[k]) for k in range(3)]
        assert all(len(got8[k]) == 0 if over[k] else got8[k].tobytes() == want[k].tobytes() for k in range(3))
        assert (cc8 == cc).all() and (ec8 == ec).all() and (n_cand8 == n_cand).all()
        # the detection entry is what it was
        again = gpu_ctx.detect_candidates_multi(ids, ths, n_levels=3, corner_cap=40000, edgelet_cap=4800)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    finally:
        for i in ids:
            gpu_ctx.frame_release(i)


def test_engine_with_device_selection_equals_the_host_path():
    """hso_vo_options.device_select: every status record and every keyframe of three sequences, bit for bit"""
    spec = synth.EUROC
    cam = synth.camera(spec)
    seqs = [synth.sequence(30, spec=spec, seed=3300 + 11 * k, step=(0.018 + 0.002 * k, 0.005, 0.006)) for k in range(3)]

    def run(device_select):
        multi = vo.MultiVisualOdometry(cam, len(seqs), 300)
        multi.set_options(device_select=device_select)
        multi.set_first_frames([S["images"][0] for S in seqs], [S["depth0"] for S in seqs])
        got = []
        for k in range(1, 30):
            multi.add_images([S["images"][k] for S in seqs], [float(k)] * len(seqs))
            got.append([bytes(multi.status(q)) for q in range(len(seqs))])
        kfs = [[(ts, bytes(T), fid) for ts, T, fid in multi.keyframes(q)] for q in range(len(seqs))]
        counts = multi.call_counts()
        multi.close()
        return got, kfs, counts

    on, kfs_on, counts_on = run(True)
    off, kfs_off, counts_off = run(False)
    assert on == off and kfs_on == kfs_off
    assert all(len(k) >= 2 for k in kfs_on)
    # detection ran (it is counted with the other calls), as often on either path
    assert counts_on["other"][0] > 0 and counts_on["other"] == counts_off["other"]
