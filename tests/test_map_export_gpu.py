"""hso_gpu_seqmap_export_points / hso_gpu_seed_table_export (hso_amd/csrc/hso_export.hip): the live rows of sequence maps and the live
seeds of a resident table, selected, coloured and packed on the device.  Maps are built through the public hso_gpu_seqmap_* calls and
the result is compared with the numpy restatement of tests/map_export_ref.py BYTE FOR BYTE — every field of a point record is a copy
or an integer decision.  A seed's position is the one computed field: it is held to 1e-12 of the seed's distance (a dozen fp64
operations: a few thousand ulps cover contracted and uncontracted forms; reasoned, not measured), everything else to equality."""
import ctypes as C

import numpy as np
import pytest

import map_export_ref as ref
from chain_state import ChainLib, pt_word
from hso_amd import capi

pytestmark = pytest.mark.gpu

CH = ref.CHUNK
N_KFS = 3
VIEWER = 0x18            # TYPE_UNKNOWN | TYPE_GOOD
E_INVALID, E_TRUNCATED = capi.E_INVALID, capi.E_TRUNCATED


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def env():
    """one context, three resident keyframe images (frame ids 1..3) shared by every map of the module"""
    ctx = capi.Context(0)
    lib = ChainLib(capi.load())
    images = [ref.image(k) for k in range(N_KFS)]
    for k, im in enumerate(images):
        ctx.frame_upload(k + 1, im)
    yield ctx, lib, images
    ctx.close()


def keyframes(n=N_KFS):
    kfs = np.zeros(n, capi.KF_DTYPE)
    kfs["frame_id"] = np.arange(1, n + 1)
    kfs["q"][:, 3] = 1
    kfs["exposure_time"] = 1
    kfs["keyframe_id"] = 10 + 3 * np.arange(n)
    return kfs


def make_tables(n, live, rng, kinds=(3, 4)):
    """n point rows with two observation rows each (2 i -> 2 i + 1); row i is live (a type of `kinds`) where live[i]"""
    pts = np.zeros(n, capi.MAP_POINT_DTYPE)
    obs = np.zeros(2 * n, capi.OBS_DTYPE)
    pts["pos"] = rng.normal(size=(n, 3)) * 5
    pts["idist"] = rng.uniform(0.1, 1, n)
    pts["host_kf"] = np.arange(n) % N_KFS
    pts["obs_begin"] = 2 * np.arange(n)
    pts["obs_count"] = 1 + np.arange(n) % 2
    for i in range(n):
        key = ((kinds[i % len(kinds)] if live[i] else 0) << 4) | (i % 3)
        pts["pad_"][i] = pt_word(key, n_fail=i % 7, n_ok=i % 11)
    obs["kf"][0::2] = pts["host_kf"]
    obs["kf"][1::2] = (pts["host_kf"] + 1) % N_KFS
    obs["pad_"][0::2] = 2 * np.arange(n) + 1
    obs["pad_"][1::2] = -1
    obs["px"] = rng.uniform(0, ref.W, size=(2 * n, 2))
    obs["f"][:, 2] = 1
    return pts, obs


def upload_map(env, pts, obs, kfs=None, point_ids=None):
    ctx, lib, images = env
    L = lib.L
    kfs = keyframes() if kfs is None else kfs
    m = C.c_int(-1)
    lib.check(ctx.h, L.hso_gpu_seqmap_create(ctx.h, C.byref(m)), "seqmap_create")
    lib.check(ctx.h, L.hso_gpu_seqmap_set_keyframes(ctx.h, m.value, _p(kfs), len(kfs)), "seqmap_set_keyframes")
    pts, obs = np.ascontiguousarray(pts), np.ascontiguousarray(obs)
    pid = np.arange(len(pts), dtype=np.int32) if point_ids is None else np.ascontiguousarray(point_ids, np.int32)
    oid = np.arange(len(obs), dtype=np.int32)
    if len(obs):
        lib.check(ctx.h, L.hso_gpu_seqmap_patch(ctx.h, m.value, None, None, 0, _p(oid), _p(obs), len(obs)), "seqmap_patch (observations)")
    if len(pts):
        lib.check(ctx.h, L.hso_gpu_seqmap_patch(ctx.h, m.value, _p(pid), _p(pts), len(pts), None, None, 0), "seqmap_patch (points)")
    return dict(map=m.value, points=pts, obs=obs, kfs=kfs, images=list(images[:len(kfs)]) + [None] * max(0, len(kfs) - len(images)))


def check_equal(env, maps, type_mask=VIEWER, min_obs=1):
    ctx = env[0]
    want, want_begin = ref.export_points(maps, type_mask, min_obs)
    got, begin, rc = ctx.seqmap_export_points([M["map"] for M in maps], type_mask, min_obs)
    assert rc == 0 and np.array_equal(begin, want_begin), (begin, want_begin)
    assert got.tobytes() == want.tobytes()
    return got


SIZES = [0, 1, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 1]
PATTERNS = {"all": lambda n: np.ones(n, bool), "none": lambda n: np.zeros(n, bool), "last_chunk": lambda n: np.arange(n) >= (max(n - 1, 0) // CH) * CH,
            "alternate": lambda n: np.arange(n) % 2 == 0}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_counts_and_compaction_edges(env, pattern):
    rng = np.random.default_rng(7)
    for n in SIZES:
        live = PATTERNS[pattern](n)
        M = upload_map(env, *make_tables(n, live, rng))
        got = check_equal(env, [M])
        assert len(got) == int(live.sum()) and np.array_equal(got["point"], np.nonzero(live)[0])


def test_several_maps_in_one_call(env):
    rng = np.random.default_rng(8)
    a = upload_map(env, *make_tables(CH + 44, np.ones(CH + 44, bool), rng))
    e = upload_map(env, *make_tables(0, np.zeros(0, bool), rng))
    b = upload_map(env, *make_tables(70, np.arange(70) % 3 != 0, rng))
    for order in ([a, e, b], [b, a, e], [e, e, a, a]):
        got = check_equal(env, order)
        assert len(got) == sum(int(ref.selected(M["points"], VIEWER, 1).sum()) for M in order)
    got, begin, rc = env[0].seqmap_export_points([], VIEWER, 1)
    assert rc == 0 and len(got) == 0 and list(begin) == [0]


def test_selection(env):
    rng = np.random.default_rng(9)
    # every type nibble, three faces each, all live; then the bad flag; then obs_count 0..2; rows 48..52 are never patched
    n = 16 * 3 + 16 + 9
    pts, obs = make_tables(n, np.ones(n, bool), rng)
    for i in range(48):
        pts["pad_"][i] = pt_word(((i // 3) << 4) | (i % 3), n_fail=i, n_ok=2 * i)
    for i in range(48, 64):
        pts["pad_"][i] = pt_word(((i - 48) << 4) | 1, bad=True)
    for i in range(64, 73):
        pts["pad_"][i] = pt_word((3 << 4) | 2)
        pts["obs_count"][i] = (i - 64) % 3
    ids = np.concatenate([np.arange(48), np.arange(53, 53 + n - 48)]).astype(np.int32)
    M = upload_map(env, pts, obs, point_ids=ids)
    # the restatement sees the table as the device holds it: rows 48..52 all zero
    full = np.zeros(int(ids.max()) + 1, capi.MAP_POINT_DTYPE)
    full[ids] = pts
    M["points"] = full
    for bit in range(32):
        for min_obs in (0, 1, 2):
            got = check_equal(env, [M], 1 << bit, min_obs)
            if bit == 0 or bit > 15:
                assert len(got) == 0                                   # type 0 is TYPE_DELETED whatever the mask says
    got = check_equal(env, [M], 0xffffffff, 0)
    assert not np.isin(np.arange(48, 53), got["point"]).any()          # never patched
    assert not np.isin(got["point"], ids[48:64]).any()                 # HSO_PT_BAD
    assert set(got["type"]) == set(range(1, 16)) and set(got["ftr_type"]) == {0, 1, 2}
    for min_obs in (0, 1, 2):
        got = check_equal(env, [M], VIEWER, min_obs)
        tail = got[got["point"] >= ids[64]]
        assert sorted(tail["n_obs"]) == sorted(c for c in [0, 1, 2] * 3 if c >= min_obs)


def test_colour(env):
    ctx, lib, images = env
    cases = [("first", 0), ("last", 3), ("absent", None)]
    corners = [(0.0, 0.0), (ref.W - 1.0, ref.H - 1.0), (ref.W - 0.001, ref.H - 0.001), (17.9, 40.2)]
    n = len(cases) * len(corners)
    pts = np.zeros(n, capi.MAP_POINT_DTYPE)
    obs = np.zeros(4 * n, capi.OBS_DTYPE)
    obs["f"][:, 2] = 1
    for i in range(n):
        (_, where), px = cases[i // len(corners)], corners[i % len(corners)]
        host = i % N_KFS
        pts[i] = ((i, 2 * i, 3 * i), 0.5, (0, 0, 1), host, 4 * i, 4, pt_word((4 << 4) | 2))
        for j in range(4):
            o = 4 * i + j
            obs["kf"][o] = host if j == where else (host + 1 + j % 2) % N_KFS
            obs["pad_"][o] = o + 1 if j < 3 else -1
            obs["px"][o] = px if j == where else (5.0 + j, 9.0 + j)          # another observation's pixel must not be taken
    M = upload_map(env, pts, obs)
    got = check_equal(env, [M])
    absent = got[len(corners) * 2:]
    assert (absent["color"] == ref.NO_COLOR).all()
    want_px = [int(images[i % N_KFS][min(int(y), ref.H - 1), min(int(x), ref.W - 1)]) for i in range(2 * len(corners)) for x, y in [corners[i % len(corners)]]]
    assert list(got["color"][:2 * len(corners)]) == want_px
    # a shorter keyframe table: rows hosted in keyframe 2 lose colour and keyframe id
    short = keyframes(2)
    lib.check(ctx.h, lib.L.hso_gpu_seqmap_set_keyframes(ctx.h, M["map"], _p(short), 2), "seqmap_set_keyframes")
    M2 = dict(M, kfs=short, images=list(images[:2]))
    got = check_equal(env, [M2])
    beyond = got[pts["host_kf"][got["point"]] == 2]
    assert len(beyond) and (beyond["color"] == ref.NO_COLOR).all() and (beyond["keyframe_id"] == -1).all()
    # a keyframe whose frame has left the device (its own context: the module's frames stay)
    own = capi.Context(0)
    try:
        for k, im in enumerate(images):
            own.frame_upload(k + 1, im)
        Mo = upload_map((own, lib, images), pts, obs)
        own.frame_release(2)
        Mo["images"] = [images[0], None, images[2]]
        want, _ = ref.export_points([Mo], VIEWER, 1)
        got, _, rc = own.seqmap_export_points([Mo["map"]], VIEWER, 1)
        assert rc == 0 and got.tobytes() == want.tobytes()
        gone = got[pts["host_kf"][got["point"]] == 1]
        assert len(gone) and (gone["color"] == ref.NO_COLOR).all() and (gone["keyframe_id"] == 13).all()
    finally:
        own.close()


def test_capacity(env):
    ctx = env[0]
    rng = np.random.default_rng(10)
    a = upload_map(env, *make_tables(CH + 9, np.arange(CH + 9) % 4 != 1, rng))
    b = upload_map(env, *make_tables(90, np.ones(90, bool), rng))
    want, want_begin = ref.export_points([a, b], VIEWER, 1)
    total, first = int(want_begin[2]), int(want_begin[1])
    guard = np.frombuffer(bytes([0xAB]) * capi.POINT_EXPORT_DTYPE.itemsize, capi.POINT_EXPORT_DTYPE)[0]
    for cap in (total, total - 1, first, 1):
        out = np.full(total + 8, guard, capi.POINT_EXPORT_DTYPE)
        got, begin, rc = ctx.seqmap_export_points([a["map"], b["map"]], VIEWER, 1, cap=cap, out=out)
        assert rc == (0 if cap >= total else E_TRUNCATED)
        assert np.array_equal(begin, want_begin)                                  # counts stay exact
        assert out[:cap].tobytes() == want[:cap].tobytes() and out[cap:].tobytes() == np.full(total + 8 - cap, guard, capi.POINT_EXPORT_DTYPE).tobytes()
    begin = np.full(3, -1, np.int32)
    maps = np.array([a["map"], b["map"]], np.int32)
    rc = ctx.lib.hso_gpu_seqmap_export_points(ctx.h, _p(maps), 2, VIEWER, 1, None, 0, _p(begin))    # the size query
    assert rc == E_TRUNCATED and np.array_equal(begin, want_begin)


def test_errors(env):
    ctx = env[0]
    L = ctx.lib
    M = upload_map(env, *make_tables(5, np.ones(5, bool), np.random.default_rng(11)))
    maps = np.array([M["map"]], np.int32)
    bad = np.array([10 ** 6], np.int32)
    begin = np.full(2, -7, np.int32)
    out = np.zeros(8, capi.POINT_EXPORT_DTYPE)
    assert L.hso_gpu_seqmap_export_points(ctx.h, _p(bad), 1, VIEWER, 1, _p(out), 8, _p(begin)) == E_INVALID
    assert L.hso_gpu_seqmap_export_points(ctx.h, _p(maps), -1, VIEWER, 1, _p(out), 8, _p(begin)) == E_INVALID
    assert L.hso_gpu_seqmap_export_points(ctx.h, _p(maps), 1, VIEWER, 1, _p(out), -1, _p(begin)) == E_INVALID
    assert L.hso_gpu_seqmap_export_points(ctx.h, _p(maps), 1, VIEWER, 1, _p(out), 8, None) == E_INVALID
    assert L.hso_gpu_seqmap_export_points(ctx.h, _p(maps), 1, VIEWER, 1, None, 8, _p(begin)) == E_INVALID
    assert list(begin) == [-7, -7] and not out.tobytes().strip(b"\0")              # nothing was written
    n = np.full(1, -7, np.int32)
    so = np.zeros(4, capi.SEED_EXPORT_DTYPE)
    assert L.hso_gpu_seed_table_export(ctx.h, 10 ** 6, None, 0, _p(so), 4, _p(n)) == E_INVALID
    t = ctx.seed_table_create()
    assert L.hso_gpu_seed_table_export(ctx.h, t, None, 0, _p(so), -1, _p(n)) == E_INVALID
    assert L.hso_gpu_seed_table_export(ctx.h, t, None, 0, _p(so), 4, None) == E_INVALID
    assert L.hso_gpu_seed_table_export(ctx.h, t, _p(np.array([-1], np.int32)), 1, _p(so), 4, _p(n)) == E_INVALID
    assert n[0] == -7
    ctx.seed_table_destroy(t)
    check_equal(env, [M])                                                           # the context is as usable as before


# ---- seeds ----------------------------------------------------------------------------------------------------------------------
def make_seeds(n, rng):
    seeds = (capi.Seed * max(n, 1))()
    for i in range(n):
        s = seeds[i]
        s.ref_frame_id = 1 + i % N_KFS
        s.level, s.type = i % 3, i % 3
        s.px[:] = [float(rng.uniform(0, ref.W)), float(rng.uniform(0, ref.H))]
        f = rng.normal(size=3) * 0.3 + [0, 0, 1]
        s.f[:] = list(f / np.linalg.norm(f))
        s.grad[:] = [1.0, 0.0]
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        s.T_ref_w = capi.SE3.from_arrays(q, rng.normal(size=3) * 3)
        s.ref_exposure = 1.0
        s.mu, s.sigma2, s.b = float(rng.uniform(0.05, 2.0)), float(rng.uniform(1e-4, 1.0)), 10.0
    return seeds


def check_seeds(env, table, seeds, group, alive, groups=None):
    ctx, _, images = env
    n = len(alive)
    want, dist = ref.export_seeds([seeds[i] for i in range(n)], group, alive, {k + 1: im for k, im in enumerate(images)}, groups)
    got, total, rc = ctx.seed_table_export(table, None if groups is None else sorted(groups))
    assert rc == 0 and total == len(want) == len(got)
    for name in capi.SEED_EXPORT_DTYPE.names:
        if name != "pos":
            assert np.array_equal(got[name], want[name]), name
    if len(want):
        err = np.linalg.norm(got["pos"] - want["pos"], axis=1)
        assert (err <= 1e-12 * dist).all(), float((err / dist).max())
    return got


@pytest.mark.parametrize("n", [0, 1, 65, CH + 1])
def test_seed_table_sizes(env, n):
    ctx = env[0]
    rng = np.random.default_rng(20 + n)
    seeds = make_seeds(n, rng)
    group = np.arange(n) % 3
    t = ctx.seed_table_create()
    if n:
        ctx.seed_table_append(t, [seeds[i] for i in range(n)], group)
    got = check_seeds(env, t, seeds, group, np.ones(n, bool))
    assert list(got["slot"]) == list(range(n))
    ctx.seed_table_destroy(t)


def test_seed_selection_groups_and_compaction(env):
    ctx = env[0]
    n = CH + 40
    rng = np.random.default_rng(30)
    seeds = make_seeds(n, rng)
    for i, mu in zip((3, 70, 130, CH + 1, CH + 2), (0.0, -0.5, float("nan"), float("inf"), -float("inf"))):
        seeds[i].mu = mu
    group = (np.arange(n) * 7) % 5
    alive = np.ones(n, bool)
    t = ctx.seed_table_create()
    ctx.seed_table_append(t, [seeds[i] for i in range(n)], group)
    dead = np.concatenate([np.arange(0, n, 3), [n - 1]])
    ctx.seed_table_erase(t, dead)
    alive[dead] = False
    got = check_seeds(env, t, seeds, group, alive)
    assert not np.isin(got["slot"], [3, 70, 130, CH + 1, CH + 2]).any() and not np.isin(got["slot"], dead).any()
    for groups in ({2}, {0, 4}, {1, 2, 3}, set(), {9}):
        got = check_seeds(env, t, seeds, group, alive, groups)
        assert set(got["group"]) <= groups
    # capacity: the first records only, the count exact, nothing behind them
    want = check_seeds(env, t, seeds, group, alive)
    guard = np.frombuffer(bytes([0xCD]) * capi.SEED_EXPORT_DTYPE.itemsize, capi.SEED_EXPORT_DTYPE)[0]
    out = np.full(len(want) + 4, guard, capi.SEED_EXPORT_DTYPE)
    got, total, rc = ctx.seed_table_export(t, None, cap=5, out=out)
    assert rc == E_TRUNCATED and total == len(want) and out[:5].tobytes() == want[:5].tobytes()
    assert out[5:].tobytes() == np.full(len(want) - 1, guard, capi.SEED_EXPORT_DTYPE).tobytes()
    # compaction renumbers the slots; the export follows
    n_new, remap = ctx.seed_table_compact(t)
    keep = np.nonzero(alive)[0]
    assert n_new == len(keep) and list(remap[keep]) == list(range(len(keep)))
    packed = (capi.Seed * len(keep))(*[seeds[i] for i in keep])
    got = check_seeds(env, t, packed, group[keep], np.ones(len(keep), bool))
    assert len(got) == len(want) and np.array_equal(got["slot"], remap[want["slot"]])
    ctx.seed_table_destroy(t)
