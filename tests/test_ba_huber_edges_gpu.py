"""The Huber deltas of a local-BA window (src/bundle_adjustment.cpp:618-680: 1.4826 x the element nth_element leaves at floor(n / 2),
per edge kind) on PLANTED error magnitudes: the device radix select k_ba_mad_select (hso_amd/csrc/hso_ba.hip, four 8-bit digits with
a histogram in LDS, run by hso_gpu_ba_local_multi), the host arbitration of hso_gpu_ba_huber_deltas / _multi (nth_element on the
downloaded floats) and the oracle, against np.sort(keys)[len(keys) // 2].

How a magnitude is planted bit for bit: two identity poses, every edge host 0 -> target 1 at level 0 with fH = (0, 0, 1) and
idist = 1, so the projection is exactly (0, 0); a corner edge observes (v, 0) and an edgelet edge with normal (1, 0) observes (v, 0).
For a non-negative finite float32 v the magnitude is (float)sqrt(v * v) = v (v * v is exact in fp64, its root is v) or
(float)|1 * v + 0 * 0| = v.  No NaN and no infinity: nth_element on those is undefined in the reference too.

The key sets are what smooth random problems never produce: ties, zeros, counts of 1-4 and around the 1024-thread stride, keys
that differ in one digit only, a selected element with 0xFF in a digit (the digit scan stops at b < 255 and relies on the rest lying
in bin 255), all of a digit's mass in that bin, denormals, and the median at chosen edge indices.  Every assertion is an equality of
float32 bit patterns."""
import numpy as np
import pytest

from hso_amd import capi, synth
from test_ba import _obs_uv

EM2 = 480.0                                             # error_multiplier2 of the fallbacks (:664-680)
PT, LS = 0, 1


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def bits_of(pair):
    return tuple(int(b) for b in np.array(pair, np.float32).view(np.uint32))


def mix(keys_pt, keys_ls, how):
    """per-edge (kind, key) from the two kinds' keys, each kind in the given order: edge by edge ("interleave", the longer kind's
    tail last) or in two solid blocks ("blocks": corners first, "blocks_rev": edgelets first)"""
    keys_pt, keys_ls = np.asarray(keys_pt, np.float32), np.asarray(keys_ls, np.float32)
    if how == "interleave":
        n = min(len(keys_pt), len(keys_ls))
        kinds = np.concatenate([np.tile([PT, LS], n), np.full(len(keys_pt) - n, PT), np.full(len(keys_ls) - n, LS)])
        keys = np.empty(len(kinds), np.float32)
        keys[kinds == PT], keys[kinds == LS] = keys_pt, keys_ls
        return kinds.astype(np.int32), keys
    a, b = ((PT, keys_pt), (LS, keys_ls)) if how == "blocks" else ((LS, keys_ls), (PT, keys_pt))
    return np.concatenate([np.full(len(a[1]), a[0]), np.full(len(b[1]), b[0])]).astype(np.int32), np.concatenate([a[1], b[1]])


def place_median(kinds, keys, kind, at):
    """swap edges so that the (unique) median element of `kind` sits at edge index `at`"""
    mine = np.where(kinds == kind)[0]
    med = np.sort(keys[mine])[len(mine) // 2]
    src = mine[keys[mine] == med]
    assert len(src) == 1
    src, at = int(src[0]), at % len(keys)
    kinds, keys = kinds.copy(), keys.copy()
    kinds[[src, at]], keys[[src, at]] = kinds[[at, src]], keys[[at, src]]
    return kinds, keys


def window(kinds, keys):
    """(poses, fixed, idist, edges, uv) whose error magnitudes are `keys`, bit for bit (module docstring)"""
    keys = np.asarray(keys, np.float32)
    assert np.isfinite(keys).all() and not np.signbit(keys).any()
    n = len(keys)
    edges = np.zeros(n, capi.BA_EDGE_DTYPE)
    edges["point"] = np.arange(n)
    edges["host"], edges["target"], edges["level"] = 0, 1, 0
    edges["type"] = np.where(np.asarray(kinds) == LS, capi.FTR_EDGELET, capi.FTR_CORNER)
    edges["fH"] = [0.0, 0.0, 1.0]
    edges["normal"] = [1.0, 0.0]
    uv = np.zeros((n, 2)); uv[:, 0] = keys.astype(np.float64)
    edges["meas"] = uv
    return [capi.SE3.identity(), capi.SE3.identity()], np.ones(2, np.uint8), np.ones(n), edges, uv


def plain_deltas(kinds, keys):
    """the plain reference: per kind 1.4826 x the sorted keys' element at floor(n / 2), rounded to float; the fallbacks of :664-680"""
    med = lambda k: np.float32(1.4826 * float(np.sort(k)[len(k) // 2]))
    kp, kl = keys[kinds == PT], keys[kinds == LS]
    assert len(kp) or len(kl)
    with np.errstate(over="ignore"):                    # 1.4826 x FLT_MAX rounds to +inf as a float, in C as here
        return (med(kp) if len(kp) else np.float32(1.0 / EM2), med(kl) if len(kl) else np.float32(0.5 / EM2))


def distinct(rng, n, lo=1e-4, hi=3.0):
    """n distinct float32 keys in random order"""
    k = np.unique(rng.uniform(lo, hi, 2 * n + 8).astype(np.float32))
    assert len(k) >= n
    return rng.permutation(k)[:n]


def around(rng, sel, n_below, n_above, span_bits):
    """keys below and above the pattern `sel` that share its bits above `span_bits`, + sel itself: the element at rank n_below"""
    lo = sel & ~((1 << span_bits) - 1)
    below = rng.integers(lo, sel, n_below) if sel > lo else np.full(n_below, sel)
    above = rng.integers(sel + 1, sel + (1 << span_bits), n_above)
    return rng.permutation(f32(np.concatenate([below, [sel], above]).astype(np.uint32)))


# ------------------------------------------------------------------------------------------------------------ the key sets
def count_sets():
    """per-kind counts 1, 2, 3, 4 (rank floor(n / 2) of a handful) and both sides of one and two strides of the 1024-thread sweep
    (hso_ba.hip:1292, :1304), even and odd; each kind meets each count once, mixed both ways; then one kind empty (:1297, :1325-1326)"""
    rng = np.random.default_rng(1)
    counts = (1, 2, 3, 4, 1023, 1024, 1025, 2047, 2048, 2049)
    out = []
    for i, n in enumerate(counts):
        other = counts[(i + 3) % len(counts)]
        out.append(("counts %d corners, %d edgelets" % (n, other), *mix(distinct(rng, n), distinct(rng, other), ("interleave", "blocks", "blocks_rev")[i % 3])))
    for n in (1, 2, 1025):
        out.append(("%d corners, no edgelet" % n, *mix(distinct(rng, n), [], "blocks")))
        out.append(("no corner, %d edgelets" % n, *mix([], distinct(rng, n), "blocks")))
    return out


def tie_sets():
    rng = np.random.default_rng(2)
    out = []
    same = lambda v, n: np.full(n, v, np.float32)
    # all keys equal: every digit's histogram has all its mass in one bin, the rank stays floor(n / 2) down to the last digit
    out.append(("all equal", *mix(same(0.37, 1025), same(1e-3, 2048), "interleave")))
    # +0.0 everywhere: bin 0 of every digit; the delta is 0
    out.append(("all zero", *mix(same(0.0, 1024), same(0.0, 3), "blocks")))
    # zeros up to the rank and one key above: h zeros + 1 (count h + 1, rank floor((h + 1) / 2)): the non-zero key only for h = 1
    out.append(("one zero + one key | two zeros + one key", *mix([0.0, 0.5], [0.0, 0.25, 0.0], "interleave")))
    out.append(("1024 zeros + one key | 1023 zeros + one key", *mix(np.append(same(0.0, 1024), np.float32(0.5)), np.append(np.float32(0.7), same(0.0, 1023)), "blocks_rev")))
    # half zeros, half distinct keys: even count 2h -> the smallest non-zero key, odd count 2h - 1 -> the last zero
    out.append(("half zeros, even | odd", *mix(rng.permutation(np.append(same(0.0, 600), distinct(rng, 600))),
                                               rng.permutation(np.append(same(0.0, 600), distinct(rng, 599))), "interleave")))
    # two distinct values: the rank on the last copy of the lower one, on the first copy of the upper one; n even and odd
    for n in (1024, 1025):
        h = n // 2
        out.append(("two values, n = %d: last lower | first upper" % n,
                    *mix(rng.permutation(np.append(same(0.25, h + 1), same(0.75, n - h - 1))), rng.permutation(np.append(same(0.25, h), same(0.75, n - h))), "interleave")))
    return out


def digit_sets():
    """keys that differ in ONE digit of the select (hso_ba.hip:1300-1317), 256 of them so that every bin of that digit's histogram
    holds one key (byte 3 of a finite positive float stops at 0x7F: 128 values, twice)"""
    rng = np.random.default_rng(3)
    base = 0x3F000000
    i = np.arange(256, dtype=np.uint32)
    b0, b1, b2 = f32(base + i), f32(base + (i << 8)), f32(base + (i << 16))
    b3 = f32(((np.arange(256, dtype=np.uint32) >> 1) << 24) | 0x00123456)
    return [("byte 0 | byte 1", *mix(rng.permutation(b0), rng.permutation(b1), "interleave")),
            ("byte 2 | byte 3", *mix(rng.permutation(b2), rng.permutation(b3), "blocks"))]


def bin255_sets():
    """the selected element has 0xFF in a digit: the scan `for (; b < 255u; b++)` (hso_ba.hip:1312) must fall through to bin 255 with
    the rank inside it"""
    rng = np.random.default_rng(4)
    out = []
    # 0xFF in byte 0, in byte 1, in byte 2 of the selected key; the other keys spread over all bins of that digit and the lower ones
    s0 = around(rng, 0x3E7FFFFF, 300, 300, 8)
    s1 = around(rng, 0x3E00FF37, 301, 300, 16)
    s2 = around(rng, 0x3EFF1234, 300, 299, 24)
    s012 = around(rng, 0x3EFFFFFF, 257, 256, 24)
    out.append(("0xFF in byte 0 | in byte 1", *mix(s0, s1, "interleave")))
    out.append(("0xFF in byte 2 | in bytes 0-2", *mix(s2, s012, "blocks_rev")))
    for s, sel in ((s0, 0x3E7FFFFF), (s1, 0x3E00FF37), (s2, 0x3EFF1234), (s012, 0x3EFFFFFF)):
        assert np.sort(s)[len(s) // 2] == f32(sel)
    # byte 3: the largest finite bin is 0x7F — FLT_MAX (7F 7F FF FF) selected among small keys
    out.append(("FLT_MAX selected", *mix(f32([0x3F000000, 0x7F7FFFFF, 0x00000001, 0x7F7FFFFF, 0x7F7FFFFF]), f32([0x7F7FFFFF, 0x7F7FFFFF]), "interleave")))
    # ALL the mass a digit's histogram sees lies in bin 255 (c keys that share the digits above and have 0xFF there), with the rank
    # 0 and c - 1 inside it: lower keys below, upper keys above, counts chosen so that floor(n / 2) is the group's first / last key
    lower = lambda n: f32(0x3D000000 + rng.integers(0, 1 << 24, n).astype(np.uint32))
    upper = lambda n: f32(0x3F000000 + rng.integers(0, 1 << 24, n).astype(np.uint32))
    c = 40
    groups = (f32(np.full(c, 0x3E1234FF, np.uint32)),                                  # byte 0: c copies
              f32(0x3E12FF00 + rng.permutation(256)[:c].astype(np.uint32)),            # byte 1: distinct low bytes
              f32(0x3EFF0000 + rng.permutation(1 << 16)[:c].astype(np.uint32)))        # byte 2: distinct low halves
    sets = []
    for g in groups:
        first = rng.permutation(np.concatenate([lower(100), g, upper(60)]))            # n = 200, rank 100 = the group's smallest
        last = rng.permutation(np.concatenate([lower(100), g, upper(138)]))            # n = 278, rank 139 = the group's largest
        assert np.sort(first)[100] == g.min() and np.sort(last)[139] == g.max()
        sets += [first, last]
    out.append(("all mass in bin 255 of byte 0, rank 0 | rank c - 1", *mix(sets[0], sets[1], "interleave")))
    out.append(("all mass in bin 255 of byte 1, rank 0 | rank c - 1", *mix(sets[2], sets[3], "blocks")))
    out.append(("all mass in bin 255 of byte 2, rank 0 | rank c - 1", *mix(sets[4], sets[5], "interleave")))
    # one and two keys: the only mass of every digit is the selected key's own bin (rank 0, and rank n - 1 = 1)
    out.append(("0x3EFFFFFF alone | twice", *mix(f32([0x3EFFFFFF]), f32([0x3EFFFFFF, 0x3EFFFFFF]), "blocks")))
    return out


def denormal_sets():
    rng = np.random.default_rng(5)
    den = lambda n: f32(rng.integers(1, 0x00800000, n).astype(np.uint32))
    a = rng.permutation(np.concatenate([den(600), distinct(rng, 425)]))                 # the median is a denormal
    b = rng.permutation(np.concatenate([den(400), distinct(rng, 624)]))                 # the median is a normal number above 400 denormals
    c = rng.permutation(np.concatenate([den(7), f32([0x00800000, 0x007FFFFF, 0x00000001])]))
    assert np.sort(a)[len(a) // 2] < np.finfo(np.float32).tiny <= np.sort(b)[len(b) // 2]
    return [("denormal median | normal median", *mix(a, b, "interleave")), ("ten keys around the smallest normal | denormal median", *mix(c, a[:333], "blocks"))]


def order_sets():
    """where the keys lie relative to the sweep `for (k = tid; k < n; k += 1024)`: sorted both ways, and the median element of the
    corners at edge index 0, 1023, 1024 and n - 1"""
    rng = np.random.default_rng(6)
    kp, kl = distinct(rng, 1500), distinct(rng, 1001)
    out = [("ascending", *mix(np.sort(kp), np.sort(kl), "interleave")), ("descending", *mix(np.sort(kp)[::-1], np.sort(kl)[::-1], "interleave")),
           ("ascending corners, descending edgelets, blocks", *mix(np.sort(kp), np.sort(kl)[::-1], "blocks"))]
    kinds, keys = mix(kp, kl, "interleave")
    for at in (0, 1023, 1024, -1):
        out.append(("corner median at edge %d" % at, *place_median(kinds, keys, PT, at)))
    kinds, keys = mix(kp, kl, "blocks_rev")
    for at in (1023, 1024):
        out.append(("edgelet median at edge %d" % at, *place_median(kinds, keys, LS, at)))
    return out


GROUPS = dict(counts=count_sets, ties=tie_sets, digits=digit_sets, bin255=bin255_sets, denormals=denormal_sets, order=order_sets)


def test_planted_sets_are_what_they_say():
    """the key sets on the CPU: finite, non-negative, the names unique, both mixes present, and the properties the names claim"""
    names = [name for g in GROUPS.values() for name, _, _ in g()]
    assert len(names) == len(set(names))
    for g in GROUPS.values():
        for name, kinds, keys in g():
            assert keys.dtype == np.float32 and len(kinds) == len(keys) > 0 and np.isfinite(keys).all() and not np.signbit(keys).any(), name
    per_kind = sorted({int((kinds == k).sum()) for _, kinds, _ in count_sets() for k in (PT, LS)})
    assert per_kind == [0, 1, 2, 3, 4, 1023, 1024, 1025, 2047, 2048, 2049]
    for name, kinds, keys in digit_sets():
        for k, byte in zip((PT, LS), (0, 1) if name.startswith("byte 0") else (2, 3)):
            u = keys[kinds == k].view(np.uint32)
            assert len(u) >= 256 and len(np.unique((u >> (8 * byte)) & 255)) == (256 if byte < 3 else 128), name
            assert len(np.unique(u & ~np.uint32(255 << (8 * byte)))) == 1, name                   # nothing else differs
    for name, kinds, keys in bin255_sets()[:2]:
        for k in (PT, LS):
            sel = int(np.sort(keys[kinds == k])[(kinds == k).sum() // 2].view(np.uint32))
            assert 0xFF in ((sel >> 0) & 255, (sel >> 8) & 255, (sel >> 16) & 255), name
    assert bits_of(plain_deltas(*tie_sets()[1][1:])) == (0, 0)                                    # all zero: both deltas +0.0
    hc, he = plain_deltas(*bin255_sets()[2][1:])
    assert hc == he == np.float32(np.inf)                                                         # 1.4826 x FLT_MAX as a float


def test_planted_magnitudes_come_back_bit_for_bit(orc):
    """the planting itself, on the oracle: with one edge per kind the delta is 1.4826 x that very key — for zero, the smallest
    denormal, the largest denormal, ordinary keys, FLT_MAX"""
    for bits in (0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3E7FFFFF, 0x3F000001, 0x7F7FFFFF):
        kinds, keys = mix(f32([bits]), f32([bits ^ 1 if bits else 0]), "blocks")
        poses, fixed, idist, edges, uv = window(kinds, keys)
        assert bits_of(orc.ba_huber_deltas(poses, idist, edges, uv, EM2)) == bits_of(plain_deltas(kinds, keys)), hex(bits)


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_huber_deltas_on_planted_magnitudes(gpu_ctx, orc, group):
    """all windows of a group in ONE hso_gpu_ba_local_multi call (one workgroup of k_ba_mad_select per window) with n_iter = 0 and
    every pose fixed; the same windows through the host median's two entry points and the oracle"""
    sets = GROUPS[group]()
    wins = [window(kinds, keys) for _, kinds, keys in sets]
    want = [bits_of(plain_deltas(kinds, keys)) for _, kinds, keys in sets]
    got, hub = gpu_ctx.ba_local_multi([(p, fx, idist, e, uv, 0) for p, fx, idist, e, uv in wins], EM2)
    multi = gpu_ctx.ba_huber_deltas_multi([(p, idist, e, uv) for p, _, idist, e, uv in wins], EM2)
    for (name, _, _), (p, _, idist, e, uv), w, (_, _, _, res), h, m in zip(sets, wins, want, got, hub, multi):
        assert bits_of(h) == w, ("ba_local_multi", name)
        assert bits_of(m) == w, ("ba_huber_deltas_multi", name)
        assert bits_of(gpu_ctx.ba_huber_deltas(p, idist, e, uv, EM2)) == w, ("ba_huber_deltas", name)
        assert bits_of(orc.ba_huber_deltas(p, idist, e, uv, EM2)) == w, ("oracle", name)
        assert (res.iterations, res.n_solves, res.n_accepted) == (0, 0, 0), name                  # n_iter = 0: no solve


@pytest.mark.gpu
def test_huber_deltas_with_ties_on_ordinary_geometry(gpu_ctx, orc):
    """the error kernel on general poses, inverse depths, levels and normals (the planted geometry exercises none of them), with
    observations on a 1/64 grid; the four sources against each other and against a numpy statement of the magnitudes in fp64
    rounded to float (tests/test_ba.py::test_oracle_ba_huber_deltas)"""
    poses, fixed, idist, edges = synth.ba_problem(4, 60, 3, seed=52)
    uv = np.round(_obs_uv(edges, np.random.default_rng(52)) * 64.0) / 64.0
    e_pt, e_ls = [], []
    for k, e in enumerate(edges):
        Tth = orc.se3_mul(poses[e["target"]], orc.se3_inverse(poses[e["host"]]))
        pT = orc.se3_apply(Tth, e["fH"] / idist[e["point"]])
        d = (uv[k] - pT[:2] / pT[2]) / (1 << e["level"])
        if e["type"] == capi.FTR_EDGELET:
            e_ls.append(np.float32(abs(e["normal"][0] * d[0] + e["normal"][1] * d[1])))
        else:
            e_pt.append(np.float32(np.sqrt(d[0] * d[0] + d[1] * d[1])))
    assert len(e_pt) > 3 and len(e_ls) > 3
    up = lambda v: np.float32(1.4826 * float(np.sort(np.array(v, np.float32))[len(v) // 2]))
    want = bits_of((up(e_pt), up(e_ls)))
    got, hub = gpu_ctx.ba_local_multi([(poses, fixed, idist, edges, uv, 0)], EM2)
    assert bits_of(hub[0]) == want
    assert bits_of(gpu_ctx.ba_huber_deltas(poses, idist, edges, uv, EM2)) == want
    assert bits_of(gpu_ctx.ba_huber_deltas_multi([(poses, idist, edges, uv)], EM2)[0]) == want
    assert bits_of(orc.ba_huber_deltas(poses, idist, edges, uv, EM2)) == want
    assert (got[0][3].iterations, got[0][3].n_solves, got[0][3].n_accepted) == (0, 0, 0)
