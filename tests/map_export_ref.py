"""TEST INFRASTRUCTURE for tests/test_map_export_gpu.py: the map export (include/hso_gpu.h: hso_gpu_seqmap_export_points,
hso_gpu_seed_table_export) restated in numpy — the selection rule, the walk along a point's observation chain, the colour lookup and
the seed's position — plus small builders of the tables the tests hand to the device."""
import numpy as np

from hso_amd import capi

NO_COLOR = 128          # Point::color_'s initial value (include/hso/point.h:121)
PT_BAD = 1 << 18        # HSO_PT_BAD
CHUNK = 256             # EXPORT_CHUNK of hso_amd/csrc/hso_export.hip: rows per workgroup of the count and emit passes
W = H = 64              # the smallest frame the upload accepts


def image(k):
    """a frame in which every pixel's value depends on its position (and on k), so that a wrong pixel or a wrong frame shows"""
    y, x = np.mgrid[0:H, 0:W]
    return ((x * 3 + y * 7 + k * 11 + (x * y) % 5) & 0xff).astype(np.uint8)


def pixel(img, px):
    """level-0 byte ((int)px[1], (int)px[0]); the default for a frame that is not resident or a pixel outside it"""
    if img is None or not (0.0 <= px[0] < img.shape[1] and 0.0 <= px[1] < img.shape[0]):
        return NO_COLOR
    return int(img[int(px[1]), int(px[0])])


def selected(points, type_mask, min_obs):
    word = np.ascontiguousarray(points["pad_"]).view(np.uint32)
    typ = (word >> 4) & 0xf
    return (typ != 0) & (((np.uint64(type_mask) >> typ.astype(np.uint64)) & np.uint64(1)) == 1) & ((word & PT_BAD) == 0) & (points["obs_count"] >= min_obs)


def point_color(p, obs, kfs, images):
    """images[k]: level 0 of keyframe row k's frame, None when it is not resident"""
    o, hk = int(p["obs_begin"]), int(p["host_kf"])
    for _ in range(int(p["obs_count"])):
        if o < 0 or o >= len(obs):
            break
        if int(obs["kf"][o]) == hk:
            if 0 <= hk < len(kfs):
                return pixel(images[hk], obs["px"][o])
            break
        o = int(obs["pad_"][o])
    return NO_COLOR


def export_points(maps, type_mask, min_obs):
    """maps: dicts(points MAP_POINT_DTYPE, obs OBS_DTYPE, kfs KF_DTYPE, images) in call order -> (records, begin)"""
    out, begin = [], [0]
    for M in maps:
        pts = M["points"]
        rows = np.nonzero(selected(pts, type_mask, min_obs))[0] if len(pts) else []
        rec = np.zeros(len(rows), capi.POINT_EXPORT_DTYPE)
        for i, r in enumerate(rows):
            p = pts[r]
            word = int(np.uint32(np.int64(p["pad_"]) & 0xffffffff))
            hk = int(p["host_kf"])
            rec[i] = (p["pos"], r, int(M["kfs"]["keyframe_id"][hk]) if 0 <= hk < len(M["kfs"]) else -1, p["obs_count"],
                      point_color(p, M["obs"], M["kfs"], M["images"]), (word >> 4) & 0xf, word & 0xf, 0)
        out.append(rec)
        begin.append(begin[-1] + len(rec))
    return (np.concatenate(out) if out else np.zeros(0, capi.POINT_EXPORT_DTYPE)), np.array(begin, np.int32)


def quat_matrix(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def export_seeds(seeds, group, alive, images, groups=None):
    """seeds: list of capi.Seed in slot order; group / alive per slot; images: frame id -> level 0.
    -> (records, distance per record: |f * (1 / mu)|, what the position's tolerance is relative to)"""
    rec, dist = [], []
    for slot, s in enumerate(seeds):
        mu = np.float32(s.mu)
        if not alive[slot] or (groups is not None and int(group[slot]) not in groups) or not (np.isfinite(mu) and mu > 0):
            continue
        v = np.array(s.f[:]) * (1.0 / np.float64(mu))
        q, t = s.T_ref_w.to_arrays()
        pos = quat_matrix(q).T @ (v - t)                             # T_ref_w^-1 * v
        r = np.zeros(1, capi.SEED_EXPORT_DTYPE)[0]
        r["pos"], r["mu"], r["sigma2"], r["slot"], r["group"] = pos, mu, np.float32(s.sigma2), slot, int(group[slot])
        r["color"], r["type"], r["level"] = pixel(images.get(int(s.ref_frame_id)), s.px[:]), s.type, s.level
        rec.append(r); dist.append(np.linalg.norm(v))
    return (np.array(rec, capi.SEED_EXPORT_DTYPE) if rec else np.zeros(0, capi.SEED_EXPORT_DTYPE)), np.array(dist)
