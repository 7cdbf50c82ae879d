"""Exact prediction of the pose optimiser's outputs at a fixed pose (an `n_iter = 0` call) in plain numpy.

Nothing here imports the CPU restatement (oracle/) or the library.  The jobs are built so that every residual is an exact
dyadic number and no rounding is left to the order of operations:

  * T_f_w and every host pose are the identity: rotating by q = (0, 0, 0, 1) and adding t = 0 returns the argument, so
    pTarget == host_f / idist, and with idist = 1, host_f = (x, y, 1), f = (x + dx, y + dy, 1) the residual is (dx, dy) / 2^level
    exactly (x, y multiples of 2^-12 in [-0.5, 0.5), dx, dy multiples of 2^-20 or, in the shared-prefix family, of 2^-29: the sums
    x + dx fit a double's mantissa many times over);
  * grad is (1, 0) or (0, 1), so an edgelet's residual is dx or dy scaled, again exact, and exact as a float (<= 21 bits);
  * e0^2 and e1^2 are exact in double (<= 42 bits), so e0 * e0 + e1 * e1 is one rounding whether or not it is contracted
    into a fused multiply-add; the square root and every float product are single correctly rounded IEEE operations.

What remains is the selection logic itself — src/pose_optimizer.cpp:426-483 (initial errors, MAD scales) and :691-767
(thresholds, culling, final median) — restated here with elementwise float32 / float64 operations and np.sort(...)[k]."""
from collections import namedtuple

import numpy as np

# hso_pose_feat (include/hso_gpu.h), the layout the test asserts equal to the binding's
POSE_FEAT_DTYPE = np.dtype([("has_point", "<i4"), ("type", "<i4"), ("level", "<i4"), ("temporary", "<i4"),
                            ("host_pose", "<i4"), ("_pad", "<i4"), ("f", "<f8", 3), ("grad", "<f8", 2),
                            ("host_f", "<f8", 3), ("idist", "<f8")])
FTR_CORNER, FTR_EDGELET = 0, 1
N_HOSTS = 3                                                        # identity host poses a job's features point at

SIZES = (1, 2, 7, 64, 79, 80, 100, 512, 513, 1025, 2049, 4096)      # 79 / 80: the chi-square threshold; 512 / 513, 1025, 2049, 4096: the
KINDS = ("mixed", "edgelets", "corners")                           # kernel's features-per-thread slots and its cap
REGIMES = ("spread", "ties")
CASES = [(n, kind, regime) for n in SIZES for kind in KINDS for regime in REGIMES]

PosePrediction = namedtuple("PosePrediction", "error_init error_final estimated_scale mask n_deleted num_obs")


def error_multiplier2(fx, fy):
    """src/camera.cpp:59"""
    return abs(fx) if fx * fy < 0 else abs((fx + fy) * 0.5)


def _table(rng, n, kind, x, y, dx, dy, level, has_point):
    feats = np.zeros(n, POSE_FEAT_DTYPE)
    feats["has_point"] = has_point
    feats["type"] = {"mixed": np.where(rng.uniform(size=n) < 0.4, FTR_EDGELET, FTR_CORNER), "edgelets": FTR_EDGELET, "corners": FTR_CORNER}[kind]
    feats["level"] = level
    feats["temporary"] = rng.uniform(size=n) < 0.1
    feats["host_pose"] = rng.integers(0, N_HOSTS, n)
    feats["f"] = np.stack([x + dx, y + dy, np.ones(n)], axis=1)
    horizontal = rng.uniform(size=n) < 0.5
    feats["grad"] = np.stack([np.where(horizontal, 1.0, 0.0), np.where(horizontal, 0.0, 1.0)], axis=1)
    feats["host_f"] = np.stack([x, y, np.ones(n)], axis=1)
    feats["idist"] = 1.0
    return feats


def make_feats(n, kind, regime):
    """The feature table of one of CASES (the poses are identities: the caller supplies them)."""
    rng = np.random.default_rng(100000 * KINDS.index(kind) + 10000 * REGIMES.index(regime) + n)
    x = rng.integers(-2048, 2048, n) * 2.0 ** -12
    y = rng.integers(-2048, 2048, n) * 2.0 ** -12
    if regime == "spread":
        steps = rng.integers(-2 ** 14, 2 ** 14 + 1, (n, 2))
        steps[rng.uniform(size=n) < 0.1] *= 64                      # residuals past the culling thresholds
    else:
        steps = rng.integers(-8, 9, (n, 2))                         # ~20 distinct magnitudes per 100 features: equal keys at the rank
    has_point = rng.uniform(size=n) >= 0.15
    if not has_point.any():
        has_point[int(rng.integers(0, n))] = True
    return _table(rng, n, kind, x, y, steps[:, 0] * 2.0 ** -20, steps[:, 1] * 2.0 ** -20, rng.integers(0, 3, n), has_point)


PREFIX_N = 600


def make_prefix_feats():
    """600 corners at level 0 whose magnitudes 2^-6 + j * 2^-29 (j a permutation of 0..599) are distinct floats that share
    their high bytes: every radix pass has to narrow by one byte under a non-trivial prefix."""
    rng = np.random.default_rng(29)
    n = PREFIX_N
    x = rng.integers(-2048, 2048, n) * 2.0 ** -12
    y = rng.integers(-2048, 2048, n) * 2.0 ** -12
    dx = 2.0 ** -6 + rng.permutation(n) * 2.0 ** -29
    return _table(rng, n, "corners", x, y, dx, np.zeros(n), np.zeros(n, np.int64), np.ones(n, bool))


def prefix_reproj_thresh(fx, fy):
    """A culling threshold inside the family's range (about rank 300), so that its mask is not all ones."""
    return (2.0 ** -6 + 300 * 2.0 ** -29) * error_multiplier2(fx, fy)


def float_keys(feats):
    """(squared-error keys, magnitude keys) of the features with a point, as float32 — the two sets the 32-bit selects order."""
    F = feats[feats["has_point"] != 0]
    e0, e1, edge = _residuals(F)
    mag = np.where(edge, np.abs((F["grad"][:, 0] * e0 + F["grad"][:, 1] * e1).astype(np.float32)), np.sqrt(e0 * e0 + e1 * e1).astype(np.float32))
    return mag * mag, mag


def _residuals(F):
    # pTarget = host_f / idist at identity poses; e = (project2d(f) - project2d(pTarget)) / 2^level (:429-440)
    inv = 1.0 / F["idist"]
    X = F["host_f"] * inv[:, None]
    sc = 1.0 / (1 << F["level"]).astype(np.float64)
    e0 = (F["f"][:, 0] / F["f"][:, 2] - X[:, 0] / X[:, 2]) * sc
    e1 = (F["f"][:, 1] / F["f"][:, 2] - X[:, 1] / X[:, 2]) * sc
    return e0, e1, F["type"] == FTR_EDGELET


def predict(feats, fx, fy, reproj_thresh=2.0):
    """What optimizeLevenbergMarquardt3rd returns for `feats` with identity poses and no iteration.  feats needs at least one
    feature with a point."""
    f32, f64 = np.float32, np.float64
    em2 = f64(error_multiplier2(fx, fy))
    n = len(feats)
    has = feats["has_point"] != 0
    F = feats[has]
    e0, e1, edge = _residuals(F)
    n_init, n_pt, n_ls = len(F), int((~edge).sum()), int(edge.sum())
    assert n_init > 0
    err_ls = F["grad"][:, 0] * e0 + F["grad"][:, 1] * e1            # double; `float error_ls` at :442, double at :723
    err_pt = np.sqrt(e0 * e0 + e1 * e1)                             # double; `float error_pt` at :448 and :733
    ls_f, pt_f = err_ls.astype(f32), err_pt.astype(f32)
    # chi2_vec_init: float products pushed into a vector<double> (:442-450); getMedian = the rank n / 2 element (:758-761)
    init_keys = np.where(edge, ls_f * ls_f, pt_f * pt_f)
    assert init_keys.dtype == f32
    error_init = np.sqrt(f64(np.sort(init_keys)[n_init // 2])) * em2
    # MAD scales (robust_cost.cpp:67-74): 1.4826f * the rank n / 2 magnitude; the absent kind's scale is derived (:467-476)
    scale_pt = f32(1.4826) * np.sort(pt_f[~edge])[n_pt // 2] if n_pt else f32(0)
    scale_ls = f32(1.4826) * np.sort(np.abs(ls_f[edge]))[n_ls // 2] if n_ls else f32(0)
    if n_pt and not n_ls:
        scale_ls = f32(0.5 * f64(scale_pt))
    if n_ls and not n_pt:
        scale_pt = f32(2) * scale_ls
    assert scale_pt.dtype == f32 and scale_ls.dtype == f32
    estimated_scale = f64(scale_pt) * em2
    # thresholds (:696-699): floats; the chi-square one below 80 table entries (not 80 points)
    thr_pt = f32(np.sqrt(f64(5.991)) / em2) if n < 80 else f32(f64(reproj_thresh) / em2)
    thr_ls = f32(f64(1.3) / em2)
    out = np.where(edge, np.abs(err_ls) > f64(thr_ls), pt_f > thr_pt)
    mask = np.zeros(n, np.uint8)
    mask[np.flatnonzero(has)[out]] = 1
    n_deleted = int(out.sum())
    # chi2_vec_final (:723-742): edgelets squared in double, corners as float products
    final_keys = np.where(edge, err_ls * err_ls, (pt_f * pt_f).astype(f64))
    error_final = np.sqrt(np.sort(final_keys)[n_init // 2]) * em2
    return PosePrediction(float(error_init), float(error_final), float(estimated_scale), mask, n_deleted, n_init - n_deleted)
