"""pose_ref.py (exact numpy prediction of an `n_iter = 0` pose call on identity poses and dyadic residuals) against the CPU
restatement and against numbers worked out by hand.  The GPU half is in test_pose.py."""
import numpy as np
import pytest

import pose_ref
from hso_amd import capi


def identity_job(feats, reproj_thresh=2.0):
    I = capi.SE3.identity()
    return capi.make_pose_job(feats.astype(capi.POSE_FEAT_DTYPE), [I] * pose_ref.N_HOSTS, I, reproj_thresh=reproj_thresh, n_iter=0)


def assert_equals_prediction(res, mask, pred):
    """The six predicted fields, no tolerance."""
    assert res.error_init == pred.error_init
    assert res.error_final == pred.error_final
    assert res.estimated_scale == pred.estimated_scale
    assert np.array_equal(mask, pred.mask)
    assert (res.n_deleted, res.num_obs) == (pred.n_deleted, pred.num_obs)


def test_layout_and_cases():
    assert pose_ref.POSE_FEAT_DTYPE == capi.POSE_FEAT_DTYPE
    assert (pose_ref.FTR_CORNER, pose_ref.FTR_EDGELET) == (capi.FTR_CORNER, capi.FTR_EDGELET)
    assert len(pose_ref.CASES) == 72 and len(set(pose_ref.CASES)) == 72


@pytest.mark.parametrize("regime", pose_ref.REGIMES)
def test_inputs_are_what_the_cases_claim(regime):
    for n, kind, r in pose_ref.CASES:
        if r != regime:
            continue
        feats = pose_ref.make_feats(n, kind, regime)
        assert len(feats) == n and feats["has_point"].any()
        edge = feats["type"][feats["has_point"] != 0] == pose_ref.FTR_EDGELET
        assert {"edgelets": edge.all(), "corners": not edge.any(), "mixed": True}[kind]
        # residuals are whole multiples of 2^-22 (2^-20 over at most 2^2), i.e. exact
        d = (feats["f"] - feats["host_f"])[:, :2] * 2.0 ** 22
        assert np.array_equal(d, np.round(d))
        sq, mag = pose_ref.float_keys(feats)
        if regime == "ties" and n >= 100 and kind == "edgelets":
            assert len(np.unique(mag)) <= 27                               # 9 magnitudes x 3 levels
            k = np.sort(sq)[len(sq) // 2]
            assert (sq == k).sum() > 1                                  # the selected rank sits inside a run: no select can stop early
    if regime == "spread":
        n_pts = [int(pose_ref.make_feats(n, "mixed", regime)["has_point"].sum()) for n in (79, 80)]
        assert max(n_pts) < 80                                          # 80 table entries, fewer points: the rule is on the table


def test_prediction_equals_the_restatement_on_all_jobs(orc, cam):
    for n, kind, regime in pose_ref.CASES:
        feats = pose_ref.make_feats(n, kind, regime)
        res, mask = orc.pose_optimize(cam, identity_job(feats))
        pred = pose_ref.predict(feats, cam.fx, cam.fy)
        assert_equals_prediction(res, mask, pred)
        assert (res.status, res.iters, res.n_trials_total) == (0, 0, 0), (n, kind, regime)
    # non-trivial on the way: culling happened somewhere in the spread regime, nowhere in the tie regime
    assert any(pose_ref.predict(pose_ref.make_feats(n, k, "spread"), cam.fx, cam.fy).n_deleted > 0 for n, k, _ in pose_ref.CASES)
    assert all(pose_ref.predict(pose_ref.make_feats(n, k, "ties"), cam.fx, cam.fy).n_deleted == 0 for n, k, _ in pose_ref.CASES)


def test_shared_prefix_family(orc, cam):
    feats = pose_ref.make_prefix_feats()
    for keys in pose_ref.float_keys(feats):
        bits = keys.view(np.uint32)
        assert len(np.unique(bits)) == pose_ref.PREFIX_N and len(np.unique(bits >> 16)) == 1
    thr = pose_ref.prefix_reproj_thresh(cam.fx, cam.fy)
    res, mask = orc.pose_optimize(cam, identity_job(feats, thr))
    pred = pose_ref.predict(feats, cam.fx, cam.fy, thr)
    assert_equals_prediction(res, mask, pred)
    assert 250 < pred.n_deleted < 350


def test_hand_computed_job(orc):
    """Five features, em2 = 512, level-scaled residuals in units of 2^-10:
         0 corner  (3, 4)        |e| = 5    > sqrt(5.991) / 512 = 4.7808e-3 = 4.90 units  -> culled
         1 corner  (1, 0)        |e| = 1
         2 edgelet grad (1, 0), (2, 128)   e = 2    < 1.3 / 512 = 2.5391e-3 = 2.60 units
         3 edgelet grad (0, 1), (0, -3)    |e| = 3  > 2.60 units                         -> culled
         4 corner  level 1, (4, 0)         |e| = 2
       squared keys, sorted: 1 4 4 9 25 (x 2^-20): rank 5 / 2 = 2 is 4 * 2^-20, sqrt = 2^-9, x 512 = 1 (initially and finally: nothing moved);
       corner magnitudes, sorted: 1 2 5: rank 3 / 2 = 1 is 2^-9; scale = 1.4826f * 2^-9, x 512 = 1.4826f as a double."""
    cam = capi.make_camera(capi.CAM_PINHOLE, 640, 480, 512.0, 512.0, 319.5, 239.5)
    u = 2.0 ** -10
    rows = [  # type, level, grad, (dx, dy)
        (pose_ref.FTR_CORNER, 0, (1, 0), (3 * u, 4 * u)),
        (pose_ref.FTR_CORNER, 0, (0, 1), (1 * u, 0)),
        (pose_ref.FTR_EDGELET, 0, (1, 0), (2 * u, 128 * u)),
        (pose_ref.FTR_EDGELET, 0, (0, 1), (0, -3 * u)),
        (pose_ref.FTR_CORNER, 1, (1, 0), (4 * u, 0)),
    ]
    feats = np.zeros(5, pose_ref.POSE_FEAT_DTYPE)
    for i, (ty, lvl, g, (dx, dy)) in enumerate(rows):
        x, y = 0.25 - i / 16, -0.125 + i / 32
        feats[i] = (1, ty, lvl, 0, i % pose_ref.N_HOSTS, 0, (x + dx, y + dy, 1), g, (x, y, 1), 1.0)
    expected = pose_ref.PosePrediction(error_init=1.0, error_final=1.0, estimated_scale=1.4825999736785889,
                                       mask=np.array([1, 0, 0, 1, 0], np.uint8), n_deleted=2, num_obs=3)
    pred = pose_ref.predict(feats, 512.0, 512.0)
    res, mask = orc.pose_optimize(cam, identity_job(feats))
    assert_equals_prediction(res, mask, expected)
    assert_equals_prediction(res, mask, pred)
    assert res.error_in_px == 1.0 and (res.status, res.iters) == (0, 0)
