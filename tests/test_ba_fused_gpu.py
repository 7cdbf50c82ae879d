"""hso_gpu_options.ba_fused / hso_vo_options.ba_fused: a window's Levenberg rounds in ONE launch (k_ba_rounds: one workgroup per
window walks the virtual blocks the per-round kernels run as workgroups) against the per-round kernels, in the same binary.

Every output of a round is owned by one thread or one 256-thread workgroup and every sum is a fixed tree inside it, so the fused
shape has to return the SAME BITS: poses, inverse depths, per-edge chi2, result records, the written-back map of the resident
call and the engine's trajectories.  hso_gpu_ba_debug_launches tells which shape ran."""
import ctypes as C

import numpy as np
import pytest

from hso_amd import capi, synth, vo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fused_ctx():
    ctx = capi.Context(0)
    ctx.configure(ba_fused=True)
    yield ctx
    ctx.close()


def _perturbed(orc, shape, seed, noise=0.3, dp=4e-3, di=0.0, **kw):
    poses, fixed, idist, edges = synth.ba_problem(*shape, seed=seed, px_noise=noise, **kw)
    rng = np.random.default_rng(seed)
    pert = [orc.se3_mul(orc.se3_exp(np.concatenate([rng.normal(0, dp, 3), rng.normal(0, dp / 2, 3)])), p) if not fixed[i] else p for i, p in enumerate(poses)]
    if di:
        idist = idist * np.clip(1 + di * rng.normal(size=len(idist)), 0.2, 3)
    return pert, fixed, idist, edges


def _assert_same_bits(a, b, what):
    (pa, ia, ca, ra), (pb, ib, cb, rb) = a, b
    assert bytes(ra) == bytes(rb), (what, "result")
    assert np.asarray(ia).tobytes() == np.asarray(ib).tobytes(), (what, "idist")
    assert np.asarray(ca).tobytes() == np.asarray(cb).tobytes(), (what, "chi2")
    assert len(pa) == len(pb)
    for v, (x, y) in enumerate(zip(pa, pb)):
        assert bytes(x) == bytes(y), (what, "pose", v)


def _same(a, b):
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _mixed_budget_problems(orc):
    # the five windows of tests/test_ba.py::test_ba_device_loop_mixed_budgets_in_one_call
    problems = []
    for shape, seed, n_iter, noise, dp, di in (((6, 150, 3), 71, 0, 0.3, 6e-3, 0.05), ((9, 300, 4), 72, 1, 0.3, 6e-3, 0.05), ((4, 60, 3), 73, 4, 0.3, 6e-3, 0.05),
                                              ((8, 250, 4), 74, 100, 0.5, 3e-2, 0.3), ((5, 90, 3), 75, 0, 0.3, 6e-3, 0.05)):
        pert, fixed, idist, edges = _perturbed(orc, shape, seed, noise, dp, di)
        problems.append((pert, fixed, idist, edges, 1.2, 0.6, n_iter))
    return problems


def _single_window_cases(orc):
    """name -> the arguments of ba_optimize"""
    cases = {}
    cases["one_block_per_phase"] = _perturbed(orc, (3, 25, 2), 43) + (1.0, 0.6, 10)
    cases["edge_and_point_blocks"] = _perturbed(orc, (9, 300, 4), 41) + (1.0, 0.6, 10)
    p = _perturbed(orc, (18, 120, 3), 81, n_fixed=2)
    assert int((np.asarray(p[1]) == 0).sum()) == 16                  # M = 96: the 72 KiB solve, 171 pose-pair blocks
    cases["sixteen_free_poses"] = p + (1.0, 0.6, 6)
    poses, fixed, idist, edges = synth.ba_problem(5, 120, 3, seed=61, px_noise=0.3)
    idist = idist * (1 + 0.02 * np.random.default_rng(61).normal(size=len(idist)))
    cases["points_only"] = (poses, np.ones(len(poses), np.uint8), idist, edges, 1.0, 0.7, 6)
    cases["errors_only_round"] = _perturbed(orc, (9, 300, 4), 41) + (1.0, 0.6, 0)
    cases["re_entry"] = _mixed_budget_problems(orc)[3]
    return cases


CASES = ["one_block_per_phase", "edge_and_point_blocks", "sixteen_free_poses", "points_only", "errors_only_round", "re_entry"]


@pytest.mark.parametrize("name", CASES)
def test_fused_equals_unfused_bit_for_bit(gpu_ctx, fused_ctx, orc, name):
    prob = _single_window_cases(orc)[name]
    before = fused_ctx.ba_debug_launches()
    f = fused_ctx.ba_optimize(*prob)
    after = fused_ctx.ba_debug_launches()
    u = gpu_ctx.ba_optimize(*prob)
    _assert_same_bits(f, u, name)
    launches = after[1] - before[1]
    assert launches >= 1 and after[0] - before[0] == launches, (before, after)      # the fused shape ran, and nothing else
    res = f[3]
    if name == "re_entry":
        # more rounds than one launch carries: the host's read-back of the states continues the window with further launches
        assert res.n_solves > capi.BA_FUSED_ROUNDS, res.n_solves
        # a round makes one trial; one more round may follow that only restores the state before a last rejected step
        assert launches in (-(-res.n_solves // capi.BA_FUSED_ROUNDS), -(-(res.n_solves + 1) // capi.BA_FUSED_ROUNDS)), (launches, res.n_solves)
    else:
        assert launches == 1, launches
    if name == "errors_only_round":
        assert res.iterations == 0 and res.n_solves == 0 and res.init_chi2 == res.final_chi2 > 0
        assert np.array_equal(f[1], prob[2])
    elif name == "points_only":
        assert res.n_accepted >= 1 and np.abs(f[1] - prob[2]).max() > 0
    else:
        assert res.n_solves >= 2 and res.n_accepted >= 1, (res.n_solves, res.n_accepted)


def test_fused_mixed_budgets_in_one_call(gpu_ctx, fused_ctx, orc):
    problems = _mixed_budget_problems(orc)
    multi_f = fused_ctx.ba_optimize_multi(problems)
    multi_u = gpu_ctx.ba_optimize_multi(problems)
    for q, p in enumerate(problems):
        _assert_same_bits(multi_f[q], fused_ctx.ba_optimize(*p), "window %d against its fused single call" % q)
        _assert_same_bits(multi_f[q], multi_u[q], "window %d against the unfused multi call" % q)
    assert multi_f[3][3].n_solves > capi.BA_FUSED_ROUNDS and multi_f[0][3].n_solves == 0


@pytest.mark.parametrize("shape,seed", [((9, 300, 4), 41), ((3, 25, 2), 43)])
def test_fused_oracle_parity(fused_ctx, orc, shape, seed):
    """the assertions of tests/test_ba.py::test_ba_optimize_parity, on the fused shape"""
    from test_ba import _obs_uv
    poses, fixed, idist, edges = synth.ba_problem(*shape, seed=seed, px_noise=0.3)
    rng = np.random.default_rng(seed)
    pert = [orc.se3_mul(orc.se3_exp(np.concatenate([rng.normal(0, 4e-3, 3), rng.normal(0, 2e-3, 3)])), p) if not fixed[i] else p
            for i, p in enumerate(poses)]
    uv = _obs_uv(edges, rng)
    hc_o, he_o = orc.ba_huber_deltas(pert, idist, edges, uv, 480.0)
    for n_iter in (10, 3):
        po, io, co, ro = orc.ba_optimize(pert, fixed, idist, edges, hc_o, he_o, n_iter)
        pg, ig, cg, rg = fused_ctx.ba_optimize(pert, fixed, idist, edges, hc_o, he_o, n_iter)
        assert (rg.iterations, rg.n_solves, rg.n_accepted, rg.stop) == (ro.iterations, ro.n_solves, ro.n_accepted, ro.stop)
        assert rg.init_chi2 == pytest.approx(ro.init_chi2, rel=1e-10) and rg.final_chi2 == pytest.approx(ro.final_chi2, rel=1e-8)
        assert rg.robust_chi2 == pytest.approx(ro.robust_chi2, rel=1e-8) and rg.lambda_ == pytest.approx(ro.lambda_, rel=1e-6)
        assert np.abs(ig - io).max() <= 1e-9
        for a, b_ in zip(pg, po):
            assert np.abs(np.array(a.q[:]) - np.array(b_.q[:])).max() <= 1e-9 and np.abs(np.array(a.t[:]) - np.array(b_.t[:])).max() <= 1e-9
        assert np.allclose(cg, co, rtol=1e-8, atol=1e-16)
    for i in np.where(fixed)[0]:
        assert pg[i].q[:] == pert[i].q[:] and pg[i].t[:] == pert[i].t[:]


def test_fused_local_multi_equals_unfused(gpu_ctx, fused_ctx):
    """hso_gpu_ba_local_multi: the Huber kernels run in front of the loop, whichever shape the loop has"""
    from test_ba import _obs_uv
    problems = []
    for shape, seed, n_iter in (((9, 300, 4), 51, 6), ((4, 60, 3), 52, 3), ((7, 201, 3), 54, 4)):
        poses, fixed, idist, edges = synth.ba_problem(*shape, seed=seed, px_noise=0.3)
        problems.append((poses, fixed, idist, edges, _obs_uv(edges, np.random.default_rng(seed)), n_iter))
    got_f, hub_f = fused_ctx.ba_local_multi(problems, 480.0)
    got_u, hub_u = gpu_ctx.ba_local_multi(problems, 480.0)
    assert hub_f.tobytes() == hub_u.tobytes() and np.all(hub_f > 0)
    for q in range(len(problems)):
        _assert_same_bits(got_f[q], got_u[q], "window %d" % q)
        assert got_f[q][3].n_solves >= 1


def test_launch_accounting(gpu_ctx, fused_ctx):
    problems = []
    for shape, seed, n_iter in (((9, 300, 4), 51, 10), ((4, 60, 3), 52, 3), ((12, 500, 5), 53, 6)):      # tests/test_ba.py::test_ba_optimize_multi_equals_single_calls
        poses, fixed, idist, edges = synth.ba_problem(*shape, seed=seed, px_noise=0.3)
        problems.append((poses, fixed, idist, edges, 1.0 + 0.1 * seed % 3, 0.6, n_iter))
    f0 = fused_ctx.ba_debug_launches()
    multi_f = fused_ctx.ba_optimize_multi(problems)
    f1 = fused_ctx.ba_debug_launches()
    assert (f1[0] - f0[0], f1[1] - f0[1]) == (1, 1), (f0, f1)          # every window is done inside the one launch
    u0 = gpu_ctx.ba_debug_launches()
    multi_u = gpu_ctx.ba_optimize_multi(problems)
    u1 = gpu_ctx.ba_debug_launches()
    assert u1[1] - u0[1] == 0 and u1[0] - u0[0] >= 10, (u0, u1)
    for q in range(len(problems)):
        _assert_same_bits(multi_f[q], multi_u[q], "window %d" % q)


def test_configure_refuses_other_values(gpu_ctx):
    ctx = capi.Context(0)
    for bad in (2, -1):
        with pytest.raises(capi.HsoGpuError):
            ctx.configure(ba_fused=bad)
    ctx.configure(ba_fused=1)
    ctx.configure()
    assert ctx.ba_debug_launches() == (0, 0)
    ctx.close()


def test_resident_windows_fused_equal_unfused(orc, tmp_path):
    """hso_gpu_seq_local_ba on recorded map states (the smallest case of tests/test_seq_ba.py): the written-back map, the window's
    state and the culling list, byte for byte"""
    import chain_state as cs
    from test_seq_ba import BA_CASES, _capture
    name, max_fts, n_frames, first = min(BA_CASES, key=lambda c: c[1])
    recs = _capture(synth.EUROC, max_fts, n_frames, first, tmp_path)
    assert len(recs) >= 2, len(recs)
    lib = cs.ChainLib(capi.load())
    for k, st, want, _ in recs[:3]:
        outs = []
        for fused in (1, 0):
            ls = cs.LoadedState(lib, st, None)
            o = capi.GpuOptions(C.sizeof(capi.GpuOptions))
            o.ba_fused = fused
            assert capi.load().hso_gpu_configure(ls.ctx, C.byref(o)) == 0
            outs.append(ls.run_ba(st["core"], st["fixed"], st["n_iter"], st["error_multiplier2"], st["chi2_corner"], st["chi2_edgelet"]))
            n = (C.c_int64 * 2)()
            assert capi.load().hso_gpu_ba_debug_launches(ls.ctx, n) == 0
            assert (n[1] == 1 and n[0] == 1) if fused else (n[1] == 0 and n[0] >= 10), (k, fused, n[0], n[1])   # an engine-shaped window: one launch
            ls.close()
        f, u = outs
        what = "%s frame %d" % (name, k)
        assert f["result"].tobytes() == u["result"].tobytes() and f["result"]["status"] == 0, what
        assert np.array_equal(f["point_ids"], u["point_ids"]) and f["point_state"].tobytes() == u["point_state"].tobytes(), what
        assert f["culled"].tobytes() == u["culled"].tobytes(), what
        for key in ("edge_chi2", "poses_out"):
            assert f["window"][key].tobytes() == u["window"][key].tobytes(), (what, key)
        for key in f["after"]:
            assert _same(f["after"][key], u["after"][key]), (what, key)
        assert f["point_state"].tobytes() == want["point_state"].tobytes(), what       # ... and what the engine's own (unfused) call left


def test_engine_with_ba_fused_equals_the_default():
    """hso_vo_options.ba_fused: two sequences at 200 features, every status record (pose, BA errors and removals), trajectory and
    keyframe list bit for bit; the bank's context ran k_ba_rounds only with the option"""
    spec = synth.EUROC
    cam = synth.camera(spec)
    n_frames = 34
    seqs = [synth.sequence(n_frames, spec=spec, seed=3100 + 17 * k, step=(0.016 + 0.002 * k, 0.005, 0.007 - 0.001 * k), workers=4) for k in range(2)]

    def run(ba_fused):
        multi = vo.MultiVisualOdometry(cam, len(seqs), 200)
        if ba_fused:
            multi.set_options(ba_fused=True)
        multi.set_first_frames([S["images"][0] for S in seqs], [S["depth0"] for S in seqs])
        got = []
        for k in range(1, n_frames):
            multi.add_images([S["images"][k] for S in seqs], [float(k)] * len(seqs))
            got.append([bytes(multi.status(q)) for q in range(len(seqs))])
        kfs = [[(ts, bytes(T), fid) for ts, T, fid in multi.keyframes(q)] for q in range(len(seqs))]
        traj = [tuple(a.tobytes() for a in multi.trajectory(q)) for q in range(len(seqs))]
        launches = multi.ba_launches()
        ba = [[(st.ba_error_init, st.ba_error_final, st.ba_removed_1, st.ba_removed_2) for st in (vo.VoStatus.from_buffer_copy(b[q]) for b in got)] for q in range(len(seqs))]
        multi.close()
        return got, kfs, traj, ba, launches

    on, off = run(True), run(False)
    assert on[0] == off[0] and on[1] == off[1] and on[2] == off[2] and on[3] == off[3]
    assert all(len(k) >= 2 for k in off[1]), [len(k) for k in off[1]]
    assert any(e[1] > 0 for q in off[3] for e in q), "no local BA ran"
    assert on[4][1] > 0 and on[4][0] == on[4][1], on[4]
    assert off[4][1] == 0 and off[4][0] >= 10, off[4]
