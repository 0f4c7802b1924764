"""GPU: the race-env kernels at the edges of their tables and modes.

A. A 32-gate track (the ABI's maximum, parity.ring_track) through every kernel family: the per-step kernel against the oracle for
   G = 9, 31, 32, the K-step kernels in every form bit-identical to each other and free-running against the oracle, the closed-loop
   kernels (rollout in both forwards, recorder, evaluator, grid evaluator with the 32-gate condition in the LAST slot of its bank)
   against the restatements they already have -- all from parity.ring_straddle_states, so that every gate index is passed, the
   31 -> 0 wrap is taken and the gates-ahead block is read across it.  Each test asserts that on the reference side first.
B. The K-step kernels in the two evaluation modes (pause_if_collision, pause): the reference's F9 recording through the K-step
   entry points, and a ragged batch against the oracle.

A `done` flag that differs from the oracle's is accepted only with parity.knife_edge_margin < 1e-5 from the oracle's pre-step state."""
import numpy as np
import pytest
import torch

import parity as P

pytestmark = pytest.mark.gpu

E2E, INDI = 0, 1
VNAME = {E2E: "e2e", INDI: "indi"}
SENTINEL = -77777.0
N = 293           # one full workgroup plus a ragged wave


@pytest.fixture(scope="module")
def PA():
    assert torch.cuda.is_available()
    from product_adapter import ProductAdapter

    return ProductAdapter


@pytest.fixture(scope="module")
def OA():
    from oracle_adapter import OracleAdapter

    return OracleAdapter


def _kw(variant, ga, blob, **more):
    return dict(gates_ahead=ga, residual=blob if variant == E2E else None, dist_ranges=P.TRAIN_DIST_RANGES if variant == E2E else None,
                seed=3, **more)


def _straddle(adapter, trk, n, seed):
    """put a product or oracle adapter on the ring's straddle states; returns them"""
    S = 16 if adapter.variant == E2E else 13
    w, d, t, s = P.ring_straddle_states(trk, n, S, seed=seed)
    adapter.set_state(w, d if adapter.variant == E2E else None, t, s)
    return w, d, t, s


def _bits_equal(a, b):
    if a is None:
        return b is None
    if a.dtype.is_floating_point:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def _all_bits_equal(xs, ys, what):
    for j, (x, y) in enumerate(zip(xs, ys)):
        assert _bits_equal(x, y), (what, j)


# ------------------------------------------------------------------------------------------------------------------------------------
# A1. per-step kernel against the oracle, one teacher-forced step
# ------------------------------------------------------------------------------------------------------------------------------------
_STEP_CASES = [(E2E, 32, ga) for ga in range(5)] + [(E2E, 9, 4), (E2E, 31, 4)] + [(INDI, G, ga) for G in (9, 31, 32) for ga in (0, 4)]


@pytest.mark.parametrize("variant,G,ga", _STEP_CASES, ids=["%s-G%d-ga%d" % (VNAME[v], g, a) for v, g, a in _STEP_CASES])
def test_per_step_kernel_passes_every_gate_of_the_ring(PA, OA, variant, G, ga, residual_blob):
    trk = P.ring_track(G)
    kw = _kw(variant, ga, residual_blob)
    g, o = PA(variant, N, trk, **kw), OA(variant, N, trk, **kw)
    w0, d0, t0, s0 = _straddle(o, trk, N, seed=G)
    _straddle(g, trk, N, seed=G)
    a = np.zeros((N, 4), np.float32)
    oo, ro, dno, tro = o.step(a)
    wo, _, to, so = o.get_state()
    passes, wraps = P.ring_pass_census(trk, t0, to, dno, ro)            # the oracle first: every gate passed, the wrap taken
    og, rg, dng, trg = g.step(a)
    wg, _, tg, sg = g.get_state()
    mism = dng != dno
    dropped = P.assert_knife_edges(variant, mism, w0, a, d0, residual_blob, trk, t0)
    ok = ~mism
    np.testing.assert_array_equal(tg[ok], to[ok])
    np.testing.assert_array_equal(sg[ok], so[ok])
    np.testing.assert_array_equal(trg, tro)
    e_rew = float(np.abs(rg[ok] - ro[ok]).max())
    e_state = float(P.rel_err(wg[ok], wo[ok]).max())
    e_obs = float(P.obs_err(og[ok], oo[ok], world=wo[ok]).max())
    print(f"per-step {VNAME[variant]} G={G} ga={ga}: passes per gate {passes.tolist()}, wraps {wraps}, dropped {dropped}, "
          f"worst state {e_state:.2e} obs {e_obs:.2e} reward {e_rew:.2e}")
    assert dropped <= 2, dropped
    assert e_rew < P.TOL_STEP_REWARD and e_state < P.TOL_STEP_STATE and e_obs < P.TOL_STEP_OBS, (e_rew, e_state, e_obs)
    assert og.shape == (N, (20 if variant == E2E else 13) + 4 * ga)
    if G == 32:
        pr, yr = o.env.track_tables()
        np.testing.assert_allclose(g.env.gate_pos_rel, pr, rtol=0, atol=5e-7)
        np.testing.assert_allclose(g.env.gate_yaw_rel, yr, rtol=0, atol=5e-7)
    g.env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# A2. K-step kernels: every form bit-identical, one of them free-running against the oracle
# ------------------------------------------------------------------------------------------------------------------------------------
def _actions(rng, variant, n, K):
    a = rng.uniform(-1, 1, size=(K, n, 4)).astype(np.float32)
    a[1::2] = (0.124 + 0.3 * a[1::2]) if variant == E2E else (0.2 * a[1::2] + np.array([0, 0, 0, 0.22], np.float32))
    return a.astype(np.float32)


def _free_run_against_oracle(variant, o, trk, acts, outs, final, blob, max_dropped, what):
    """The method of test_gpu_round5.test_fused_rollout_against_the_oracle_above_65536_envs: the oracle steps the same actions; an env
    whose `done` differs is dropped from then on, and only with the knife-edge proof from the oracle's pre-step state.  Returns the
    oracle's per-step (world after, done) for the callers that need them."""
    og, rg, dg, tg = (t.cpu().numpy() for t in outs)
    K, n = acts.shape[:2]
    valid = np.ones(n, bool)
    worst_obs, worst_rew, dones, worlds, dns = 0.0, 0.0, 0, [], []
    for k in range(K):
        w_pre, d_pre, t_pre, _ = o.get_state()
        oo, ro, dno, tro = o.step(acts[k])
        mism = (dg[k].astype(bool) != dno) & valid
        P.assert_knife_edges(variant, mism, w_pre, acts[k], d_pre, blob, trk, t_pre, where=f"{what} step {k}")
        valid &= ~mism
        np.testing.assert_array_equal(tg[k].astype(bool)[valid], tro[valid])
        worst_rew = max(worst_rew, float(np.abs(rg[k][valid] - ro[valid]).max()))
        wcur = o.get_state()[0]
        worst_obs = max(worst_obs, float(P.obs_err(og[k][valid], oo[valid], wcur[valid]).max()))
        dones += int(dno.sum())
        worlds.append(wcur); dns.append(dno)
    wg, _, tgt_g, sg = final
    wo2, _, to2, so2 = o.get_state()
    np.testing.assert_array_equal(tgt_g[valid], to2[valid])
    np.testing.assert_array_equal(sg[valid], so2[valid])
    worst_state = float(P.rel_err(wg[valid], wo2[valid]).max())
    dropped = int((~valid).sum())
    print(f"{what}: dones {dones}, dropped on knife edges {dropped}, worst state {worst_state:.2e} obs {worst_obs:.2e} reward {worst_rew:.2e}")
    assert dropped <= max_dropped, dropped
    assert worst_obs < P.TOL_FREE_RUN and worst_state < P.TOL_FREE_RUN and worst_rew < 5 * P.TOL_STEP_REWARD, (worst_obs, worst_state, worst_rew)
    return np.stack(worlds), np.stack(dns), valid, dones


def _k_step_paths(make, acts_np):
    """The same K steps through rollout_device in the given forms, step_sequence_device and K x step_device, each on a fresh handle
    from make(): [(name, kernel, (obs, rew, done, trunc), final state tensors, per-step world or None)]."""
    K = acts_np.shape[0]
    runs = []
    for path in ("auto", "general", "multi_wave", "general_multi_wave", "launches", "steps"):
        g = make()
        env = g.env
        acts = torch.as_tensor(acts_np).to(env.device)
        n, L = env.num_envs, env.state_len
        out = (torch.full((K, n, L), SENTINEL, device=env.device), torch.empty((K, n), device=env.device),
               torch.empty((K, n), dtype=torch.uint8, device=env.device), torch.empty((K, n), dtype=torch.uint8, device=env.device))
        worlds, kernel = None, ""
        if path == "launches":
            env.step_sequence_device(acts, out)
        elif path == "steps":
            worlds = []
            for k in range(K):
                o, r, d, t = env.step_device(acts[k].contiguous())
                if not env.pause:
                    out[0][k].copy_(o)
                out[1][k].copy_(r); out[2][k].copy_(d); out[3][k].copy_(t)
                worlds.append(env.get_state_tensors()[0].clone())
            worlds = torch.stack(worlds)
        else:
            env.set_rollout_form(path)
            kernel = env.rollout_kernel_name()
            env.rollout_device(acts, out)
        torch.cuda.synchronize()
        runs.append((path, kernel, out, env.get_state_tensors(), worlds, g))
    return runs


@pytest.mark.parametrize("variant,ga", [(E2E, 4), (E2E, 1), (INDI, 4), (INDI, 1)], ids=["e2e-ga4", "e2e-ga1", "indi-ga4", "indi-ga1"])
def test_k_step_kernels_on_the_ring_agree_and_follow_the_oracle(PA, OA, variant, ga, residual_blob):
    G, K = 32, 12
    trk = P.ring_track(G)
    kw = _kw(variant, ga, residual_blob)
    o = OA(variant, N, trk, **kw)
    o.env.set_limits(8, 0.01)                       # every env is auto-reset at step 8 and redraws a start on the ring
    o.reset()
    w0, d0, t0, s0 = _straddle(o, trk, N, seed=G)
    episode = o.env.episode.astype(np.int64)

    def make():
        g = PA(variant, N, trk, **kw)
        g.env.max_steps = 8
        g.reset()
        _straddle(g, trk, N, seed=G)
        g.env.set_state_tensors(episode=episode)
        return g

    acts = _actions(np.random.default_rng(11 + ga), variant, N, K)
    runs = _k_step_paths(make, acts)
    names = {r[0]: r[1] for r in runs}
    print("kernels:", names)
    assert "rollout_kernel" in names["general_multi_wave"] and "rollout_stash_kernel" in names["general"], names
    for path, _, out, state, _, _ in runs[1:]:
        _all_bits_equal(runs[0][2], out, path + " outputs")
        _all_bits_equal(runs[0][3], state, path + " final state")
    g0 = runs[0][5]
    _, dns, valid, dones = _free_run_against_oracle(variant, o, trk, acts, runs[0][2], g0.get_state(), residual_blob, 2,
                                                    f"K-step {VNAME[variant]} G=32 ga={ga} [{names['auto']}]")
    # the oracle's first step passed every gate and wrapped; its step 8 reset every env
    rew0 = runs[0][2][1][0].cpu().numpy()
    assert (rew0[valid] > 5.0).all() and not dns[0].any() and dones >= N
    for r in runs:
        r[5].env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# A3. closed-loop kernels on the 32-gate ring, gates_ahead = 4 (L = 36 / 29)
# ------------------------------------------------------------------------------------------------------------------------------------
def _prepare(trk, seed=32):
    def prepare(env):
        w, d, t, s = P.ring_straddle_states(trk, env.num_envs, env.STATE_LEN, seed=seed)
        env.set_state_tensors(world=w, dist=d if env.STATE_LEN == 16 else None, target=t, steps=s)
        env.update_states()
    return prepare


@pytest.mark.parametrize("variant", ["e2e", "indi"])
@pytest.mark.parametrize("precision", ["f16-operands", "f32"])
def test_closed_loop_rollout_on_the_ring_equals_policy_plus_step_launches(variant, precision):
    """qr_rollout_policy == K x [policy kernel, clip, step kernel] bit for bit (tests/test_gpu_policy.py) on the ring, L = 36 / 29,
    n = 256 + 37, K = 48, from the straddle states: the first step passes every gate and wraps 31 -> 0."""
    from test_gpu_policy import _closed_loop_equals_launches

    trk = P.ring_track(32)
    (obs, act, logp, rew, done, trunc, last), env = _closed_loop_equals_launches(variant, N, precision, 4, track=trk, prepare=_prepare(trk))
    S, t0 = env.STATE_LEN, np.arange(N) % 32
    assert obs.shape[-1] == (36 if variant == "e2e" else 29)
    assert not bool(done[0].any()) and bool((rew[0] > 5.0).all())       # every env passed its gate at the first step, gate 31 included
    # ... and the observation after it shows the rows of gates (t + 2 + a) % 32, read across the wrap
    rel = np.concatenate([env.gate_pos_rel, env.gate_yaw_rel[:, None]], axis=1)
    nxt = obs[1].cpu().numpy()[:, S:S + 16].reshape(N, 4, 4)
    for a in range(4):
        np.testing.assert_array_equal(nxt[:, a], rel[(t0 + 2 + a) % 32])
    print(f"closed loop {variant} {precision}: passes at step 0 {int((rew[0] > 5.0).sum())}, wraps {int((t0 == 31).sum())}, dones {int(done.sum())}")
    env.close()


def _ring_window(t0):
    def check(rows, s, final_target, what):
        end0, tgt0, tgt1, rew0 = rows[0, :, s + 5], rows[0, :, s + 6], rows[1, :, s + 6], rows[0, :, s + 4]
        exp0 = torch.as_tensor(t0, dtype=torch.float32, device=rows.device)
        assert torch.equal(tgt0, exp0) and bool((end0 == 0).all()) and bool((rew0 > 5.0).all()), what
        assert torch.equal(tgt1, (exp0 + 1) % 32), what                 # every gate passed at the first step, 31 -> 0 included
        ends = [int((rows[:, :, s + 5] == c).sum()) for c in (1, 2)]
        print(what, "passes at step 0:", rows.shape[1], "wraps:", int((exp0 == 31).sum()), "crashes / time-limit ends:", ends)
        assert ends[0] + ends[1] >= rows.shape[1] and ends[1] >= 1       # and every env was restarted inside the window
    return check


@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_flight_recorder_on_the_ring_equals_the_rollout_kernel(variant):
    """qr_record_policy == qr_rollout_policy bit for bit (tests/test_gpu_record.py) on the ring, gates_ahead 4, n = 256 + 37, K = 64,
    time limit 30, from the straddle states; stochastic, so that the command clip is exercised too."""
    from test_gpu_record import _rows_equal_the_rollout_kernel

    trk = P.ring_track(32)
    _rows_equal_the_rollout_kernel(variant, 4, N, "f16-operands", True, K=64, track=trk, prepare=_prepare(trk), max_steps=30,
                                   nonvacuous=_ring_window(np.arange(N) % 32))


@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_evaluator_on_the_ring_equals_the_spec(variant):
    """qr_evaluate_policy == tests/eval_spec.py over the per-step loop (tests/test_gpu_evaluate.py) on the ring, gates_ahead 4,
    n = 256 + 37, K = 64, time limit 30, one gate per lap, from the straddle states."""
    from test_gpu_evaluate import _records_equal_the_spec_closed_loop

    trk = P.ring_track(32)

    def nonvacuous(srec):
        print(f"evaluator {variant}: passes {int(srec[:, 0].sum())}, crashes {int(srec[:, 1].sum())}, time-limit ends {int(srec[:, 2].sum())}, "
              f"laps {srec[:, 14:22].sum(axis=0).tolist()}")
        assert (srec[:, 0] >= 1).all() and (srec[:, 14] >= 1).all()      # every env passed its gate: those at gate 31 wrapped to 0
        assert (srec[:, 1] + srec[:, 2] >= 1).all()                       # and was restarted inside the window

    _records_equal_the_spec_closed_loop(variant, 4, N, "f32", K=64, gpl=1, track=trk, prepare=_prepare(trk), max_steps=30, nonvacuous=nonvacuous)


@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_grid_evaluator_with_the_ring_in_the_last_condition_slot(variant):
    """qr_evaluate_policy_grid with a capacity-3 condition bank whose LAST slot holds the 32-gate ring (the slot-stride boundary):
    every group equals the standalone evaluator on a twin handle bit for bit, as in tests/test_gpu_eval_grid.py.  The ring groups
    start from the straddle states (group and twin alike), so gate passes and the wrap are in the records."""
    import eval_spec as S
    import test_gpu_eval_grid as TG
    from optimal_quad_control_rl_amd import TRAIN_DISTURBANCE_RANGES
    from optimal_quad_control_rl_amd.conditions import Condition
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    E, K, ga, precision = 256, 64, 4, "f16-operands"
    trk = P.ring_track(32)
    conds = TG._conditions(variant)[:2] + [Condition("ring 32", *trk, TRAIN_DISTURBANCE_RANGES if variant == "e2e" else None, 1.0, 30, 1)]
    pol, cog = [0, 0, 1], [0, 2, 2]
    # the handle's own configuration is none of the conditions' (the call must not use it), but has 32 gates: qr_set_state reduces
    # the targets it is given modulo the HANDLE's gate count
    env = TG._twin(variant, len(pol) * E, ga, conds[2].replace(max_steps=97, start_pos=(0.3, -0.2, -1.0), gate_pos=trk[0] + np.float32(0.2)))
    sets = TG._two_policies(variant, env.state_len)
    pbank, cbank = TG._policy_bank(env.state_len, sets), TG._condition_bank(variant, conds, capacity=3)
    env.condition_starts(conds, cog, E)
    w, d, t, s = P.ring_straddle_states(trk, E, env.STATE_LEN, seed=32)
    world, dist, target, steps, episode = env.get_state_tensors()
    for g in (1, 2):
        sl = slice(g * E, (g + 1) * E)
        world[sl] = torch.as_tensor(w).to(env.device); target[sl] = torch.as_tensor(t).to(env.device); steps[sl] = 0
        if dist is not None:
            dist[sl] = torch.as_tensor(d).to(env.device)
    env.set_state_tensors(world, dist, target, steps, episode)
    assert torch.equal(env.get_state_tensors()[2], target) and int(target.max()) == 31
    rec, recf = TG._records(env)
    env.evaluate_grid_device(pbank, cbank, pol, cog, E, K, rec, recf, precision=precision)
    after, obs_after = env.get_state_tensors(), env.states_tensor.clone()
    for g in range(len(pol)):
        lo, hi = g * E, (g + 1) * E
        twin = TG._twin(variant, E, ga, conds[cog[g]])
        if cog[g] == 2:
            _prepare(trk)(twin)
        mp = MfmaPolicy(twin.state_len).set_weights(sets[pol[g]])
        trec, trecf = TG._records(twin)
        twin.evaluate_device(mp, K, conds[cog[g]].gates_per_lap, trec, trecf, precision=precision)
        srec = trec.cpu().numpy()
        print(f"grid {variant} group {g} ({conds[cog[g]].name}): passes {int(srec[:, 0].sum())}, crashes {int(srec[:, 1].sum())}, "
              f"time-limit ends {int(srec[:, 2].sum())}")
        if cog[g] == 2:
            assert (srec[:, 0] >= 1).all() and (srec[:, 14] >= 1).all() and (srec[:, 1] + srec[:, 2] >= 1).all()
        assert torch.equal(rec[lo:hi], trec), ("integer records", g)
        assert torch.equal(recf[lo:hi].view(torch.int32), trecf.view(torch.int32)), ("float records", g)
        TG._group_equals(after, twin, lo, hi, "group %d" % g)
        assert torch.equal(obs_after[lo:hi], twin.states_tensor), ("observation buffer", g)
        twin.close(); mp.close()
    env.close(); pbank.close(); cbank.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# A4. ABI edge: 33 gates
# ------------------------------------------------------------------------------------------------------------------------------------
def test_set_track_refuses_33_gates_and_keeps_the_32_gate_track(PA, residual_blob):
    import ctypes as C
    from optimal_quad_control_rl_amd import _lib

    trk = P.ring_track(32)

    def one_step(g):
        _straddle(g, trk, N, seed=32)
        return g.step(np.full((N, 4), 0.1, np.float32)) + g.get_state()

    g = PA(E2E, N, trk, **_kw(E2E, 4, residual_blob))
    before = one_step(g)
    gp, gy, sp = (np.ascontiguousarray(x, np.float32) for x in P.ring_track(33))
    f32p = C.POINTER(C.c_float)
    code = g.env._L.qr_set_track(g.env._h, gp.ctypes.data_as(f32p), gy.ctypes.data_as(f32p), 33, sp.ctypes.data_as(f32p))
    msg = g.env._L.qr_last_error().decode()
    assert code == _lib.QR_E_INVALID and "qr_set_track" in msg and "QR_MAX_GATES" in msg, (code, msg)
    assert _lib.QR_MAX_GATES == 32
    after = one_step(g)
    for x, y in zip(before, after):
        assert x is None or np.array_equal(x, y, equal_nan=True)
    g.env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# B1. the reference's F9 recording through the K-step entry points
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["general", "general_multi_wave", "launches"])
@pytest.mark.parametrize("variant", [E2E, INDI], ids=["e2e", "indi"])
def test_f9_modes_through_the_k_step_entry_points(PA, variant, path, residual_blob):
    """tests/golden/f9_modes.npz (4 envs, 40 steps, pause_if_collision from the start, pause from `pause_from_step`) as TWO K-step
    calls: [0, pause_from) and, with pause set, [pause_from, 40).  Reward / observation / world within 1e-4, done / target / steps
    exact (test_gpu_golden.test_modes' tolerances); under pause the world is bit-unchanged and no observation row is written."""
    vname = VNAME[variant]
    d = P.load("f9_modes")
    acts_np = d[vname + "_actions"]
    H, n = acts_np.shape[:2]
    p0 = int(d[vname + "_pause_from_step"])
    assert 0 < p0 < H
    g = PA(variant, n, P.tracks()["zigzag"], gates_ahead=1, residual=residual_blob, pause_if_collision=True)
    env = g.env
    g.set_state(d[vname + "_world0"], d[vname + "_dist0"] if variant == E2E else None, d[vname + "_target0"], d[vname + "_steps0"])
    g.observe()
    acts = torch.as_tensor(np.ascontiguousarray(acts_np, dtype=np.float32)).to(env.device)
    if path != "launches":
        env.set_rollout_form(path)
    expected = "rollout_stash_kernel" if path == "general" else "rollout_kernel"

    def call(lo, hi):
        K = hi - lo
        out = (torch.full((K, n, env.state_len), SENTINEL, device=env.device), torch.full((K, n), SENTINEL, device=env.device),
               torch.full((K, n), 7, dtype=torch.uint8, device=env.device), torch.full((K, n), 7, dtype=torch.uint8, device=env.device))
        if path == "launches":
            env.step_sequence_device(acts[lo:hi].contiguous(), out)
        else:
            assert env.rollout_kernel_name() == "qr::%s<%d, 1>" % (expected, variant), env.rollout_kernel_name()
            env.rollout_device(acts[lo:hi].contiguous(), out)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out]

    def check(lo, hi, out, observed):
        obs, rew, done, trunc = out
        worst = [0.0, 0.0]
        for k in range(lo, hi):
            np.testing.assert_array_equal(done[k - lo].astype(bool), d[vname + "_done"][k].astype(bool), err_msg=f"step {k}")
            worst[0] = max(worst[0], float(np.abs(rew[k - lo] - d[vname + "_reward"][k]).max()))
            if observed:
                worst[1] = max(worst[1], float(P.obs_err(obs[k - lo], d[vname + "_obs"][k]).max()))
        w, _, t, s = g.get_state()
        np.testing.assert_array_equal(t, d[vname + "_target"][hi - 1])
        np.testing.assert_array_equal(s, d[vname + "_steps"][hi - 1])
        e_world = float(P.rel_err(w, d[vname + "_world"][hi - 1]).max())
        print(f"F9 {vname} {path} steps [{lo}, {hi}): worst reward {worst[0]:.2e} obs {worst[1]:.2e} world {e_world:.2e}, dones {int(done.astype(bool).sum())}")
        assert worst[0] < 1e-4 and worst[1] < 1e-4 and e_world < 1e-4, (worst, e_world)
        return w

    check(0, p0, call(0, p0), observed=True)
    before = env.get_state_tensors()[0].clone()
    g.set_pause(True)
    out = call(p0, H)
    check(p0, H, out, observed=False)
    assert _bits_equal(env.get_state_tensors()[0], before)              # pause: no world write-back ...
    assert (out[0] == SENTINEL).all()                                   # ... and no observation store
    assert not out[2].any()                                             # R:570-572: nothing is done while paused
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# B2. pause_if_collision at a ragged size against the oracle
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,tname", [(E2E, "zigzag"), (INDI, "square")], ids=["e2e", "indi"])
def test_pause_if_collision_k_step_kernels_agree_and_follow_the_oracle(PA, OA, variant, tname, residual_blob):
    """n = 300, K = 40, pause_if_collision: an env that ends (a third start just above the ground and crash into it, the others
    run into the time limit of 30 at staggered steps; on the CPU oracle alone: 300 of 300 frozen, 100 before their limit) is FROZEN,
    not reset.  rollout_device in both general forms, step_sequence_device and K x step_device are bit-identical; one of them
    follows the oracle free-running (knife-edge drops <= 2); a frozen env's world row stays bit-identical from its terminal step to
    the end on both sides, and its done / reward afterwards are the oracle's."""
    n, K = 300, 40
    trk = P.tracks()[tname]
    kw = _kw(variant, 1, residual_blob, pause_if_collision=True)
    o = OA(variant, n, trk, **kw)
    o.env.set_limits(30, 0.01)
    o.reset()
    w0, d0, t0, _ = o.get_state()
    low = np.arange(n) % 3 == 0                     # a third of the envs 1 .. 15 cm above the ground, sinking at 1 m/s: ground crashes
    w0[low, 2] = (-0.01 - 0.14 * ((np.arange(n) * 0.6180339887) % 1.0)).astype(np.float32)[low]
    w0[low, 5] = 1.0
    s0 = np.where(low, 0, np.random.default_rng(4).integers(0, 30, n)).astype(np.int32)   # the others: the time limit, staggered
    o.set_state(w0, d0, t0, s0)
    episode = o.env.episode.astype(np.int64)

    def make():
        g = PA(variant, n, trk, **kw)
        g.env.max_steps = 30
        g.reset()
        g.set_state(w0, d0 if variant == E2E else None, t0, s0)
        g.env.set_state_tensors(episode=episode)
        return g

    acts = _actions(np.random.default_rng(8), variant, n, K)
    runs = [r for r in _k_step_paths(make, acts) if r[0] in ("general", "general_multi_wave", "launches", "steps")]
    names = {r[0]: r[1] for r in runs}
    assert "rollout_stash_kernel" in names["general"] and "rollout_kernel" in names["general_multi_wave"], names
    for path, _, out, state, _, _ in runs[1:]:
        _all_bits_equal(runs[0][2], out, path + " outputs")
        _all_bits_equal(runs[0][3], state, path + " final state")
    steps_run = [r for r in runs if r[0] == "steps"][0]
    worlds_o, dns, valid, _ = _free_run_against_oracle(variant, o, trk, acts, runs[0][2], steps_run[5].get_state(), residual_blob, 2,
                                                       f"pause_if_collision {VNAME[variant]} n={n} [{names['general']}]")
    frozen = dns.any(axis=0)
    first = np.where(frozen, dns.argmax(axis=0), K)
    crashes = int((frozen & (s0 + first + 1 < 30)).sum())
    print(f"frozen envs {int(frozen.sum())} of {n} (before their time limit: {crashes})")
    assert frozen.sum() >= n / 3 and crashes >= n / 6                   # the oracle alone froze at least a third of the envs
    worlds_g = steps_run[4].cpu().numpy()
    w_start = np.asarray(w0, np.float32)
    for side, worlds in (("oracle", worlds_o), ("product", worlds_g)):
        for i in np.nonzero(frozen & valid)[0]:
            k0 = first[i]
            held = worlds[k0 - 1, i] if k0 > 0 else w_start[i]
            assert (worlds[k0:, i].view(np.uint32) == held.view(np.uint32)).all(), (side, i, k0)
    for r in runs:
        r[5].env.close()
