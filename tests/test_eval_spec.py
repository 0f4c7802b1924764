"""CPU: the lap / crash accounting specification (tests/eval_spec.py) on hand-written sequences with known answers, its chunking
property, its agreement with the reference's rule for lap times (every gates_per_lap-th gate-passage time, differenced -- what
get_gate_passage_times / get_lap_times do, FP:261-289, restated here), and the non-vacuity of the scenario the GPU comparison uses,
established on the CPU oracle."""
import numpy as np
import pytest

import eval_spec as S


def _seq(K, passes=(), done=(), trunc=(), num_gates=8):
    """One env: target-before / target-after / done / trunc / reward sequences of K steps with passes and finishes at the given
    1-based step numbers (a finish resets the target to 0)."""
    tb, ta = np.zeros((K, 1), np.int64), np.zeros((K, 1), np.int64)
    dn, tr = np.zeros((K, 1), bool), np.zeros((K, 1), bool)
    t = 0
    for k in range(K):
        tb[k] = t
        if k + 1 in passes:
            t = (t + 1) % num_gates
        if k + 1 in done or k + 1 in trunc:
            dn[k] = True
            tr[k] = k + 1 in trunc
            t = 0
        ta[k] = t
    return tb, ta, dn, tr, np.ones((K, 1), np.float32)


def test_a_gate_every_63_steps_gives_laps_of_252_steps():
    K = 63 * 4 * 3 + 10
    rec, recf = S.new_records(1)
    S.run(rec, recf, *_seq(K, passes=range(63, K + 1, 63)), gates_per_lap=4)
    r = rec[0]
    assert r[0] == 12 and r[1] == 0 and r[2] == 0 and r[3] == 12 and r[4] == 756 and r[5] == K
    assert r[6:14].tolist() == [252, 252, 252, 0, 0, 0, 0, 0]
    assert r[14:22].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    assert r[22] == 0 and r[23] == 0
    assert recf[0].tolist() == [float(K), 0.0, 0.0, 0.0]


def test_a_crash_mid_lap_restarts_the_count_and_the_clock():
    # passes at 50, 100, 150 (three of four), crash at 170, then passes at 200, 230, 260, 290: lap 1 = 290 - 170 = 120 steps
    rec, recf = S.new_records(1)
    S.run(rec, recf, *_seq(300, passes=(50, 100, 150, 200, 230, 260, 290), done=(170,)), gates_per_lap=4)
    r = rec[0]
    assert r[0] == 7 and r[1] == 1 and r[2] == 0 and r[3] == 4 and r[4] == 290 and r[5] == 300
    assert r[6:14].tolist() == [120, 0, 0, 0, 0, 0, 0, 0] and r[14:22].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    # returns: the episode that ended at step 170 earned 170; 130 steps into the running one
    assert recf[0].tolist() == [130.0, 170.0, 170.0 * 170.0, 0.0]


def test_a_time_limit_end_is_counted_apart_from_a_crash():
    rec, recf = S.new_records(1)
    S.run(rec, recf, *_seq(100, done=(30,), trunc=(80,)), gates_per_lap=4)
    assert rec[0, 1] == 1 and rec[0, 2] == 1 and rec[0, 4] == 80
    assert recf[0].tolist() == [20.0, 80.0, 30.0 * 30.0 + 50.0 * 50.0, 0.0]


def test_a_pass_on_a_done_step_is_not_counted():
    tb, ta, dn, tr, rw = _seq(20, passes=(5,), done=(10,))
    tb[9], ta[9] = 1, 0          # the target moved on the finishing step (pass + reset, as seen from outside): not a pass
    rec, recf = S.new_records(1)
    S.run(rec, recf, tb, ta, dn, tr, rw, gates_per_lap=1)
    assert rec[0, 0] == 1 and rec[0, 1] == 1 and rec[0, 3] == 0 and rec[0, 14] == 1 and rec[0, 6] == 5
    # ... and with a reset target that differs from the one before (num_gates > 2, reset to 0 from gate 5) it is still no pass
    rec2, _ = S.new_records(1)
    S.step(rec2, None, [5], [0], [True], [False], None, 1)
    assert rec2[0, 0] == 0 and rec2[0, 1] == 1


def test_a_ninth_lap_is_not_recorded_but_moves_the_boundary():
    K = 10 * 9 + 5
    rec, _ = S.new_records(1)
    tb, ta, dn, tr, _ = _seq(K, passes=range(10, K + 1, 10))
    S.run(rec, None, tb, ta, dn, tr, None, gates_per_lap=1)
    r = rec[0]
    assert r[0] == 9 and r[3] == 9 and r[4] == 90 and r[5] == K
    assert r[6:14].tolist() == [10] * 8 and r[14:22].tolist() == [1] * 8


def _random_sequences(rng, K, n, num_gates, p_pass, p_done):
    tb, ta = np.zeros((K, n), np.int64), np.zeros((K, n), np.int64)
    dn, tr = rng.random((K, n)) < p_done, rng.random((K, n)) < 0.3
    tr &= dn
    ps = rng.random((K, n)) < p_pass
    t = np.zeros(n, np.int64)
    for k in range(K):
        tb[k] = t
        t = np.where(ps[k], (t + 1) % num_gates, t)
        t = np.where(dn[k], 0, t)
        ta[k] = t
    rw = rng.normal(0, 3, (K, n)).astype(np.float32)
    return tb, ta, dn, tr, rw


def test_split_sequence_equals_the_whole():
    rng = np.random.default_rng(0)
    K, n = 2000, 257
    seq = _random_sequences(rng, K, n, 8, 0.02, 0.002)
    whole = S.run(*S.new_records(n), *seq, gates_per_lap=4)
    for cut in (1200, 1, 1999, 777):
        rec, recf = S.new_records(n)
        S.run(rec, recf, *[a[:cut] for a in seq], gates_per_lap=4)
        S.run(rec, recf, *[a[cut:] for a in seq], gates_per_lap=4)
        assert np.array_equal(rec, whole[0]) and np.array_equal(recf.view(np.uint32), whole[1].view(np.uint32)), cut
    assert whole[0][:, 14:22].sum() > 0 and whole[0][:, 1].sum() > 0 and whole[0][:, 2].sum() > 0


def test_lap_durations_are_differences_of_every_gates_per_lap_th_passage_time():
    """The reference's rule (FP:261-289): gate_passage_times = [0] + the time of every pass; lap_times = differences of every
    gates_per_lap-th entry.  Restated for a crash-free env in steps."""
    rng = np.random.default_rng(1)
    K, n, gpl = 3000, 64, 3
    tb, ta, dn, tr, rw = _random_sequences(rng, K, n, 6, 0.01, 0.0)
    rec, _ = S.new_records(n)
    S.run(rec, None, tb, ta, dn, tr, None, gates_per_lap=gpl)
    assert rec[:, 14].sum() > n / 2
    for i in range(n):
        passage = [0] + [k + 1 for k in range(K) if ta[k, i] != tb[k, i]]
        laps = np.diff(passage[::gpl])
        assert rec[i, 0] == len(passage) - 1
        assert rec[i, 14:22].tolist() == [1 if q < len(laps) else 0 for q in range(8)]
        assert rec[i, 6:14].tolist() == [int(laps[q]) if q < len(laps) else 0 for q in range(8)]
        assert rec[i, 4] == (passage[::gpl][-1] if len(laps) else 0)


def _oracle_scenario(variant, residual_blob):
    from oracle import oracle as O

    import parity as P

    sc = S.SCENARIO
    gp, gy, sp = S.scenario_track()
    n, K = sc["envs"], sc["steps"]
    env = O.OracleEnv(O.E2E if variant == "e2e" else O.INDI, n, gp, gy, sp, sc["gates_ahead"])
    if variant == "e2e":
        env.set_residual(residual_blob)
        env.set_disturbance(P.TRAIN_DIST_RANGES, 1.0)
    env.set_limits(sc["max_steps"], 0.01)
    env.seed(sc["seed"])
    env.reset()
    act = np.tile(np.asarray(sc[variant + "_action"], np.float32), (n, 1))
    rec, recf = S.new_records(n)
    for _ in range(K):
        tb = env.target_gates.copy()
        _, rew, done, trunc = env.step(act)
        S.step(rec, recf, tb, env.target_gates, done, trunc, rew, sc[variant + "_gates_per_lap"])
    return rec, recf


def test_gpu_scenario_is_not_vacuous_indi(residual_blob):
    rec, recf = _oracle_scenario("indi", residual_blob)
    nv = S.nonvacuous_indi(rec)
    print(nv, "passes", int(rec[:, 0].sum()))
    assert nv["ok"], nv
    assert int((rec[:, 1] + rec[:, 2]).sum()) > 0 and float(np.abs(recf[:, 2]).sum()) > 0


def test_gpu_scenario_is_not_vacuous_e2e(residual_blob):
    rec, recf = _oracle_scenario("e2e", residual_blob)
    nv = S.nonvacuous_e2e(rec)
    print(nv, "passes", int(rec[:, 0].sum()))
    assert nv["ok"], nv
