"""CPU: the black box's bookkeeping specification (tests/blackbox_spec.py) on hand-made rows, CrashLog's unrolling and tables against
it, the Python binding on a library without the entry point, and the package surface (the C entry point itself is pinned in
tests/abi_table.py)."""
import numpy as np
import pytest

import blackbox_spec as B

S_LEN = 13
R = S_LEN + 8


def _rows(K, ends):
    """[K][M][R] rows whose every element names its (step, env, column); ends[i] = {step: end code} of env i"""
    M = len(ends)
    rows = (1000.0 * np.arange(K)[:, None, None] + 100.0 * np.arange(M)[None, :, None] + np.arange(R)[None, None, :]).astype(np.float32)
    rows[:, :, S_LEN + 5] = 0.0
    for i, e in enumerate(ends):
        for k, code in e.items():
            rows[k, i, S_LEN + 5] = code
    rows[:, :, S_LEN + 6] = (np.arange(K)[:, None] // 3 + np.arange(M)[None, :]) % 4          # target gate
    return rows


# env 0 crashes at step 0; env 1 crashes at 3 (< W - 1) and again at 9; env 2 never ends; env 3 hits the time limit at 5, crashes at 11
ENDS = [{0: 1.0}, {3: 1.0, 9: 1.0}, {}, {5: 2.0, 11: 1.0}]


@pytest.mark.parametrize("first_step", [0, 5, 2 ** 33 + 3])
def test_spec_on_hand_made_rows(first_step):
    K, W = 14, 8
    rows = _rows(K, ENDS)
    slot = lambda k: (first_step + k) % W
    written, st, trig = B.run(rows, first_step, W, B.ON_CRASH)
    assert trig.tolist() == [0, 3, -1, 11]
    assert st.tolist() == [[1, 1, slot(0), 0], [1, 4, slot(3), 0], [0, 14, -1, 0], [1, 12, slot(11), 0]]
    assert sorted(written[0]) == [slot(0)] and np.array_equal(written[0][slot(0)], rows[0, 0])          # a trigger at step 0: one row
    assert sorted(written[1]) == sorted(slot(k) for k in range(4))                                      # a trigger at c < W - 1: c + 1 rows
    for k in range(4):
        assert np.array_equal(written[1][slot(k)], rows[k, 1])
    assert sorted(written[2]) == list(range(W))                                                         # no trigger: the last W steps
    for k in range(K - W, K):
        assert np.array_equal(written[2][slot(k)], rows[k, 2])
    for k in range(11 - W + 1, 12):                                                                     # the time-limit end at 5 is not a crash
        assert np.array_equal(written[3][slot(k)], rows[k, 3])
    # the valid slots, oldest first, end at the trigger slot / at the last step's slot
    assert B.valid_slots(st[1], first_step, K, W) == [slot(k) for k in range(4)]
    assert B.valid_slots(st[2], first_step, K, W) == [slot(k) for k in range(K - W, K)]
    assert B.valid_slots(st[3], first_step, K, W) == [slot(k) for k in range(4, 12)]
    # the other triggers
    assert B.run(rows, first_step, W, B.ON_TIME_LIMIT)[2].tolist() == [-1, -1, -1, 5]
    assert B.run(rows, first_step, W, B.ON_CRASH | B.ON_TIME_LIMIT)[2].tolist() == [0, 3, -1, 5]
    w0, st0, trig0 = B.run(rows, first_step, W, 0)                                                      # trigger 0: the last W steps of every env
    assert trig0.tolist() == [-1] * 4 and st0.tolist() == [[0, 14, -1, 0]] * 4
    for i in range(4):
        assert sorted(w0[i]) == list(range(W)) and all(np.array_equal(w0[i][slot(k)], rows[k, i]) for k in range(K - W, K))


def test_spec_with_fewer_steps_than_slots():
    K, W, first = 5, 8, 6
    rows = _rows(K, [{}, {2: 1.0}])
    source, st, trig = B.run_arrays(rows, first, W, 1)
    assert st.tolist() == [[0, 5, -1, 0], [1, 3, 0, 0]] and trig.tolist() == [-1, 2]
    assert source[:, 0].tolist() == [2, 3, 4, -1, -1, -1, 0, 1]                                         # slots 3, 4, 5 are never touched
    assert source[:, 1].tolist() == [2, -1, -1, -1, -1, -1, 0, 1]
    ring = B.ring_from_source(rows, source, -7.0)
    assert (ring[3:6] == -7.0).all() and (ring[1:6, 1] == -7.0).all() and np.array_equal(ring[0, 1], rows[2, 1])
    assert B.valid_slots(st[0], first, K, W) == [6, 7, 0, 1, 2] and B.valid_slots(st[1], first, K, W) == [6, 7, 0]


@pytest.mark.parametrize("trigger", [0, 1, 2, 3])
@pytest.mark.parametrize("K1", [1, 4, 6, 13])
def test_spec_two_calls_equal_one(trigger, K1):
    K, W, first = 14, 8, 3
    rows = _rows(K, ENDS)
    src, st, trig = B.run_arrays(rows, first, W, trigger)
    whole = B.ring_from_source(rows, src, -7.0)
    s1, st1, t1 = B.run_arrays(rows[:K1], first, W, trigger)
    ring1 = B.ring_from_source(rows[:K1], s1, -7.0)
    s2, st2, t2 = B.run_arrays(rows[K1:], first + K1, W, trigger, st1)
    ring2 = B.ring_from_source(rows[K1:], s2, ring1)
    assert np.array_equal(ring2, whole) and np.array_equal(st2, st)
    assert np.array_equal(np.where(t1 >= 0, t1, np.where(t2 >= 0, t2 + K1, -1)), trig)
    assert not (s2[:, st1[:, 0] != 0] >= 0).any()                                                        # an env frozen by the first call stores nothing more


def test_cause_bits():
    t = np.zeros(13, np.float32)
    t[2] = -1.0
    assert B.cause_bits(t, 1) == B.CAUSE_GATE and B.cause_bits(t, 2) == B.CAUSE_TIME_LIMIT
    g = t.copy(); g[2] = 1e-6
    assert B.cause_bits(g, 1) == B.CAUSE_GROUND and B.cause_bits(g, 2) == B.CAUSE_GROUND | B.CAUSE_TIME_LIMIT
    for col, v in ((0, 10.5), (1, -10.5), (9, 1001.0), (10, -1001.0), (11, 1e4)):
        o = t.copy(); o[col] = v
        assert B.cause_bits(o, 1) == B.CAUSE_OOB
    e = t.copy(); e[0] = 10.0; e[9] = 1000.0; e[2] = 0.0                                                 # the comparisons are strict
    assert B.cause_bits(e, 1) == B.CAUSE_GATE
    b = g.copy(); b[1] = 11.0
    assert B.cause_bits(b, 1) == B.CAUSE_GROUND | B.CAUSE_OOB


# ---------------------------------------------------------------------------------------------------------------------------------
# CrashLog against the spec
# ---------------------------------------------------------------------------------------------------------------------------------
def _crash_log(first_step, trigger, K=14, W=8):
    from optimal_quad_control_rl_amd.blackbox import CrashLog

    rows = _rows(K, ENDS)
    source, st, trig = B.run_arrays(rows, first_step, W, trigger)
    ring = B.ring_from_source(rows, source, np.nan)
    term = np.arange(4 * S_LEN, dtype=np.float32).reshape(4, S_LEN)
    for i in np.nonzero(trig >= 0)[0]:
        st[i, 3] = [B.CAUSE_GROUND, B.CAUSE_GATE, 0, B.CAUSE_TIME_LIMIT | B.CAUSE_OOB][i]
    return CrashLog(ring, st, term, first_step + K - 1, 0.01), rows, st, trig


@pytest.mark.parametrize("first_step", [0, 5, 21])
@pytest.mark.parametrize("trigger", [0, 1, 3])
def test_crash_log_unrolls_and_pads_like_the_spec(first_step, trigger, tmp_path):
    K, W = 14, 8
    log, rows, st, trig = _crash_log(first_step, trigger)
    assert (log.window, log.num_envs, log.row_len, log.state_len) == (W, 4, R, S_LEN)
    assert np.array_equal(log.frozen, trig >= 0) and np.array_equal(log.frozen_envs(), np.nonzero(trig >= 0)[0])
    for i in range(4):
        last = trig[i] if trig[i] >= 0 else K - 1
        v = min(last + 1, W)
        assert log.valid[i] == v and log.slots(i) == B.valid_slots(st[i], first_step, K, W)
        assert np.array_equal(log.flight(i), rows[last - v + 1:last + 1, i])                              # oldest -> newest
        fr = log.as_flight_record(i)
        assert fr.rows.shape == (v, 1, R) and np.array_equal(fr.end[:, 0], rows[last - v + 1:last + 1, i, S_LEN + 5])
    padded, valid, envs = log.flights()
    assert padded.shape == (len(envs), W, R) and np.array_equal(valid, log.valid[envs])
    for j, i in enumerate(envs):
        assert np.array_equal(padded[j, :valid[j]], log.flight(i)) and np.isnan(padded[j, valid[j]:]).all()
    if len(envs):
        assert np.array_equal(log.trigger_rows(), rows[trig[envs], envs])
    ts = log.terminal_state
    assert np.isnan(ts[~log.frozen]).all() and np.array_equal(ts[log.frozen], log.terminal[log.frozen])
    with np.load(log.save_npz(str(tmp_path / "log.npz"))) as z:
        assert sorted(z.files) == sorted(["ring", "status", "terminal", "last_step", "dt", "flights", "valid", "envs"])
        assert np.array_equal(z["status"], st) and int(z["last_step"]) == first_step + K - 1 and np.array_equal(z["envs"], envs)
        assert np.array_equal(z["flights"], padded, equal_nan=True)


def test_cause_counts_and_by_gate_on_synthetic_status():
    from optimal_quad_control_rl_amd.blackbox import CrashLog

    W, M = 4, 6
    ring = np.zeros((W, M, R), np.float32)
    #            frozen rows slot cause
    st = np.array([[1, 9, 2, 1], [1, 3, 2, 8], [0, 7, -1, 0], [1, 4, 3, 4 | 2], [1, 1, 0, 8], [1, 2, 1, 1 | 2]], np.int32)
    for i, gate in enumerate([3, 0, 2, 1, 0, 3]):
        ring[:, i, S_LEN + 6] = 5                      # only the trigger row's target counts
        if st[i, 0]:
            ring[st[i, 2], i, S_LEN + 6] = gate
    log = CrashLog(ring, st, None, 11, 0.01)
    assert log.cause_counts() == {"ground": 2, "out_of_bounds": 2, "gate": 2, "time_limit": 1}
    assert log.by_gate(4).tolist() == [[0, 0, 0, 2], [0, 1, 0, 1], [2, 0, 0, 0], [0, 1, 0, 0]]            # rows: ground, out of bounds, gate, time limit
    assert log.by_gate().shape == (4, 4) and log.terminal_state is None
    assert log.cause.tolist() == st[:, 3].tolist() and log.valid.tolist() == [4, 3, 4, 4, 1, 2]
    none = CrashLog(ring, np.zeros((M, 4), np.int32), None, 11, 0.01)
    assert none.cause_counts() == {"ground": 0, "out_of_bounds": 0, "gate": 0, "time_limit": 0} and none.by_gate(4).sum() == 0
    assert none.flights()[0].shape == (0, W, R)
    with pytest.raises(ValueError):
        CrashLog(ring.astype(np.float64), st, None, 11, 0.01)
    with pytest.raises(ValueError):
        CrashLog(ring, st[:-1], None, 11, 0.01)
    with pytest.raises(ValueError):
        CrashLog(ring, st, np.zeros((M, S_LEN + 1), np.float32), 11, 0.01)


# ---------------------------------------------------------------------------------------------------------------------------------
# the binding and the package surface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_library_without_the_black_box_is_reported_by_symbol_name():
    from optimal_quad_control_rl_amd import _lib
    from optimal_quad_control_rl_amd.vec_env import Quadcopter3DGates

    class Old:   # a library built from older sources: no such attribute
        pass

    env = Quadcopter3DGates.__new__(Quadcopter3DGates)   # the binding asks for the symbol before it touches anything else
    env._L = Old()
    env._h = None                                        # (nothing to release)
    with pytest.raises(_lib.QuadraceError, match="qr_blackbox_policy"):
        env.blackbox_policy_device(None, 8, np.zeros(4, np.float32))


def test_package_exports_the_black_box_lazily():
    import optimal_quad_control_rl_amd as pkg
    from optimal_quad_control_rl_amd import blackbox
    from optimal_quad_control_rl_amd.vec_env import Quadcopter3DGates

    assert pkg.blackbox_policy is blackbox.blackbox_policy and pkg.CrashLog is blackbox.CrashLog
    assert "blackbox_policy" in pkg.__all__ and "CrashLog" in pkg.__all__
    assert callable(Quadcopter3DGates.blackbox_policy_device) and Quadcopter3DGates.BLACKBOX_ST_INTS == blackbox.ST_INTS == 4
    assert blackbox.TRIGGERS == {"none": 0, "crash": 1, "time_limit": 2, "any": 3}
    with pytest.raises(ValueError, match="trigger"):
        blackbox.blackbox_policy(None, None, 10, trigger="sometimes")


def test_the_black_box_code_object_is_its_own_and_linted():
    from optimal_quad_control_rl_amd import build, isa_lint

    lib = build.build_native_locked()
    blobs = list(isa_lint.code_objects(lib))
    mine = [b for b in blobs if b"blackbox_policy_kernel" in b]
    assert len(mine) == 1 and b"record_policy_kernel" not in mine[0]                                       # a translation unit of its own
    assert isa_lint.lint_library(lib, {}) == []
