"""CPU: the flight recorder in the package (its C entry points are pinned in tests/abi_table.py), its code object among the linted
ones, and FlightRecord turns a synthetic [K][M][R] array into what a plain NumPy restatement gives."""
import numpy as np
import pytest


def test_package_exports_the_recorder_lazily():
    import optimal_quad_control_rl_amd as pkg
    from optimal_quad_control_rl_amd import recording
    from optimal_quad_control_rl_amd.vec_env import Quadcopter3DGates

    assert pkg.record_policy is recording.record_policy and pkg.FlightRecord is recording.FlightRecord
    assert "record_policy" in pkg.__all__ and "FlightRecord" in pkg.__all__
    assert callable(Quadcopter3DGates.record_policy_device) and Quadcopter3DGates.RECORD_EXTRA == recording.RECORD_EXTRA == 8


def test_the_recorder_code_object_is_linted():
    """The lint walks every code object of the built library: the recorder's kernels are in one of them, and the library is clean."""
    from optimal_quad_control_rl_amd import build, isa_lint

    lib = build.build_native_locked()
    assert "quadrace_record.hip" in build.SOURCES
    blobs = list(isa_lint.code_objects(lib))
    with_recorder = [b for b in blobs if b"record_policy_kernel" in b]
    assert len(with_recorder) == 1 and b"eval_policy_kernel" not in with_recorder[0]       # a translation unit of its own
    stats = {}
    assert isa_lint.lint_library(lib, stats) == []
    assert stats["code_objects"] == len(blobs) >= 8


# ---------------------------------------------------------------------------------------------------------------------------------
# FlightRecord on a synthetic record: two envs, several episodes, every end code, target wraps, an open last episode
# ---------------------------------------------------------------------------------------------------------------------------------
def _synthetic(state_len):
    K, M, R = 23, 2, state_len + 8
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((K, M, R)).astype(np.float32)
    rows[:, :, state_len:state_len + 4] = rng.uniform(-1, 1, (K, M, 4)).astype(np.float32)
    rows[3, 0, state_len] = 1.0; rows[4, 0, state_len + 1] = -1.0                          # commands at the Box's edges
    # env 0: crash at row 4, time limit at row 11, crash at row 12 (a one-row episode), then open; env 1: ends on the very last row
    end = np.zeros((K, M), np.float32)
    end[4, 0], end[11, 0], end[12, 0] = 1.0, 2.0, 1.0
    end[9, 1], end[22, 1] = 2.0, 1.0
    # targets: 3 gates, wrap 2 -> 0; a change across an episode end is the reset, not a pass
    tgt = np.zeros((K, M), np.float32)
    tgt[:, 0] = [0, 0, 1, 1, 2, 0, 0, 1, 2, 0, 1, 1, 0, 0, 1, 2, 2, 0, 0, 1, 1, 2, 0]
    tgt[:, 1] = [0, 1, 2, 0, 1, 2, 0, 1, 2, 2, 0, 0, 0, 1, 1, 1, 2, 2, 0, 0, 1, 2, 0]
    steps = np.zeros((K, M), np.float32)
    for i in range(M):
        c = 5 if i else 0                                                                  # env 1 was already flying when the record began
        for k in range(K):
            steps[k, i] = c
            c = 0 if end[k, i] else c + 1
    rows[:, :, state_len + 5], rows[:, :, state_len + 6], rows[:, :, state_len + 7] = end, tgt, steps
    return rows


@pytest.mark.parametrize("state_len", [16, 13])
def test_flight_record_equals_a_numpy_restatement(state_len, tmp_path):
    from optimal_quad_control_rl_amd.recording import LOG_KEYS, FlightRecord

    rows, dt, S = _synthetic(state_len), np.float32(0.01), state_len
    fr = FlightRecord(rows, 0.01)
    K, M = rows.shape[:2]
    assert (fr.num_steps, fr.num_envs, fr.state_len) == (K, M, S)
    for view, want in ((fr.world, rows[:, :, :S]), (fr.command, rows[:, :, S:S + 4]), (fr.reward, rows[:, :, S + 4]), (fr.end, rows[:, :, S + 5]),
                       (fr.target, rows[:, :, S + 6]), (fr.steps, rows[:, :, S + 7])):
        assert view.dtype == np.float32 and np.array_equal(view, want) and np.shares_memory(view, rows)
    assert fr.t.dtype == np.float32 and np.array_equal(fr.t, rows[:, :, S + 7] * dt)
    want_counts = np.zeros((M, 3), np.int64)
    for i in range(M):
        end, tgt = rows[:, i, S + 5], rows[:, i, S + 6]
        # episodes: cut after every row that ended one
        eps, a = [], 0
        for k in range(K):
            if end[k] != 0:
                eps.append((a, k + 1)); a = k + 1
        if a < K:
            eps.append((a, K))
        assert fr.episodes(i) == eps
        passes = [k for k in range(K - 1) if end[k] == 0 and tgt[k + 1] != tgt[k]]
        assert fr.gate_passes(i).tolist() == passes and len(passes) > 0
        want_counts[i] = [len(passes), int((end == 1).sum()), int((end == 2).sum())]
    assert fr.episodes(0) == [(0, 5), (5, 12), (12, 13), (13, 23)] and fr.episodes(1) == [(0, 10), (10, 23)]   # open / closed last episode
    assert fr.gate_passes(0).tolist() == [1, 3, 6, 7, 8, 9, 13, 14, 16, 18, 20, 21]        # 4 -> 5 and 11 -> 12 -> 13 are resets, not passes
    assert np.array_equal(fr.counts(), want_counts) and fr.counts().dtype == np.int64
    assert want_counts.tolist() == [[12, 2, 1], [14, 1, 1]]
    # log_dict: exactly the reference's sixteen keys, float32 formulas bit for bit
    for i, ep in ((0, None), (0, 1), (0, 2), (1, 1), (0, 3)):
        a, b = (0, K) if ep is None else fr.episodes(i)[ep]
        d = fr.log_dict(i, ep)
        assert tuple(d) == LOG_KEYS == ("t", "x", "y", "z", "vx", "vy", "vz", "V", "phi", "theta", "psi", "u1", "u2", "u3", "u4", "u") and len(d) == 16
        w, c = rows[a:b, i, :S], rows[a:b, i, S:S + 4]
        want = {"t": rows[a:b, i, S + 7] * dt, "x": w[:, 0], "y": w[:, 1], "z": w[:, 2], "vx": w[:, 3], "vy": w[:, 4], "vz": w[:, 5],
                "V": np.sqrt(w[:, 3] ** 2 + w[:, 4] ** 2 + w[:, 5] ** 2), "phi": w[:, 6], "theta": w[:, 7], "psi": w[:, 8],
                "u1": (c[:, 0] + 1) / 2, "u2": (c[:, 1] + 1) / 2, "u3": (c[:, 2] + 1) / 2, "u4": (c[:, 3] + 1) / 2}
        want["u"] = np.stack([want["u1"], want["u2"], want["u3"], want["u4"]], axis=1)
        for k in LOG_KEYS:
            assert d[k].dtype == np.float32 and d[k].shape == want[k].shape and np.array_equal(d[k].view(np.uint32), want[k].view(np.uint32)), k
        assert d["u"].shape == (b - a, 4) and float(d["u"].min()) >= 0.0 and float(d["u"].max()) <= 1.0
        path = fr.save_npz(str(tmp_path / ("flight_%d_%s.npz" % (i, ep))), i, ep)
        with np.load(path) as z:
            assert sorted(z.files) == sorted(LOG_KEYS)
            for k in LOG_KEYS:
                assert z[k].dtype == np.float32 and np.array_equal(z[k].view(np.uint32), d[k].view(np.uint32)), k
    assert fr.log_dict(0, 2)["t"].tolist() == [0.0] and fr.log_dict(1)["t"][0] == np.float32(5) * dt
    with pytest.raises(ValueError):
        FlightRecord(rows.astype(np.float64), 0.01)
    with pytest.raises(ValueError):
        FlightRecord(rows[:, :, :-1], 0.01)
