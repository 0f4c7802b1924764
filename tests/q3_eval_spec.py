"""NumPy restatement of the q3 evaluators' accounting (q3_eval_body in csrc/quad3d.hip; record layout in include/quad3d.h), from what
the ABI already exposes per step: the state, target and step counter before each step, the target after it, and q3_step's reward /
done / trunc.  Same statements in the same order as the kernel; all times are integer step counts, so the integer record is exact, and
the float record is sequential float32 arithmetic in step order (one add per step; one multiply and two adds per finished episode).

    rec  [N, 12] int32   [0] steps  [1] SUCCESS  [2] TIMEOUT  [3] OOB  [4] GROUND  [5] COLLISION  [6] sum of SUCCESS lengths
                         [7] sum of all lengths  [8] gate passes on steps that do not end the episode  [9] shortest SUCCESS (0 = none)
                         [10], [11] 0
    recf [N, 4] float32  running return, sum of finished returns, sum of their squares, 0

End causes are exclusive, in priority order:
    hover   SUCCESS = done and not trunc; else TIMEOUT if pre_steps + 1 >= max_steps; else OOB
    gates   SUCCESS = done and reward == 10 (the final-gate override is the last one in step_wait); else TIMEOUT if trunc; else GROUND if
            the pre-step z > 0; else OOB by the reference's pre-step predicate; else COLLISION
"""
import numpy as np

REC_INTS, REC_FLOATS = 12, 4
STEPS, SUCCESS, TIMEOUT, OOB, GROUND, COLLISION, SUCCESS_LEN, ALL_LEN, PASSES, BEST = range(10)


def classify(kind, pre_state, pre_steps, rew, done, trunc, max_steps):
    """One step of N envs -> bool arrays (success, timeout, oob, ground, collision); all False where `done` is False."""
    done, trunc = np.asarray(done, bool), np.asarray(trunc, bool)
    s = np.asarray(pre_state)
    none = np.zeros(done.shape, bool)
    if kind == "hover":
        success = done & ~trunc
        timeout = done & ~success & (np.asarray(pre_steps, np.int64) + 1 >= int(max_steps))
        oob = done & ~success & ~timeout
        return success, timeout, oob, none, none.copy()
    assert kind == "gates", kind
    success = done & (np.asarray(rew, np.float32) == np.float32(10.0))
    timeout = done & ~success & trunc
    rest = done & ~success & ~timeout
    ground = rest & (s[:, 2] > 0)
    rest = rest & ~ground
    pre_oob = (np.abs(s[:, 0]) > 10) | (np.abs(s[:, 1]) > 10) | (np.abs(s[:, 9]) > 1000) | (np.abs(s[:, 10]) > 1000) | (np.abs(s[:, 11]) > 1000)
    oob = rest & pre_oob
    collision = rest & ~oob
    return success, timeout, oob, ground, collision


def evaluate(kind, pre_state, pre_target, pre_steps, post_target, rew, done, trunc, max_steps, rec=None, recf=None):
    """pre_state [K, N, 16]; pre_target, pre_steps, post_target [K, N] int; rew [K, N] float32; done, trunc [K, N]; optional starting
    records (a continued evaluation).  Returns (rec [N, 12] int32, recf [N, 4] float32)."""
    pre_state = np.asarray(pre_state)
    rew = np.asarray(rew)
    assert rew.dtype == np.float32, rew.dtype
    K, n = rew.shape
    assert pre_state.shape == (K, n, 16), pre_state.shape
    done, trunc = np.asarray(done).astype(bool), np.asarray(trunc).astype(bool)
    pre_target, pre_steps, post_target = (np.asarray(a).astype(np.int64) for a in (pre_target, pre_steps, post_target))
    for a in (done, trunc, pre_target, pre_steps, post_target):
        assert a.shape == (K, n), a.shape
    if kind == "gates":
        # a shaped reward can never meet the equality that marks the finished track: every reward that is not one of step_wait's two
        # overrides (+10 on a step that ends the episode, -10 for a collision or the ground) stays below 5 in magnitude
        override = done & ((rew == np.float32(10.0)) | (rew == np.float32(-10.0)))
        assert bool((np.abs(rew[~override]) < 5.0).all())
    r = np.zeros((n, REC_INTS), np.int64) if rec is None else np.array(rec, np.int64)
    f = np.zeros((n, REC_FLOATS), np.float32) if recf is None else np.array(recf, np.float32)
    assert r.shape == (n, REC_INTS) and f.shape == (n, REC_FLOATS)
    for k in range(K):
        success, timeout, oob, ground, collision = classify(kind, pre_state[k], pre_steps[k], rew[k], done[k], trunc[k], max_steps)
        d = done[k]
        assert np.array_equal(success | timeout | oob | ground | collision, d)
        assert int(success.sum() + timeout.sum() + oob.sum() + ground.sum() + collision.sum()) == int(d.sum())   # exclusive
        length = pre_steps[k] + 1            # the env's step counter at the end: after the increment, before the reset
        r[:, STEPS] += 1
        r[:, PASSES] += (~d & (post_target[k] != pre_target[k]))
        f[:, 0] = f[:, 0] + rew[k]           # float32 + float32, rounded once
        for col, m in ((SUCCESS, success), (TIMEOUT, timeout), (OOB, oob), (GROUND, ground), (COLLISION, collision)):
            r[:, col] += m
        r[:, ALL_LEN] += np.where(d, length, 0)
        r[:, SUCCESS_LEN] += np.where(success, length, 0)
        best = r[:, BEST]
        r[:, BEST] = np.where(success & ((best == 0) | (length < best)), length, best)
        sq = (f[:, 0] * f[:, 0]).astype(np.float32)
        f[:, 1] = np.where(d, f[:, 1] + f[:, 0], f[:, 1])
        f[:, 2] = np.where(d, f[:, 2] + sq, f[:, 2])
        f[:, 0] = np.where(d, np.float32(0.0), f[:, 0])
    assert r.max(initial=0) < 2 ** 31
    return r.astype(np.int32), f
