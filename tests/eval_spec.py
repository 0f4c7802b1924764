"""Plain NumPy restatement of the lap / crash accounting of the on-device evaluator (qr_evaluate_policy, csrc/quadrace_eval.hip;
record layout in include/quadrace.h).  Test infrastructure: the GPU tests drive a per-step loop through the C ABI, feed what that loop
observes from outside -- the target gate before and after every step, done, trunc, reward -- through `step()` below and demand that the
kernel's records are EQUAL.  All times are integer step counts, so the integer record has no rounding at all; the float record is three
sequential float32 sums (one add per step; one multiply and two adds per finished episode), reproduced here operation by operation.

Record of an env, 24 int32:
    0 gate passes counted        1 crashes (done and not trunc)      2 time-limit ends (trunc)
    3 passes since its last (re)start     4 step index of its last lap boundary or (re)start     5 steps evaluated so far
    6..13 sum of lap durations (steps), lap 1..8 since a (re)start       14..21 number of laps counted, lap 1..8       22, 23 zero
and 4 float32: return of the running episode, sum of finished episodes' returns, sum of their squares, zero.
"""
import numpy as np

REC_INTS, MAX_LAPS, REC_FLOATS = 24, 8, 4


def new_records(n):
    return np.zeros((n, REC_INTS), np.int32), np.zeros((n, REC_FLOATS), np.float32)


def step(rec, recf, target_before, target_after, done, trunc, reward, gates_per_lap):
    """One env step of every env, in place.  target_after is the target gate AFTER the step's auto-reset (what qr_get_state shows)."""
    tb, ta = np.asarray(target_before), np.asarray(target_after)
    done, trunc = np.asarray(done).astype(bool), np.asarray(trunc).astype(bool)
    rec[:, 5] += 1                                                   # 1.
    passed = ~done & (ta != tb)                                      # 2. a pass on the step that ends the episode is not counted
    rec[passed, 0] += 1                                              # 3.
    rec[passed, 3] += 1
    lap = passed & (rec[:, 3] % gates_per_lap == 0)
    j = rec[:, 3] // gates_per_lap
    for q in range(1, MAX_LAPS + 1):
        sel = lap & (j == q)
        rec[sel, 5 + q] += rec[sel, 5] - rec[sel, 4]
        rec[sel, 13 + q] += 1
    rec[lap, 4] = rec[lap, 5]                                        # (also for a ninth, tenth ... lap: the boundary moves)
    crash = done & ~trunc                                            # 4.
    rec[crash, 1] += 1
    rec[trunc, 2] += 1
    rec[done, 3] = 0
    rec[done, 4] = rec[done, 5]
    if recf is not None:
        r = np.asarray(reward, np.float32)
        with np.errstate(all="ignore"):
            recf[:, 0] = recf[:, 0] + r                              # float32 + float32, rounded once
            ep = recf[done, 0]
            recf[done, 1] = recf[done, 1] + ep
            recf[done, 2] = recf[done, 2] + ep * ep                  # the product is rounded to float32 before the add (no FMA)
        recf[done, 0] = 0.0
    return rec, recf


def run(rec, recf, target_before, target_after, done, trunc, reward, gates_per_lap):
    """K steps: every argument after recf is [K, n]."""
    for k in range(len(done)):
        step(rec, recf, target_before[k], target_after[k], done[k], trunc[k], None if reward is None else reward[k], gates_per_lap)
    return rec, recf


def nonvacuous_indi(rec):
    """The straight-track INDI scenario exercises every part of the record (conditions, not numbers)."""
    n = rec.shape[0]
    with_lap = int((rec[:, 14:22].sum(axis=1) > 0).sum())
    return dict(ok=with_lap >= 0.10 * n and bool((rec[:, 14:22].sum(axis=0) > 0).all()) and rec[:, 1].sum() >= 1 and rec[:, 2].sum() >= 1,
                envs_with_lap=with_lap, lap_slots=rec[:, 14:22].sum(axis=0).tolist(), crashes=int(rec[:, 1].sum()), timeouts=int(rec[:, 2].sum()))


def nonvacuous_e2e(rec):
    """The straight-track E2E scenario with gates_per_lap = 1."""
    n = rec.shape[0]
    with_pass = int((rec[:, 0] > 0).sum())
    slots = rec[:, 14:22].sum(axis=0)
    return dict(ok=with_pass >= 0.10 * n and int((slots > 0).sum()) >= 2 and rec[:, 1].sum() >= 1,
                envs_with_pass=with_pass, lap_slots=slots.tolist(), crashes=int(rec[:, 1].sum()))


# the scenario of the GPU comparison (tests/test_gpu_evaluate.py), checked for non-vacuity on the CPU oracle in tests/test_eval_spec.py
SCENARIO = dict(num_gates=16, gate_dx=0.4, gate_z=-1.5, start=(-1.0, 0.0, -1.5), gates_ahead=1, max_steps=250, steps=600, seed=5, envs=2048,
                indi_action=(0.0, -0.15, 0.0, 0.3), indi_gates_per_lap=2, e2e_action=(0.4, 0.4, 0.4, 0.4), e2e_gates_per_lap=1)


def scenario_track():
    g = SCENARIO["num_gates"]
    pos = np.stack([SCENARIO["gate_dx"] * np.arange(g), np.zeros(g), np.full(g, SCENARIO["gate_z"])], axis=1).astype(np.float32)
    return pos, np.zeros(g, np.float32), np.asarray(SCENARIO["start"], np.float32)
