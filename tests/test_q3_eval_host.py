"""No GPU: the q3 evaluators' accounting as restated in tests/q3_eval_spec.py on hand-written step tables, summarize_q3_eval on
hand-written records, the ctypes signatures (the header side is pinned in tests/abi_table.py), the stale-library error, and the
argument checks that need no device."""
import ctypes as C
import types

import numpy as np
import pytest

import q3_eval_spec as spec


def _table(kind, rows, max_steps):
    """rows: one list per step of per-env dicts (pre-step z / x, pre target and steps, post target, reward, done, trunc)."""
    K, n = len(rows), len(rows[0])
    t = dict(pre_state=np.zeros((K, n, 16), np.float64 if kind == "hover" else np.float32), pre_target=np.zeros((K, n), np.int32),
             pre_steps=np.zeros((K, n), np.int32), post_target=np.zeros((K, n), np.int32), rew=np.zeros((K, n), np.float32),
             done=np.zeros((K, n), np.uint8), trunc=np.zeros((K, n), np.uint8))
    for k, step in enumerate(rows):
        for i, r in enumerate(step):
            t["pre_state"][k, i, 0], t["pre_state"][k, i, 2] = r.get("x", 0.0), r.get("z", -1.0)
            t["pre_target"][k, i], t["pre_steps"][k, i] = r.get("tg", 0), r["steps"]
            t["post_target"][k, i] = r.get("tg2", r.get("tg", 0))
            t["rew"][k, i], t["done"][k, i], t["trunc"][k, i] = r.get("rew", 0.25), r.get("done", 0), r.get("trunc", 0)
    return dict(kind=kind, max_steps=max_steps, **t)


def _gates_rows():
    # env 0: pass at step 0, final pass (SUCCESS, length 3) at step 2, then a shorter SUCCESS (length 2), then flying
    # env 1: COLLISION, then GROUND, then OOB (pre-step x = 10.5), then TIMEOUT at max_steps = 5, then a step
    # env 2: ground AND out of bounds before the step -> GROUND wins; TIMEOUT beats ground; SUCCESS beats the time limit
    e0 = [dict(steps=0, tg=0, tg2=1, rew=0.5), dict(steps=1, tg=1, rew=0.125), dict(steps=2, tg=1, tg2=3, rew=10.0, done=1),
          dict(steps=0, tg=1, tg2=1, rew=-0.5), dict(steps=1, tg=1, tg2=0, rew=10.0, done=1), dict(steps=0, tg=0, rew=0.75)]
    e1 = [dict(steps=0, rew=-10.0, done=1), dict(steps=0, z=0.01, rew=-10.0, done=1), dict(steps=0, x=10.5, rew=0.0625, done=1),
          dict(steps=4, rew=0.1, done=1, trunc=1), dict(steps=0, rew=0.2), dict(steps=1, rew=0.3)]
    e2 = [dict(steps=0, z=0.5, x=-11.0, rew=-10.0, done=1), dict(steps=4, z=0.5, rew=-10.0, done=1, trunc=1),
          dict(steps=4, tg=1, tg2=2, rew=10.0, done=1, trunc=1), dict(steps=0, rew=0.0), dict(steps=1, rew=0.0), dict(steps=2, rew=0.0)]
    return [[e0[k], e1[k], e2[k]] for k in range(6)]


def test_gates_table_reaches_every_class():
    rec, recf = spec.evaluate(**_table("gates", _gates_rows(), 5))
    assert rec.dtype == np.int32 and recf.dtype == np.float32 and rec.shape == (3, 12) and recf.shape == (3, 4)
    #                          steps S  T  O  G  C  sumS sumAll passes best
    assert rec[0].tolist() == [6, 2, 0, 0, 0, 0, 5, 5, 1, 2, 0, 0]
    assert rec[1].tolist() == [6, 0, 1, 1, 1, 1, 0, 1 + 1 + 1 + 5, 0, 0, 0, 0]
    assert rec[2].tolist() == [6, 1, 1, 0, 1, 0, 5, 1 + 5 + 5, 0, 5, 0, 0]
    f = np.float32
    r1, r2 = f(f(f(0.5) + f(0.125)) + f(10.0)), f(f(-0.5) + f(10.0))
    assert recf[0].tolist() == [f(0.75), f(r1 + r2), f(f(r1 * r1) + f(r2 * r2)), 0.0]
    assert recf[1, 0] == f(f(0.2) + f(0.3))


def test_hover_table_and_priorities():
    # env 0: goal (SUCCESS, length 3); env 1: out of bounds before the limit (OOB), then the limit (TIMEOUT); env 2: out of bounds ON
    # the limit step counts as TIMEOUT (the step counter reached max_steps), goal on the limit step is trunc -> TIMEOUT too
    rows = [[dict(steps=2, rew=100.0, done=1), dict(steps=1, rew=-1.0, done=1, trunc=1), dict(steps=3, rew=-1.0, done=1, trunc=1)],
            [dict(steps=0, rew=-0.01), dict(steps=3, rew=-0.02, done=1, trunc=1), dict(steps=3, rew=100.0, done=1, trunc=1)]]
    rec, recf = spec.evaluate(**_table("hover", rows, 4))
    assert rec[0].tolist() == [2, 1, 0, 0, 0, 0, 3, 3, 0, 3, 0, 0]
    assert rec[1].tolist() == [2, 0, 1, 1, 0, 0, 0, 2 + 4, 0, 0, 0, 0]
    assert rec[2].tolist() == [2, 0, 2, 0, 0, 0, 0, 8, 0, 0, 0, 0]
    assert recf[0].tolist() == [np.float32(-0.01), 100.0, 10000.0, 0.0]


@pytest.mark.parametrize("kind", ["hover", "gates"])
def test_continuation(kind):
    rows = _gates_rows()
    if kind == "hover":
        rows = [[dict(steps=k % 4, rew=float(k) - 2.5, done=int(k % 4 == 3 or k == 1), trunc=int(k % 4 == 3)) for _ in range(2)] for k in range(6)]
    t = _table(kind, rows, 5 if kind == "gates" else 4)
    whole = spec.evaluate(**t)
    for a in (1, 2, 5):
        cut = lambda s: {k: (v[s] if isinstance(v, np.ndarray) else v) for k, v in t.items()}
        r1, f1 = spec.evaluate(**cut(slice(0, a)))
        r2, f2 = spec.evaluate(rec=r1, recf=f1, **cut(slice(a, None)))
        assert np.array_equal(r2, whole[0]) and np.array_equal(f2.view(np.uint32), whole[1].view(np.uint32)), a


def test_spec_refuses_a_shaped_reward_that_could_meet_the_equality():
    rows = [[dict(steps=0, rew=7.5)]]
    with pytest.raises(AssertionError):
        spec.evaluate(**_table("gates", rows, 5))


def test_summarize_q3_eval():
    from optimal_quad_control_rl_amd import evaluation as ev

    assert (ev.Q3_REC_INTS, ev.Q3_REC_FLOATS) == (12, 4) == (spec.REC_INTS, spec.REC_FLOATS)
    rec = np.array([[50, 2, 1, 0, 0, 1, 30, 70, 5, 12, 0, 0],
                    [50, 1, 0, 1, 1, 1, 10, 40, 2, 10, 0, 0],
                    [50, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0]], np.int32)
    recf = np.array([[0.5, 8.0, 40.0, 0], [0.0, 4.0, 24.0, 0], [1.5, 0, 0, 0]], np.float32)
    s = ev.summarize_q3_eval(rec, recf, 0.01)
    assert s["envs"] == 3 and s["steps"] == 50 and s["episodes"] == 8
    assert (s["successes"], s["timeouts"], s["out_of_bounds"], s["ground"], s["collisions"]) == (3, 1, 1, 1, 2)
    assert s["success_rate"] == 3 / 8
    assert s["mean_success_seconds"] == pytest.approx(40 * 0.01 / 3) and s["best_success_seconds"] == pytest.approx(0.10)
    assert s["mean_episode_seconds"] == pytest.approx(110 * 0.01 / 8)
    assert s["gates_per_episode"] == pytest.approx((8 + 3) / 8)
    assert s["mean_reward"] == pytest.approx(12.0 / 8) and s["std_reward"] == pytest.approx(np.sqrt(64.0 / 8 - 1.5 ** 2))
    assert set(s) == {"envs", "steps", "episodes", "successes", "timeouts", "out_of_bounds", "ground", "collisions", "success_rate",
                      "mean_success_seconds", "best_success_seconds", "mean_episode_seconds", "gates_per_episode", "mean_reward", "std_reward"}
    # no recf; episodes without a success; no episode at all
    assert ev.summarize_q3_eval(rec, None, 0.01)["mean_reward"] is None
    t = ev.summarize_q3_eval(np.array([[9, 0, 2, 1, 0, 0, 0, 20, 0, 0, 0, 0]], np.int32), np.zeros((1, 4), np.float32), 0.01)
    assert t["success_rate"] == 0.0 and t["mean_success_seconds"] is None and t["best_success_seconds"] is None
    assert t["mean_episode_seconds"] == pytest.approx(20 * 0.01 / 3) and t["gates_per_episode"] == 0.0 and t["mean_reward"] == 0.0
    e = ev.summarize_q3_eval(np.zeros((4, 12), np.int32), np.zeros((4, 4), np.float32), 0.01)
    assert e["envs"] == 4 and e["episodes"] == 0 and e["steps"] == 0
    for k in ("success_rate", "mean_success_seconds", "best_success_seconds", "mean_episode_seconds", "gates_per_episode", "mean_reward", "std_reward"):
        assert e[k] is None, k
    with pytest.raises(AssertionError):
        ev.summarize_q3_eval(np.zeros((4, 24), np.int32), None, 0.01)


def test_signatures_and_exports():
    import optimal_quad_control_rl_amd as pkg
    from optimal_quad_control_rl_amd import _lib, evaluation

    vp, i32 = C.c_void_p, C.c_int32
    assert _lib.SIGNATURES["q3_evaluate_policy"] == (C.c_int, [vp, vp, i32, i32, vp, vp, vp])
    assert _lib.SIGNATURES["q3_evaluate_policy_bank"] == (C.c_int, [vp, vp, i32, i32, i32, i32, vp, vp, vp])
    assert "q3_evaluate_policy" in _lib.OPTIONAL_SYMBOLS and "q3_evaluate_policy_bank" in _lib.OPTIONAL_SYMBOLS
    for name in ("evaluate_q3_policy", "evaluate_q3_policies", "summarize_q3_eval"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(evaluation, name), name


@pytest.mark.parametrize("name", ["q3_evaluate_policy", "q3_evaluate_policy_bank"])
def test_stale_library_error_names_the_symbol(name):
    from optimal_quad_control_rl_amd import _lib

    stale = types.SimpleNamespace(q3_rollout_policy=lambda *a: 0)      # a library built before the evaluators existed
    with pytest.raises(_lib.QuadraceError) as e:
        _lib.require(stale, name)
    assert name in str(e.value) and "rebuild" in str(e.value) and e.value.code == _lib.QR_E_STATE
    assert _lib.require(stale, "q3_rollout_policy") is stale.q3_rollout_policy


def test_evaluate_q3_policies_argument_checks():
    from optimal_quad_control_rl_amd import evaluation as ev

    env = types.SimpleNamespace(num_envs=1024)
    wrapped = types.SimpleNamespace(venv=env)
    for kw in (dict(envs_per_policy=0), dict(envs_per_policy=128), dict(envs_per_policy=384), dict(envs_per_policy=-256)):
        with pytest.raises(ValueError, match="multiple of 256"):
            ev.evaluate_q3_policies([object()], env, **kw)
    with pytest.raises(ValueError, match="multiple of envs_per_policy"):
        ev.evaluate_q3_policies([object()], wrapped, envs_per_policy=768)
    with pytest.raises(ValueError, match="multiple of envs_per_policy"):
        ev.evaluate_q3_policies([object()], types.SimpleNamespace(num_envs=256), envs_per_policy=512)
    with pytest.raises(ValueError, match="n_eval_steps"):
        ev.evaluate_q3_policies([object()], env, n_eval_steps=0)
    with pytest.raises(ValueError, match="at least one policy"):
        ev.evaluate_q3_policies([], env)
