"""The shared host code of the closed-loop launches (optimal_quad_control_rl_amd/_closed_loop.py), without a GPU: the argument helpers
of the env methods, the reading of a model's precision, and -- with a fake env and a fake launch -- the step loop of the banked
evaluators, whose ordering rules (seed -> reset -> share per batch, fresh records per batch, the window summarised before the second
launch, padded slots never summarised) are pinned here."""
import types

import numpy as np
import pytest
import torch

from optimal_quad_control_rl_amd import _closed_loop as cl
from optimal_quad_control_rl_amd import evaluation


@pytest.mark.parametrize("make", [lambda v: torch.tensor(v, dtype=torch.float32), lambda v: list(v), lambda v: np.array(v, dtype=np.float64),
                                  lambda v: np.array([v], dtype=np.float64), lambda v: torch.nn.Parameter(torch.tensor(v, dtype=torch.float64))],
                         ids=["tensor", "list", "f64[4]", "f64[1,4]", "parameter"])
def test_log_std_array(make):
    values = [-0.5, 0.25, 0.0, 1.5]
    a = cl.log_std_array(make(values))
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (4,) and a.flags["C_CONTIGUOUS"]
    assert np.array_equal(a, np.array(values, dtype=np.float32))
    cl._f32p(a)   # what the callers do with it


@pytest.mark.parametrize("bad", [[0.0] * 3, np.zeros((2, 4)), torch.zeros(5)])
def test_log_std_array_refuses_a_wrong_size(bad):
    with pytest.raises(ValueError):
        cl.log_std_array(bad)


def test_precision_rule():
    ns = types.SimpleNamespace
    assert cl._model_precision(None) == cl._model_precision(ns()) == cl._model_precision([]) == "f16-operands"
    assert cl._model_precision(ns(precision="f16-operands", policy_forward="torch")) == "f16-operands"
    for m in (ns(precision="f32"), ns(precision="f32-collect"), ns(policy_forward="f32class"), ns(precision="f16-operands", policy_forward="f32class")):
        assert cl._model_precision(m) == cl._model_precision([m]) == "f32"
        assert cl._model_precision([None, ns(), m, None]) == "f32"
    assert cl._model_precision([None, ns(), None]) == "f16-operands"
    assert evaluation._model_precision is cl._model_precision and evaluation._actor is cl._actor   # tools/ import them from there
    assert cl._precision_flags("f16-operands") == 0 and cl._precision_flags("f32") == 2
    with pytest.raises(ValueError):
        cl._precision_flags("f64")


def test_model_readers():
    pi = torch.nn.Sequential(torch.nn.Linear(3, 4))
    net = types.SimpleNamespace(pi=pi, log_std=torch.nn.Parameter(torch.full((4,), -0.5)))
    native = types.SimpleNamespace(_net=net)                                                  # ppo.PPO
    sb3 = types.SimpleNamespace(policy=types.SimpleNamespace(net=net))                        # sb3.PPO: policy.net is the ActorCritic
    for model in (native, sb3):
        assert cl._actor(model) is pi and cl._as_actor(model) == (pi, model)
        ls = cl.model_log_std(model)
        assert not ls.requires_grad and torch.equal(ls, torch.full((4,), -0.5))
    assert cl._as_actor(pi) == (pi, None)                                                     # a bare actor has no owner ...
    assert torch.equal(cl.model_log_std(None), torch.zeros(4))                                # ... and no log_std
    assert torch.equal(cl.model_log_std(types.SimpleNamespace(_net=types.SimpleNamespace(pi=pi))), torch.zeros(4))


def test_rollout_outputs():
    out = cl.rollout_outputs(5, 7, 20, "cpu")
    assert [tuple(t.shape) for t in out] == [(5, 7, 20), (5, 7, 4), (5, 7), (5, 7), (5, 7), (5, 7)]
    assert [t.dtype for t in out] == [torch.float32] * 4 + [torch.uint8] * 2
    assert all(t.device.type == "cpu" and t.is_contiguous() for t in out)
    assert len({t.data_ptr() for t in out}) == 6
    rec, recf = cl.zero_records(6, (24, 4), "cpu")
    assert rec.dtype == torch.int32 and tuple(rec.shape) == (6, 24) and recf.dtype == torch.float32 and tuple(recf.shape) == (6, 4)
    assert not rec.any() and not recf.any()


@pytest.mark.parametrize("exc", [AssertionError, ValueError])
def test_check_records_raises_the_callers_exception(exc):
    rec, recf = cl.zero_records(6, (12, 4), "cpu")      # right shapes, but not on a GPU
    for args in ((rec, recf), (rec, None), (None, recf), (np.zeros((6, 12), np.int32), None)):
        with pytest.raises(exc, match="rec"):
            cl.check_records(*args, 6, (12, 4), exc)


def test_group_size():
    assert cl.group_size(256, 1024, "envs_per_policy", "policy") == (256, 4) and cl.group_size(512, 512, "envs_per_cell", "cell") == (512, 1)
    for e in (0, 128, 384, -256):
        with pytest.raises(ValueError, match="envs_per_cell must be a multiple of 256 .*one cell"):
            cl.group_size(e, 1024, "envs_per_cell", "cell")
    with pytest.raises(ValueError, match="multiple of envs_per_policy"):
        cl.group_size(768, 1024, "envs_per_policy", "policy")


E, SLOTS = 4, 2          # the driver only slices by E: the fakes need no multiple of 256


def _drive(phases):
    """3 policies on 2 slots through fly_batches with a fake env (records its calls) and a fake launch (adds the phase's step count to
    column 0 of every row of `rec`, and 10 x slot + policy to column 1, so a summary shows which launches it saw and whose rows)."""
    log, seen = [], []
    env = types.SimpleNamespace(seed=lambda s: log.append(("seed", s)), reset_device=lambda: log.append(("reset_device",)),
                                share_starts=lambda e: log.append(("share_starts", e)))
    bank = types.SimpleNamespace(load_torch=lambda slot, actor: log.append(("load", slot, actor)))
    actors = [("actor0", None), ("actor1", None), ("actor2", None)]
    plan = evaluation.plan_policy_batches(3, SLOTS)
    assert plan == [([0, 1], 2), ([2, 2], 1)]

    def launch(indices, steps, rec, recf):
        log.append(("launch", tuple(indices), steps))
        seen.append((rec.data_ptr(), int(rec[:, 0].max()), float(recf.abs().max())))
        rec[:, 0] += steps
        recf[:, 0] += 0.5 * steps
        for slot, idx in enumerate(indices):
            rec[slot * E:(slot + 1) * E, 1] = 10 * slot + idx

    def summarise(idx, rec, recf):
        assert tuple(rec.shape) == (E, 5) and tuple(recf.shape) == (E, 3) and rec.dtype == torch.int32 and recf.dtype == torch.float32
        log.append(("summarise", idx))
        return dict(policy=idx, steps=rec[:, 0].tolist(), who=rec[:, 1].tolist(), fsum=float(recf[:, 0].sum()))

    out = cl.fly_batches(plan, evaluation._shared_starts(env, bank, actors, E, 7), launch, phases, (5, 3), summarise, SLOTS * E, E, "cpu")
    return out, log, seen


def test_fly_batches_two_phases():
    out, log, seen = _drive([30, 12])
    start = lambda a, b: [("load", 0, a), ("load", 1, b), ("seed", 7), ("reset_device",), ("share_starts", E)]
    assert log == (start("actor0", "actor1")
                   + [("launch", (0, 1), 30), ("summarise", 0), ("summarise", 1), ("launch", (0, 1), 12), ("summarise", 0), ("summarise", 1)]
                   + start("actor2", "actor2")
                   + [("launch", (2, 2), 30), ("summarise", 2), ("launch", (2, 2), 12), ("summarise", 2)])
    # records: zero at the first launch of EVERY batch, the same tensors (30 steps in) at the second
    assert [s[1:] for s in seen] == [(0, 0.0), (30, 15.0), (0, 0.0), (30, 15.0)]
    assert seen[0][0] == seen[1][0] and seen[2][0] == seen[3][0]
    # the window summary saw the first phase only, the total both; every kept group its own rows; the padded slot gave nothing
    assert [idx for idx, _ in out] == [0, 1, 2]
    for idx, (window, total) in out:
        slot = idx % SLOTS
        assert window == dict(policy=idx, steps=[30] * E, who=[10 * slot + idx] * E, fsum=15.0 * E)
        assert total == dict(policy=idx, steps=[42] * E, who=[10 * slot + idx] * E, fsum=21.0 * E)


def test_fly_batches_one_phase():
    out, log, seen = _drive([25])
    start = lambda a, b: [("load", 0, a), ("load", 1, b), ("seed", 7), ("reset_device",), ("share_starts", E)]
    assert log == (start("actor0", "actor1") + [("launch", (0, 1), 25), ("summarise", 0), ("summarise", 1)]
                   + start("actor2", "actor2") + [("launch", (2, 2), 25), ("summarise", 2)])
    assert [s[1:] for s in seen] == [(0, 0.0), (0, 0.0)]
    assert [(idx, len(s), s[0]["steps"], s[0]["who"]) for idx, s in out] == [(0, 1, [25] * E, [0] * E), (1, 1, [25] * E, [11] * E), (2, 1, [25] * E, [2] * E)]


def test_phases_and_window_total():
    assert evaluation._phases(2000, 1200) == [1200, 800] and evaluation._phases(64, 64) == [64] and evaluation._phases(2, 1) == [1, 1]
    for n, w in ((10, 0), (10, 11), (0, 0)):
        with pytest.raises(ValueError, match="window_steps"):
            evaluation._phases(n, w)
    one = dict(crashes_per_env=0.5, gates_per_env=3.0, lap_seconds=[1.0, None])
    for summaries in ([one], [one, dict(one, gates_per_env=4.0)]):
        r = evaluation._window_total(summaries)
        assert r["total"] is summaries[-1] and "crashes_per_window" not in r["total"]
        assert r["window"] == dict(one, crashes_per_window=0.5, gates_per_window=3.0) and r["window"]["lap_seconds"] is not one["lap_seconds"]
