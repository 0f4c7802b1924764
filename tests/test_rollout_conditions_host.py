"""CPU: the closed-loop rollout across a mix of flight conditions in the package (qr_rollout_policy_conditions itself is pinned in
tests/abi_table.py); plan_condition_groups is a pure function checked on hand-made sizes; the
--train-scales / --train-tracks arguments of tools/train_ppo.py expand to the expected conditions on a stub env."""
import importlib.util
import os
import types

import numpy as np
import pytest

from abi_decl import stub_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def test_package_surface():
    import optimal_quad_control_rl_amd as pkg
    from optimal_quad_control_rl_amd import conditions
    from optimal_quad_control_rl_amd.vec_env import Quadcopter3DGates

    assert pkg.plan_condition_groups is conditions.plan_condition_groups and "plan_condition_groups" in pkg.__all__
    assert callable(Quadcopter3DGates.rollout_policy_conditions_device) and callable(Quadcopter3DGates.condition_reset)


def test_plan_condition_groups_equal_shares_and_remainder():
    from optimal_quad_control_rl_amd.conditions import plan_condition_groups as plan

    assert plan(256, 1) == [0]
    assert plan(768, 3) == [0, 1, 2]
    assert plan(1536, 3) == [0, 0, 1, 1, 2, 2]
    assert plan(65536, 4) == [c for c in range(4) for _ in range(64)]
    # 7 groups for 3 conditions: 3, 2, 2 -- the remainder goes to the lowest index; 8 groups: 3, 3, 2
    assert plan(7 * 256, 3) == [0, 0, 0, 1, 1, 2, 2]
    assert plan(8 * 256, 3) == [0, 0, 0, 1, 1, 1, 2, 2]
    # larger groups: 4 groups of 512
    assert plan(2048, 3, envs_per_group=512) == [0, 0, 1, 2]
    assert plan(2048, 3, 512, weights=None) == plan(2048, 3, 512, weights=[1, 1, 1]) == plan(2048, 3, 512, weights=[5.0, 5.0, 5.0])


def test_plan_condition_groups_weights():
    from optimal_quad_control_rl_amd.conditions import plan_condition_groups as plan

    assert plan(8 * 256, 2, weights=[3, 1]) == [0] * 6 + [1] * 2
    assert plan(8 * 256, 3, weights=[2, 1, 1]) == [0] * 4 + [1] * 2 + [2] * 2
    # quotas 3.5, 1.75, 1.75 of 7 groups -> floors 3, 1, 1, the two left over go to the largest remainders (1 and 2)
    assert plan(7 * 256, 3, weights=[2, 1, 1]) == [0] * 3 + [1] * 2 + [2] * 2
    # quotas 2.5, 2.5 of 5: the tie of the remainders goes to the lowest index
    assert plan(5 * 256, 2, weights=[1, 1]) == [0, 0, 0, 1, 1]
    for n, c, w in ((16 * 256, 3, [1, 2, 5]), (10 * 256, 4, [0.4, 0.3, 0.2, 0.1]), (256 * 256, 5, [9, 1, 1, 1, 1])):
        m = plan(n, c, weights=w)
        assert len(m) == n // 256 and m == sorted(m) and set(m) == set(range(c))
        share = [m.count(k) for k in range(c)]
        assert all(abs(s - len(m) * x / sum(w)) < 1.0 for s, x in zip(share, w))   # largest remainder: within one group of the quota


def test_plan_condition_groups_every_condition_gets_a_group_or_value_error():
    from optimal_quad_control_rl_amd.conditions import plan_condition_groups as plan

    with pytest.raises(ValueError):
        plan(2 * 256, 3)                             # fewer groups than conditions
    with pytest.raises(ValueError):
        plan(4 * 256, 2, weights=[1, 0])             # a zero weight
    with pytest.raises(ValueError):
        plan(4 * 256, 2, weights=[100, 1])           # a share that rounds to no group
    assert plan(4 * 256, 2, weights=[5, 3]) == [0, 0, 0, 1]   # quotas 2.5, 1.5: floors 2, 1, the group left over goes to the lowest index of the tie
    with pytest.raises(ValueError):
        plan(3 * 256, 3, weights=[5, 1, 1])          # quotas 2.14, 0.43, 0.43 -> 2, 1, 0: the last condition would not be flown


def test_plan_condition_groups_refuses_what_the_abi_refuses():
    from optimal_quad_control_rl_amd.conditions import plan_condition_groups as plan

    for bad in (dict(num_envs=768, num_conditions=0), dict(num_envs=0, num_conditions=1), dict(num_envs=-256, num_conditions=1),
                dict(num_envs=1000, num_conditions=2),                              # not a whole number of groups
                dict(num_envs=768, num_conditions=1, envs_per_group=128),           # below one workgroup
                dict(num_envs=768, num_conditions=1, envs_per_group=384),           # not a multiple of 256
                dict(num_envs=768, num_conditions=1, envs_per_group=0),
                dict(num_envs=1024, num_conditions=1, envs_per_group=768),          # num_groups * envs_per_group != num_envs
                dict(num_envs=256, num_conditions=1, envs_per_group=512),
                dict(num_envs=768, num_conditions=3, weights=[1, 1]),               # one weight per condition
                dict(num_envs=768, num_conditions=3, weights=[1, -1, 1]),
                dict(num_envs=768, num_conditions=3, weights=[1, float("nan"), 1]),
                dict(num_envs=768, num_conditions=3, weights=[0, 0, 0])):
        with pytest.raises(ValueError):
            plan(**bad)


def _stub_env(variant=0):
    from optimal_quad_control_rl_amd import square_track

    gp, gy, sp = square_track()
    return stub_env(0, VARIANT=variant, gate_pos=np.asarray(gp, np.float32), gate_yaw=np.asarray(gy, np.float32), num_gates=len(gy),
                    start_pos=np.asarray(sp, np.float32), disturbance_ranges=np.array([[-0.03, 0.03]] * 6), disturbance_scale=1, max_steps=1200)


def _tool():
    spec = importlib.util.spec_from_file_location("train_ppo", os.path.join(ROOT, "tools", "train_ppo.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)          # defines functions only: the run itself is main()
    return tool


def test_train_ppo_condition_arguments():
    from optimal_quad_control_rl_amd import square_track, zigzag_track
    from optimal_quad_control_rl_amd.evaluation import default_gates_per_lap

    tool = _tool()
    env = _stub_env()
    assert tool.train_conditions(env, "e2e", None, None) is None
    # --train-scales: one condition per scale, the env's own track
    conds = tool.train_conditions(env, "e2e", tool.parse_scales("0.5,1,2"), None)
    assert [c.name for c in conds] == ["scale=0.5", "scale=1", "scale=2"] and [c.disturbance_scale for c in conds] == [0.5, 1.0, 2.0]
    assert all(np.array_equal(c.gate_pos, env.gate_pos) and c.max_steps == 1200 for c in conds)
    with pytest.raises(SystemExit):
        tool.train_conditions(_stub_env(1), "indi", [1.0], None)                 # INDI has no disturbances
    # --train-tracks: one per track, with its own start and lap length
    zg, zy, zs = zigzag_track()
    sq = square_track()
    for variant, name in ((0, "e2e"), (1, "indi")):
        conds = tool.train_conditions(_stub_env(variant), name, None, tool.parse_tracks("square,zigzag"))
        assert [c.name for c in conds] == ["square", "zigzag"]
        assert np.array_equal(conds[1].gate_pos, np.asarray(zg, np.float32)) and np.array_equal(conds[1].start_pos, np.asarray(zs, np.float32))
        assert np.array_equal(conds[0].start_pos, np.asarray(sq[2], np.float32))
        assert conds[1].num_gates == len(zy) and conds[0].num_gates == len(sq[1])
        for c in conds:
            assert c.gates_per_lap == default_gates_per_lap(types.SimpleNamespace(num_gates=c.num_gates, gate_pos=c.gate_pos, gate_yaw=c.gate_yaw))
        assert conds[0].gates_per_lap == 4                                       # square_track() lists its four gates twice
        assert all((c.disturbance_ranges is None) == (variant == 1) for c in conds)
    # both: the product, track-major
    conds = tool.train_conditions(env, "e2e", [0.5, 2.0], ["zigzag", "square"])
    assert [c.name for c in conds] == ["zigzag x0.5", "zigzag x2", "square x0.5", "square x2"]
    assert [c.disturbance_scale for c in conds] == [0.5, 2.0, 0.5, 2.0]
    assert conds[0].num_gates == len(zy) and conds[2].num_gates == len(sq[1])
    with pytest.raises(SystemExit):
        tool.parse_tracks("oval")
    text = tool.format_condition_stats([dict(name="scale=2", episodes=3, mean_return=1.5, mean_length=200.0, crashes=2, time_limits=1)])
    assert text.split() == ["scale=2", "episodes", "3", "ep_rew", "1.50", "ep_len", "200.0", "crashes", "2", "time", "limits", "1"]
