"""CPU: the condition bank and the grid evaluation in the package (the C entry points are pinned in tests/abi_table.py); the batching arithmetic of evaluate_grid is a pure function; Condition / disturbance_sweep / robustness_table and the
argument handling of tools/robustness_sweep.py work on hand-made data."""
import importlib.util
import os
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def test_package_exports_the_grid_names_lazily():
    import optimal_quad_control_rl_amd as pkg
    from optimal_quad_control_rl_amd import conditions, evaluation
    from optimal_quad_control_rl_amd.vec_env import Quadcopter3DGates

    assert pkg.evaluate_grid is evaluation.evaluate_grid
    assert pkg.Condition is conditions.Condition and pkg.ConditionBank is conditions.ConditionBank
    assert pkg.disturbance_sweep is conditions.disturbance_sweep
    for name in ("evaluate_grid", "Condition", "ConditionBank", "disturbance_sweep"):
        assert name in pkg.__all__, name
    assert callable(Quadcopter3DGates.evaluate_grid_device) and callable(Quadcopter3DGates.condition_starts)
    for m in ("set", "close"):
        assert callable(getattr(conditions.ConditionBank, m))
    assert callable(evaluation.plan_grid_batches) and callable(evaluation.robustness_table)


def test_plan_grid_batches_visits_every_cell_once_and_pads_with_a_real_cell():
    from optimal_quad_control_rl_amd.evaluation import plan_grid_batches

    assert plan_grid_batches(1, 1, 1) == [([(0, 0)], 1)]
    assert plan_grid_batches(2, 3, 6) == [([(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)], 6)]
    assert plan_grid_batches(2, 3, 4) == [([(0, 0), (0, 1), (0, 2), (1, 0)], 4), ([(1, 1), (1, 2), (1, 2), (1, 2)], 2)]
    assert plan_grid_batches(1, 3, 8) == [([(0, 0), (0, 1), (0, 2)] + [(0, 2)] * 5, 3)]
    assert plan_grid_batches(3, 1, 1) == [([(p, 0)], 1) for p in range(3)]
    for P, Cn, slots in ((7, 10, 256), (5, 3, 4), (1, 17, 16), (16, 16, 256), (3, 5, 15), (13, 1, 4)):
        plan = plan_grid_batches(P, Cn, slots)
        assert len(plan) == -(-(P * Cn) // slots)
        assert all(len(cells) == slots and 1 <= kept <= slots for cells, kept in plan)
        assert all(kept == slots for _, kept in plan[:-1])                                   # only the last launch is padded
        kept_all = [cell for cells, kept in plan for cell in cells[:kept]]
        assert kept_all == [(p, c) for p in range(P) for c in range(Cn)]                     # every cell exactly once, policy-major
        assert all(cell == cells[kept - 1] for cells, kept in plan for cell in cells[kept:])  # the padding repeats a real cell of that launch
    for bad in ((0, 3, 4), (3, 0, 4), (3, 3, 0), (-1, 3, 4)):
        with pytest.raises(ValueError):
            plan_grid_batches(*bad)


def _fake_env(variant=0):
    gp = np.array([[0, 0, -1.5], [1, 0, -1.5], [2, 1, -1.5]], dtype=np.float32)
    return types.SimpleNamespace(VARIANT=variant, gate_pos=gp, gate_yaw=np.array([0.0, 0.1, 0.2], np.float32), num_gates=3,
                                 start_pos=np.array([-1.0, 0.0, -1.5], np.float32),
                                 disturbance_ranges=np.array([[-0.03, 0.03]] * 6), disturbance_scale=1, max_steps=1200)


def test_condition_from_env_copies_and_never_aliases():
    from optimal_quad_control_rl_amd.conditions import Condition

    env = _fake_env()
    c = Condition.from_env(env)
    assert c.name == "env" and c.num_gates == 3 and c.max_steps == 1200 and c.gates_per_lap == 3 and c.disturbance_scale == 1.0
    for a, b in ((c.gate_pos, env.gate_pos), (c.gate_yaw, env.gate_yaw), (c.start_pos, env.start_pos), (c.disturbance_ranges, env.disturbance_ranges)):
        assert a.dtype == np.float32 and np.array_equal(a, b.astype(np.float32)) and not np.shares_memory(a, b)
    env.gate_pos[0, 0] = 9.0; env.gate_yaw[1] = 9.0; env.start_pos[2] = 9.0; env.disturbance_ranges[0, 0] = 9.0
    assert c.gate_pos[0, 0] == 0.0 and c.gate_yaw[1] == np.float32(0.1) and c.start_pos[2] == -1.5 and c.disturbance_ranges[0, 0] == np.float32(-0.03)
    # overrides replace fields by name; a track that lists its gates twice has half the lap length; the caller's arrays are copied too
    twice = np.concatenate([env.gate_pos, env.gate_pos])
    d = Condition.from_env(env, name="twice", gate_pos=twice, gate_yaw=np.concatenate([env.gate_yaw, env.gate_yaw]), max_steps=77)
    assert d.name == "twice" and d.num_gates == 6 and d.gates_per_lap == 3 and d.max_steps == 77 and not np.shares_memory(d.gate_pos, twice)
    assert Condition.from_env(env, gates_per_lap=5).gates_per_lap == 5
    # an INDI env has no disturbances
    i = Condition.from_env(_fake_env(variant=1))
    assert i.disturbance_ranges is None and i.disturbance_scale == 1.0
    with pytest.raises(ValueError):
        Condition("bad", env.gate_pos, env.gate_yaw[:2], env.start_pos, None, 1.0, 10, 1)
    e = c.replace(disturbance_scale=2)
    assert e.disturbance_scale == 2.0 and c.disturbance_scale == 1.0 and np.array_equal(e.gate_pos, c.gate_pos)


def test_disturbance_sweep_varies_the_scale_only():
    from optimal_quad_control_rl_amd.conditions import disturbance_sweep

    env = _fake_env()
    env.max_steps = 500
    scales = [0, 0.5, 1, 2, 3]
    conds = disturbance_sweep(env, scales)
    assert [c.disturbance_scale for c in conds] == [float(s) for s in scales]
    assert [c.name for c in conds] == ["scale=0", "scale=0.5", "scale=1", "scale=2", "scale=3"]
    for c in conds:
        assert np.array_equal(c.gate_pos, conds[0].gate_pos) and np.array_equal(c.gate_yaw, conds[0].gate_yaw)
        assert np.array_equal(c.start_pos, conds[0].start_pos) and np.array_equal(c.disturbance_ranges, conds[0].disturbance_ranges)
        assert c.max_steps == 500 and c.gates_per_lap == 3
    assert env.disturbance_scale == 1                      # the env itself is not touched
    assert disturbance_sweep(env, []) == []


def _result(crashes, flying, gates):
    return {"window": {"crashes_per_window": crashes, "gates_per_window": gates}, "total": {"flying_lap_seconds": flying}}


def test_robustness_table_on_hand_made_results():
    from optimal_quad_control_rl_amd.evaluation import robustness_table

    res = [[_result(0.0, 2.5, 20.0), _result(0.25, 2.75, 15.5), _result(1.5, None, 2.0)],
           [_result(0.125, 3.0, 18.0), _result(0.5, None, 9.0), _result(2.0, None, 0.0)]]
    names = ["x0", "x1", "x3"]
    t = robustness_table(res, names)
    assert t == [[("x0", 0.0, 2.5, 20.0), ("x1", 0.25, 2.75, 15.5), ("x3", 1.5, None, 2.0)],
                 [("x0", 0.125, 3.0, 18.0), ("x1", 0.5, None, 9.0), ("x3", 2.0, None, 0.0)]]
    assert robustness_table([], names) == []
    with pytest.raises(ValueError):
        robustness_table(res, names[:2])


def test_robustness_sweep_expands_arguments_and_formats(tmp_path):
    spec = importlib.util.spec_from_file_location("robustness_sweep", os.path.join(ROOT, "tools", "robustness_sweep.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.parse_scales("0,0.5,1,2,3") == [0.0, 0.5, 1.0, 2.0, 3.0] and tool.parse_scales(" 2 , 1 ") == [2.0, 1.0]
    for bad in ("", "a,1", "1,1", "-1", "inf", "nan"):
        with pytest.raises(SystemExit):
            tool.parse_scales(bad)
    assert tool.parse_tracks("square,zigzag") == ["square", "zigzag"] and tool.parse_tracks("zigzag") == ["zigzag"]
    for bad in ("", "oval", "square,square"):
        with pytest.raises(SystemExit):
            tool.parse_tracks(bad)
    assert tool.condition_grid(["square", "zigzag"], [0.0, 2.0], "e2e") == [("square", 0.0), ("square", 2.0), ("zigzag", 0.0), ("zigzag", 2.0)]
    assert tool.condition_grid(["square", "zigzag"], [0.0, 2.0], "indi") == [("square", None), ("zigzag", None)]
    assert tool.condition_name("square", 0.5) == "square x0.5" and tool.condition_name("zigzag", None) == "zigzag"
    run = tmp_path / "run"
    run.mkdir()
    for name in ("b.zip", "a.zip"):
        (run / name).write_bytes(b"")
    assert tool.expand([str(run), str(run / "a.zip")]) == [str(run / "a.zip"), str(run / "b.zip")]
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(SystemExit):
        tool.expand([str(empty)])
    text = tool.format_table("run/a.zip", [("square x1", 0.0625, 2.3456, 20.5), ("square x3", 1.5, None, 3.0)])
    lines = text.split("\n")
    assert lines[0] == "run/a.zip" and "crashes/window" in lines[1] and len(lines) == 4
    assert lines[2].split() == ["square", "x1", "0.0625", "2.346", "20.50"] and lines[3].split() == ["square", "x3", "1.5000", "-", "3.00"]
