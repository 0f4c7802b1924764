"""CPU: the evaluation functions in the package (the C entry point is pinned in tests/abi_table.py), and summarize_eval turns a
hand-made record into the hand-computed summary."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_package_exports_the_evaluation_functions_lazily():
    import optimal_quad_control_rl_amd as pkg
    from optimal_quad_control_rl_amd import evaluation

    assert pkg.evaluate_policy is evaluation.evaluate_policy and pkg.summarize_eval is evaluation.summarize_eval
    assert "evaluate_policy" in pkg.__all__ and "summarize_eval" in pkg.__all__
    from optimal_quad_control_rl_amd.vec_env import Quadcopter3DGates

    assert callable(Quadcopter3DGates.evaluate_device)


def test_summarize_eval_on_a_hand_made_record():
    from optimal_quad_control_rl_amd.evaluation import summarize_eval

    rec = np.zeros((3, 24), np.int32)
    #            gates crash limit since  t0  steps | lap sums 1..8                  | lap counts 1..8
    rec[0] = [9, 1, 0, 5, 1900, 2000, 300, 250, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    rec[1] = [13, 0, 1, 1, 1990, 2000, 296, 504, 260, 0, 0, 0, 0, 0, 1, 2, 1, 0, 0, 0, 0, 0, 0, 0]
    rec[2] = [0, 3, 0, 0, 1500, 2000, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    recf = np.array([[1.0, 10.0, 100.0, 0.0], [2.0, 20.0, 400.0, 0.0], [0.5, -30.0, 300.0, 0.0]], np.float32)
    s = summarize_eval(rec, recf, 0.01, 4)
    assert (s["envs"], s["steps"], s["gates_per_lap"]) == (3, 2000, 4)
    assert (s["gates"], s["crashes"], s["timeouts"], s["episodes"]) == (22, 4, 1, 5)
    assert s["gates_per_env"] == 22 / 3 and s["crashes_per_env"] == 4 / 3
    assert s["laps_counted"] == [2, 3, 1, 0, 0, 0, 0, 0]
    assert s["lap_seconds"] == [596 * 0.01 / 2, 754 * 0.01 / 3, 260 * 0.01 / 1, None, None, None, None, None]
    assert s["first_lap_seconds"] == 596 * 0.01 / 2
    assert s["flying_lap_seconds"] == (754 + 260) * 0.01 / 4
    assert s["mean_reward"] == 0.0                                   # (10 + 20 - 30) / 5
    assert abs(s["std_reward"] - (800.0 / 5) ** 0.5) < 1e-12         # sqrt(sum of squares / episodes - mean^2)
    # no laps, no episodes, no float record: None where there is nothing to average
    z = summarize_eval(np.zeros((2, 24), np.int32), None, 0.01, 4)
    assert z["lap_seconds"] == [None] * 8 and z["first_lap_seconds"] is None and z["flying_lap_seconds"] is None
    assert z["mean_reward"] is None and z["std_reward"] is None and z["episodes"] == 0
    e = summarize_eval(np.zeros((0, 24), np.int32), None, 0.01, 4)   # an empty record: no division by the env count
    assert e["envs"] == 0 and e["steps"] == 0 and e["gates_per_env"] == 0.0 and e["crashes_per_env"] == 0.0 and e["lap_seconds"] == [None] * 8
    # tensors are accepted as well
    import torch

    assert summarize_eval(torch.as_tensor(rec), torch.as_tensor(recf), 0.01, 4) == s


def test_default_gates_per_lap_halves_a_repeated_gate_list():
    from types import SimpleNamespace

    from optimal_quad_control_rl_amd import square_track, zigzag_track
    from optimal_quad_control_rl_amd.evaluation import default_gates_per_lap

    def env(track):
        gp, gy, _ = track
        return SimpleNamespace(num_gates=len(gp), gate_pos=np.asarray(gp, np.float32), gate_yaw=np.asarray(gy, np.float32))

    assert default_gates_per_lap(env(square_track())) == 4          # lists its four gates twice
    z = env(zigzag_track())
    assert default_gates_per_lap(z) == z.num_gates


def test_benchmark_times_the_tools_loop_as_it_stands():
    """tools/bench_evaluate.py times a copy of evaluate() of tools/reference_recipe_run.py (the tool itself trains before it evaluates):
    the two loop bodies are the same lines, but for the step count being a variable in the copy."""
    def body(path):
        lines = open(os.path.join(ROOT, "tools", path)).read().split("\n")
        start = next(i for i, ln in enumerate(lines) if ln.strip().startswith("for k in range(") and "step_device" in lines[i + 1])
        out = []
        for ln in lines[start:]:
            if ln.strip().startswith(("laps =", "return ")):
                break
            out.append(ln.strip())
        return out

    ref, copy = body("reference_recipe_run.py"), body("bench_evaluate.py")
    assert len(ref) > 15 and ref[0] == "for k in range(2000):" and copy[0] == "for k in range(K):"
    assert ref[1:] == copy[1:]
