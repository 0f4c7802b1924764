"""CPU: the policy bank and its evaluation in the package (the C entry points are pinned in tests/abi_table.py); rank_policies orders hand-made results as documented; the batching arithmetic of evaluate_policies is a pure function."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def test_package_exports_the_bank_names_lazily():
    import optimal_quad_control_rl_amd as pkg
    from optimal_quad_control_rl_amd import evaluation, policy
    from optimal_quad_control_rl_amd.vec_env import Quadcopter3DGates

    assert pkg.evaluate_policies is evaluation.evaluate_policies and pkg.rank_policies is evaluation.rank_policies
    assert pkg.MfmaPolicyBank is policy.MfmaPolicyBank
    for name in ("evaluate_policies", "rank_policies", "MfmaPolicyBank"):
        assert name in pkg.__all__, name
    assert callable(Quadcopter3DGates.evaluate_bank_device) and callable(Quadcopter3DGates.share_starts)
    for m in ("set_weights", "load_torch", "close"):
        assert callable(getattr(policy.MfmaPolicyBank, m))


def _result(crashes_per_window, flying):
    return {"window": {"crashes_per_window": crashes_per_window}, "total": {"flying_lap_seconds": flying}}


def test_rank_policies_orders_hand_made_results():
    from optimal_quad_control_rl_amd.evaluation import rank_policies

    over = _result(0.5, 1.0)       # the fastest lap of all, but over the crash bound
    no_lap = _result(0.0, None)    # never crashes, never completes a flying lap
    slow = _result(0.05, 3.0)      # clean, slow
    fast = _result(0.1, 2.0)       # clean (exactly at the bound), fast
    assert rank_policies([over, no_lap, slow, fast]) == [3, 2, 1, 0]
    # the unranked tail is ordered by crash rate, whatever the reason it is unranked
    assert rank_policies([_result(0.9, None), _result(0.3, 1.0), _result(0.6, None), fast]) == [3, 1, 2, 0]
    # the bound is an argument: at 1.0 the crashing-but-fast policy wins
    assert rank_policies([over, no_lap, slow, fast], max_crashes_per_window=1.0) == [0, 3, 2, 1]
    # ties keep the list order; the result is always a permutation
    assert rank_policies([fast, dict(fast), slow]) == [0, 1, 2]
    assert rank_policies([]) == []


def test_plan_policy_batches_slices_and_pads():
    from optimal_quad_control_rl_amd.evaluation import plan_policy_batches

    assert plan_policy_batches(1, 1) == [([0], 1)]
    assert plan_policy_batches(4, 4) == [([0, 1, 2, 3], 4)]
    assert plan_policy_batches(3, 4) == [([0, 1, 2, 2], 3)]                       # padded by repeating a policy
    assert plan_policy_batches(9, 4) == [([0, 1, 2, 3], 4), ([4, 5, 6, 7], 4), ([8, 8, 8, 8], 1)]
    assert plan_policy_batches(5, 1) == [([i], 1) for i in range(5)]
    for num, slots in ((1027, 256), (10, 16), (17, 16), (256, 256)):
        plan = plan_policy_batches(num, slots)
        assert len(plan) == -(-num // slots)
        assert all(len(idx) == slots and 1 <= kept <= slots for idx, kept in plan)
        kept_all = [i for idx, kept in plan for i in idx[:kept]]
        assert kept_all == list(range(num))                                        # every policy exactly once, in order
        assert all(i == idx[kept - 1] for idx, kept in plan for i in idx[kept:])   # the padding repeats a policy of that batch
    with pytest.raises(ValueError):
        plan_policy_batches(0, 4)
    with pytest.raises(ValueError):
        plan_policy_batches(3, 0)


def test_rank_checkpoints_finds_and_orders_checkpoints(tmp_path):
    """tools/rank_checkpoints.py: a directory stands for its *.zip files, timesteps come from the checkpoint's `data` member."""
    import importlib.util
    import json
    import zipfile

    spec = importlib.util.spec_from_file_location("rank_checkpoints", os.path.join(ROOT, "tools", "rank_checkpoints.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    run = tmp_path / "run"
    run.mkdir()
    for name, steps in (("model_b.zip", 200), ("model_a.zip", 3000)):
        with zipfile.ZipFile(run / name, "w") as z:
            z.writestr("data", json.dumps({"num_timesteps": steps}))
    (run / "notes.txt").write_text("not a checkpoint")
    extra = tmp_path / "other.zip"
    with zipfile.ZipFile(extra, "w") as z:
        z.writestr("data", json.dumps({}))
    paths = tool.expand([str(run), str(extra), str(run / "model_a.zip")])
    assert paths == [str(run / "model_a.zip"), str(run / "model_b.zip"), str(extra)]      # no duplicate, directory expanded by name
    assert [tool.timesteps_of(p) for p in paths] == [3000, 200, 0]
    assert tool.fmt(None).strip() == "-" and tool.fmt(1.23456) == "1.235"
    with pytest.raises(SystemExit):
        tool.expand([str(_empty_dir(tmp_path))])


def _empty_dir(tmp_path):
    d = tmp_path / "empty"
    d.mkdir()
    return d
