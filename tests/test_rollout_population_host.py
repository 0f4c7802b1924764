"""CPU: the closed-loop rollout for a population of policies in the package (qr_rollout_policy_population itself is pinned in
tests/abi_table.py); the 32-byte sampling table entry; the [G][4] / [G] argument conversion of _closed_loop.py; PopulationPPO's argument
checks on a stub env (they come before anything touches a GPU)."""
import os
import re

import numpy as np
import pytest

from abi_decl import stub_env as _stub_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sampling_table_entry_is_32_bytes_in_the_launch_header():
    from optimal_quad_control_rl_amd import build

    text = open(os.path.join(build.CSRC, "quadrace_launch.hpp")).read()
    body = text.split("struct PopulationEntry {")[1].split("};")[0]
    fields = re.sub(r"//[^\n]*", "", body)
    assert re.findall(r"(float|uint32_t)\s+([^;]+);", fields) == [("float", "std[4]"), ("float", "logp_const"), ("uint32_t", "seed_lo, seed_hi"),
                                                                   ("uint32_t", "pad")]
    assert "static_assert(sizeof(PopulationEntry) == 32" in text


def test_package_surface():
    import optimal_quad_control_rl_amd as pkg
    from optimal_quad_control_rl_amd import population
    from optimal_quad_control_rl_amd.vec_env import Quadcopter3DGates

    assert pkg.PopulationPPO is population.PopulationPPO and "PopulationPPO" in pkg.__all__
    assert callable(Quadcopter3DGates.rollout_policy_population_device)
    for method in ("collect", "train", "learn", "state_dict", "load_state_dict", "load_bank"):
        assert callable(getattr(population.PopulationPPO, method)), method
    assert os.path.exists(os.path.join(ROOT, "tools", "train_population.py"))


def test_group_argument_conversion():
    import torch

    from optimal_quad_control_rl_amd._closed_loop import log_std_array, log_std_rows, noise_seed_array

    rows = log_std_rows([[0.0, -1.0, 0.5, 2.0], np.arange(4), torch.full((4,), -0.25)], 3)
    assert rows.dtype == np.float32 and rows.shape == (3, 4) and rows.flags["C_CONTIGUOUS"]
    assert np.array_equal(rows[1], log_std_array(np.arange(4))) and np.array_equal(rows[2], np.full(4, -0.25, np.float32))
    t = torch.arange(8, dtype=torch.float64).view(2, 4)
    assert np.array_equal(log_std_rows(t, 2), np.arange(8, dtype=np.float32).reshape(2, 4))
    assert np.array_equal(log_std_rows(np.zeros((2, 4)), 2), np.zeros((2, 4), np.float32))
    for bad, g in (([[0.0] * 4], 2), (np.zeros((2, 3)), 2), (np.zeros(8), 2), ([], 1)):
        with pytest.raises(ValueError):
            log_std_rows(bad, g)
    seeds = noise_seed_array([0, 7, 2 ** 64 - 1, -1], 4)
    assert seeds.dtype == np.uint64 and seeds.tolist() == [0, 7, 2 ** 64 - 1, 2 ** 64 - 1]
    with pytest.raises(ValueError):
        noise_seed_array([1, 2], 3)


def test_population_argument_checks_come_first():
    from optimal_quad_control_rl_amd.population import PopulationPPO

    two = [dict(seed=3), dict(seed=4, learning_rate=1e-4)]
    with pytest.raises(ValueError, match="n_steps"):
        PopulationPPO(_stub_env(512), [dict(seed=3, n_steps=16), dict(seed=4, n_steps=32)])                # unequal n_steps
    with pytest.raises(ValueError, match="n_steps"):
        PopulationPPO(_stub_env(512), [dict(seed=3, n_steps=16), dict(seed=4)], n_steps=32)                 # ... against the shared value
    with pytest.raises(ValueError, match="policy_forward"):
        PopulationPPO(_stub_env(512), [dict(seed=3, policy_forward="f32class"), dict(seed=4)], n_steps=16)
    for e in (128, 384, 0, 257):
        with pytest.raises(ValueError, match="256"):
            PopulationPPO(_stub_env(768), two, envs_per_member=e, n_steps=16)                               # not a multiple of 256
    with pytest.raises(ValueError, match="num_envs"):
        PopulationPPO(_stub_env(768), two, envs_per_member=256, n_steps=16)                                 # 2 * 256 != 768
    with pytest.raises(ValueError, match="num_envs"):
        PopulationPPO(_stub_env(1024), two + [dict(seed=5)], envs_per_member=512, n_steps=16)               # 3 * 512 != 1024
    with pytest.raises(ValueError, match="num_envs"):
        PopulationPPO(_stub_env(1000), two, envs_per_member=512, n_steps=16)                                # not whole groups
    with pytest.raises(ValueError):
        PopulationPPO(_stub_env(512), [], n_steps=16)
    with pytest.raises(ValueError, match="fused_collect"):
        PopulationPPO(_stub_env(512), two, n_steps=16, fused_collect=False)
    with pytest.raises(ValueError, match="condition_of_member"):
        PopulationPPO(_stub_env(512), two, n_steps=16, condition_of_member=[0, 0])                          # a map without conditions


def test_train_population_arguments():
    import importlib.util

    spec = importlib.util.spec_from_file_location("train_population", os.path.join(ROOT, "tools", "train_population.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)          # defines functions only: the run itself is main()
    assert tool.parse_seeds("0-9") == list(range(10))
    assert tool.parse_seeds("3,5,8-10") == [3, 5, 8, 9, 10]
    assert tool.parse_seeds("7") == [7]
    for bad in ("", "5-3", "a", "1,,2"):
        with pytest.raises(SystemExit):
            tool.parse_seeds(bad)
    args = tool.parser().parse_args(["--seeds", "0-2", "--envs-per-member", "512"])
    assert args.envs_per_member == 512 and tool.parse_seeds(args.seeds) == [0, 1, 2]
