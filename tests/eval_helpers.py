"""What the GPU tests of the three on-device evaluators share (tests/test_gpu_evaluate.py, test_gpu_eval_bank.py, test_gpu_eval_grid.py;
tests/test_gpu_table_edges.py reaches them through those modules): the scenario's handles, the two kinds of test policy as layer
lists and as MfmaPolicy, policy banks, zeroed records and the state comparison of one group against a twin handle.  A plain module
next to eval_spec.py; nothing here asserts anything about the evaluators by itself."""
import ctypes as C

import numpy as np
import torch

import eval_spec as S

SENTINEL = -77777.0
SC = S.SCENARIO


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _env(variant, n, gates_ahead, seed=SC["seed"], track=None, max_steps=SC["max_steps"]):
    from optimal_quad_control_rl_amd import Quadcopter3DGates, Quadcopter3DGatesINDI, TRAIN_DISTURBANCE_RANGES

    trk = S.scenario_track() if track is None else track
    if variant == "e2e":
        env = Quadcopter3DGates(n, *trk, gates_ahead=gates_ahead, seed=seed, infos_mode="none")   # residual MLPs: the default
        env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    else:
        env = Quadcopter3DGatesINDI(n, *trk, gates_ahead=gates_ahead, seed=seed, infos_mode="none")
    env.max_steps = max_steps
    env.reset_device()
    return env


def _constant_layers(obs_len, action):
    """zero weights and an output bias: the action does not depend on the observation"""
    z = np.zeros
    return [(z((120, obs_len), np.float32), z(120, np.float32)), (z((120, 120), np.float32), z(120, np.float32)),
            (z((120, 120), np.float32), z(120, np.float32)), (z((4, 120), np.float32), np.asarray(action, np.float32))]


def _closed_loop_layers(obs_len, action, seed=3, gain=5.0):
    """seeded random weights around `action`: action = bias + an observation-dependent term of a few hundredths, so the scenario
    keeps its character while every action depends on the observation the kernel fed to its forward"""
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    torch.manual_seed(seed)
    net = ActorCritic(obs_len, 4)
    with torch.no_grad():
        net.pi[-1].weight.mul_(gain)
        net.pi[-1].bias.copy_(torch.as_tensor(action, dtype=torch.float32))
    return [(m.weight.detach().clone(), m.bias.detach().clone()) for m in net.pi if isinstance(m, torch.nn.Linear)]


def _constant_policy(obs_len, action):
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    return MfmaPolicy(obs_len).set_weights(_constant_layers(obs_len, action))


def _closed_loop_policy(obs_len, action, seed=3, gain=5.0):
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    return MfmaPolicy(obs_len).set_weights(_closed_loop_layers(obs_len, action, seed, gain))


def _policy_bank(obs_len, layer_sets, capacity=None):
    from optimal_quad_control_rl_amd.policy import MfmaPolicyBank

    bank = MfmaPolicyBank(obs_len, capacity or len(layer_sets))
    for slot, layers in enumerate(layer_sets):
        bank.set_weights(slot, layers)
    return bank


def _records(env):
    return (torch.zeros((env.num_envs, S.REC_INTS), dtype=torch.int32, device=env.device),
            torch.zeros((env.num_envs, S.REC_FLOATS), dtype=torch.float32, device=env.device))


def _group_equals(env_state, twin, lo, hi, what):
    """rows [lo, hi) of the five state tensors `env_state` are bit-equal to the whole of `twin`'s"""
    for name, x, y in zip(("world", "disturbances", "target", "steps", "episode"), env_state, twin.get_state_tensors()):
        assert x is None or torch.equal(x[lo:hi], y), (what, name)
