"""CPU-side checks of the command history (qr_rollout_policy_history, qr_evaluate_policy_history_grid): the identities of its restatement
(tests/command_history_spec.py), the argument validation of PPO(command_history=...) and evaluate_sensing_grid(command_history=...), the
two entry points in the header, the ctypes table and the build, NULL handles, and the rule obs_len + 4 H is a policy length exactly when
gates_ahead + H <= 4.  No GPU."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import abi_decl
import command_history_spec as CH
from optimal_quad_control_rl_amd import _lib, build

ROLLOUT, EVAL = "qr_rollout_policy_history", "qr_evaluate_policy_history_grid"
TWINS = {ROLLOUT: "qr_rollout_policy_sensing", EVAL: "qr_evaluate_policy_sensing_grid"}


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def _sensing_queue_update(queue, cmd, d):
    """the queue update of the per-step loops in tests/test_gpu_rollout_sensing.py and tests/test_gpu_sensing_grid.py (`_loop`), in NumPy"""
    queue = queue.copy()
    if d > 0:
        fly = queue[:, 4 * (d - 1):4 * d].copy()
        queue[:, 4:4 * d] = queue[:, :4 * (d - 1)].copy()
        queue[:, :4] = cmd
    else:
        fly = cmd
    return fly, queue


def _episode(rng, n, steps):
    cmds = rng.uniform(-1, 1, (steps, n, 4)).astype(np.float32)
    done = rng.uniform(size=(steps, n)) < 0.15
    return cmds, done


@pytest.mark.parametrize("d", range(5))
def test_for_h_up_to_d_the_queue_is_the_sensing_queue(d):
    rng = np.random.default_rng(d)
    n, steps = 37, 40
    cmds, done = _episode(rng, n, steps)
    for H in range(d + 1):
        q_spec = np.zeros((n, 16), np.float32)
        q_sen = np.zeros((n, 16), np.float32)
        for k in range(steps):
            fly_a, q_spec = CH.push(q_spec, cmds[k], d, H)
            fly_b, q_sen = _sensing_queue_update(q_sen, cmds[k], d)
            assert np.array_equal(fly_a, fly_b) and np.array_equal(q_spec, q_sen), (H, k)
            q_spec = CH.clear(q_spec, done[k])
            q_sen[done[k]] = 0.0
            assert np.array_equal(q_spec, q_sen), (H, k)
    assert done.any() and not done.all()


def test_fly_is_independent_of_h_and_the_queue_ends_at_max_d_h():
    rng = np.random.default_rng(7)
    n, steps = 29, 48
    cmds, done = _episode(rng, n, steps)
    for d in range(5):
        flown = {}
        for H in range(5):
            q = rng.uniform(-1, 1, (n, 16)).astype(np.float32)            # whatever the caller left behind max(d, H) is dropped by the first push
            q[:, :4 * max(d, H)] = 0.0
            age = np.zeros(n, np.int64)                                   # steps since the episode's start
            seq = []
            for k in range(steps):
                seen = CH.row(np.zeros((n, 5), np.float32), q, H)
                assert seen.shape == (n, 5 + 4 * H)
                for j in range(H):                                        # entry j: the command of j + 1 steps ago, zeros before the episode's start
                    past = cmds[k - j - 1] if k - j - 1 >= 0 else np.zeros((n, 4), np.float32)
                    want = np.where((age > j)[:, None], past, np.float32(0.0))
                    assert np.array_equal(seen[:, 5 + 4 * j:9 + 4 * j], want), (d, H, k, j)
                before = q.copy()
                fly, pushed = CH.push(q, cmds[k], d, H)
                assert np.array_equal(q, before) and fly is not cmds[k], "push modifies nothing"
                q = pushed
                assert not q[:, 4 * max(d, H):].any(), (d, H, k)
                term = CH.terminal_row(np.ones((n, 5), np.float32), q, H)
                assert term.shape == (n, 5 + 4 * H) and bool((term[:, :5] == 1.0).all())
                if H:                                                     # u_k in front, then what the step's row carried, moved back by one
                    assert np.array_equal(term[:, 5:9], cmds[k]) and np.array_equal(term[:, 9:], seen[:, 5:5 + 4 * (H - 1)])
                q = CH.clear(q, done[k])
                assert not q[done[k]].any()
                age = np.where(done[k], 0, age + 1)
                seq.append(fly)
            flown[H] = np.stack(seq)
        for H in range(1, 5):
            assert np.array_equal(flown[H], flown[0]), (d, H)
        if d == 0:
            assert np.array_equal(flown[0], cmds)


def test_the_functions_take_torch_tensors_and_modify_nothing():
    q = torch.arange(3 * 16, dtype=torch.float32).reshape(3, 16)
    cmd = torch.full((3, 4), -1.0)
    keep = q.clone()
    fly, q2 = CH.push(q, cmd, 2, 3)
    assert torch.equal(q, keep) and torch.equal(fly, keep[:, 4:8]) and torch.equal(q2[:, :4], cmd) and torch.equal(q2[:, 4:12], keep[:, :8])
    assert not bool(q2[:, 12:].any())
    q3 = CH.clear(q2, torch.tensor([0, 1, 0], dtype=torch.uint8))
    assert not bool(q3[1].any()) and torch.equal(q3[0], q2[0]) and bool(q2[1].any())
    assert CH.row(torch.zeros((3, 13)), q2, 3).shape == (3, 25) and CH.terminal_row(torch.zeros((3, 13)), q2, 1).shape == (3, 17)


# ---- obs_len + 4 H is a policy length exactly when gates_ahead + H <= 4 --------------------------------------------------------------------
def test_the_longer_row_is_a_policy_length_exactly_when_ga_plus_h_is_at_most_4():
    src = open(os.path.join(build.CSRC, "quadrace_launch.hpp")).read()
    body = src[src.index("auto dispatch_L("):]
    body = body[:body.index("default:")]
    lengths = {int(m) for m in re.findall(r"case (\d+):", body)}
    assert lengths == set(CH.POLICY_LENGTHS)
    for variant in (0, 1):
        for ga in range(5):
            for H in range(1, 9):
                length = CH.obs_len(variant, ga) + 4 * H
                assert (length in lengths) == (ga + H <= 4), (variant, ga, H, length)
                if ga + H <= 4:
                    assert length == CH.obs_len(variant, ga + H)
    from optimal_quad_control_rl_amd.evaluation import check_command_history

    for ga in range(5):
        assert check_command_history(0, ga) == 0
        for H in range(1, 6):
            if ga + H <= 4:
                assert check_command_history(H, ga) == H
            else:
                with pytest.raises(ValueError, match="command_history"):
                    check_command_history(H, ga)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="command_history"):
            check_command_history(bad, 0)


# ---- the entry points ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [ROLLOUT, EVAL])
def test_entry_point_is_declared_bound_and_optional(name):
    text, code = abi_decl.header_of(name)
    _, ret, names, types_ = abi_decl.declaration(code, name)
    twin = abi_decl.declaration(abi_decl.header_of(TWINS[name])[1], TWINS[name])
    at = twin[2].index("sensing_of_group") + 1
    assert names == twin[2][:at] + ["history"] + twin[2][at:], "the sensing call's list with `history` directly behind sensing_of_group"
    assert types_ == twin[3][:at] + ["int32_t"] + twin[3][at:] and ret == "int"
    restype, argtypes = _lib.SIGNATURES[name]
    twin_bound = _lib.SIGNATURES[TWINS[name]][1]
    assert restype is C.c_int and list(argtypes) == list(twin_bound[:at]) + [C.c_int32] + list(twin_bound[at:])
    assert name in _lib.OPTIONAL_SYMBOLS and name in abi_decl.version_comment(text)
    assert abi_decl.define(code, "QR_ABI_VERSION") == 3
    assert name in open(os.path.join(build.CSRC, "exports.map")).read()
    for src in ("quadrace_rollout_history.hip", "quadrace_eval_history.hip"):
        assert src in build.SOURCES and src not in build.PER_SOURCE_FLAGS and src not in build.NO_VGPR_FORM
        assert os.path.exists(os.path.join(build.CSRC, src))
    comment = text.split("int qr_rollout_policy_history(")[0].rsplit("/*", 1)[1]
    for word in ("CONTRACT", "bit for bit", "Refused before anything is launched", "the computed ones, not the flown ones","NOT modelled", "max(d, H)",
                 "gates_ahead + H <= 4", "[rows][N][L']"):
        assert word in comment.replace("\n *", ""), word
    assert "noise on the entries" in text.split("typedef struct qr_sensing_bank")[0].rsplit("NOT modelled", 1)[1][:200]
    assert hasattr(C.CDLL(build.build_native()), name)


def test_null_handles_are_refused_without_a_device():
    L = _lib.load()
    rc = L.qr_rollout_policy_history(*([None] * 5), 1, 256, None, None, None, 1, 1, None, 0, 0, 0, *([None] * 9))
    assert rc == _lib.QR_E_INVALID and b"qr_rollout_policy_history" in L.qr_last_error() and b"null env" in L.qr_last_error()
    rc = L.qr_evaluate_policy_history_grid(*([None] * 5), 1, 256, None, None, None, None, 1, 1, 0, 0, 0, *([None] * 4))
    assert rc == _lib.QR_E_INVALID and b"null env" in L.qr_last_error()


# ---- Python arguments ----------------------------------------------------------------------------------------------------------------------
def _stub_env(gates_ahead=1, q3=False):
    env = types.SimpleNamespace(num_envs=512, device=torch.device("cpu"), gates_ahead=gates_ahead, state_len=24, VARIANT=0)
    if q3:
        env.KIND, env.trainer_state = "hover", lambda: None
        del env.gates_ahead
    return env


def test_ppo_refuses_a_command_history_it_cannot_fly_before_it_touches_the_env():
    from optimal_quad_control_rl_amd.ppo import PPO

    with pytest.raises(ValueError, match="command_history must be 0 or an integer in 1 .. 4 - gates_ahead"):
        PPO(_stub_env(1), fused_collect=True, command_history=4)
    with pytest.raises(ValueError, match="command_history"):
        PPO(_stub_env(0), fused_collect=True, command_history=5)
    with pytest.raises(ValueError, match="command_history"):
        PPO(_stub_env(0), fused_collect=True, command_history=-1)
    with pytest.raises(ValueError, match="command_history needs fused_collect=True"):
        PPO(_stub_env(1), fused_collect=False, command_history=2)
    with pytest.raises(ValueError, match="command_history needs fused_collect=True on a race env"):
        PPO(_stub_env(q3=True), fused_collect=True, command_history=2)


def test_evaluate_sensing_grid_refuses_a_command_history_it_cannot_fly():
    from optimal_quad_control_rl_amd import evaluate_sensing_grid

    for ga, H in ((1, 4), (4, 1), (0, 5), (0, -2)):
        with pytest.raises(ValueError, match="command_history must be 0 or an integer"):
            evaluate_sensing_grid([], [], [], _stub_env(ga), command_history=H)
