"""CPU-side checks of training under observation noise and command delay (no GPU needed): the entry point qr_rollout_policy_sensing
against include/quadrace.h and optimal_quad_control_rl_amd/_lib.py and what it refuses without a device; sensing.plan_sensor_mix; the two
flags of tools/train_ppo.py; and the argument checks of PPO(sensing=...), which come before the env is touched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import abi_decl
import test_abi_host
from abi_table import f32p, i32, i32p, row, u64, vp
from optimal_quad_control_rl_amd import _lib
from optimal_quad_control_rl_amd import sensing as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "qr_rollout_policy_sensing"
ARGS = ["env", "policy", "conditions", "dynamics", "sensing", "num_groups", "envs_per_group", "condition_of_group", "dynamics_of_group",
        "sensing_of_group", "num_steps", "log_std", "noise_seed", "first_step", "flags", "pending_dev", "obs_out_dev", "act_out_dev", "logp_out_dev",
        "rew_out_dev", "done_out_dev", "trunc_out_dev", "last_obs_dev", "stream"]
TYPES = ["qr_env *", "qr_policy *", "qr_condition_bank *", "qr_dynamics_bank *", "qr_sensing_bank *", "int32_t", "int32_t", "const int32_t *",
         "const int32_t *", "const int32_t *", "int32_t", "const float *", "uint64_t", "uint64_t", "int32_t", "float *", "float *", "float *", "float *",
         "float *", "uint8_t *", "uint8_t *", "float *", "void *"]
BOUND = [vp] * 5 + [i32, i32, i32p, i32p, i32p, i32, f32p, u64, u64, i32] + [vp] * 9
NULL_CALL = (None,) * 5 + (1, 256, None, None, None, 1, None, 0, 0, 0) + (None,) * 9
ROW = row(NAME, ARGS, types=TYPES, bound=BOUND, optional=True, in_version_comment=NAME, in_exports="qr_*", source="quadrace_rollout_sensing.hip",
          default_flags=True, vgpr_form=True, defines={"QR_ABI_VERSION": 3},
          contract=("int " + NAME, ["CONTRACT", "bit for bit", "Refused before anything is launched", "ORDINARY env id", "NOISY row",
                                    "TERMINAL-OBSERVATION ROWS ARE CLEAN", "pending carried", "row 0 of obs_out", "scalar registers", "no atomic", "canonical order"]),
          same_as=[((0, 4), "qr_rollout_policy_dynamics", (0, 4)), ((5, 9), "qr_rollout_policy_dynamics", (4, 8)),
                   ((10, 15), "qr_rollout_policy_dynamics", (8, 13)), ((16, None), "qr_rollout_policy_dynamics", (13, None)),
                   ((4, 5), "qr_evaluate_policy_sensing_grid", (4, 5)), ((9, 10), "qr_evaluate_policy_sensing_grid", (10, 11)),
                   ((15, 16), "qr_evaluate_policy_sensing_grid", (15, 16))],
          null_call=(NULL_CALL, _lib.QR_E_INVALID, NAME.encode()))


# ---- header <-> _lib <-> the built library --------------------------------------------------------------------------------------------------
def test_the_entry_point_is_pinned():
    test_abi_host.test_pinned_entry_points(ROW)
    assert NAME in _lib.SIGNATURES and NAME in _lib.OPTIONAL_SYMBOLS
    assert len(ARGS) == len(TYPES) == len(BOUND) == len(NULL_CALL) == 24
    assert not NAME.startswith(("qr_sensing_", "qr_dynamics_", "qr_es_"))          # those prefixes are counted by other test files


def test_signature_row_matches_the_argument_list():
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is C.c_int and list(argtypes) == BOUND
    _, ret, names, types_ = abi_decl.declaration(abi_decl.header()[1], NAME)
    assert ret == "int" and names == ARGS and types_ == TYPES
    for c_type, ctype in zip(types_, argtypes):
        assert abi_decl.binding_matches(c_type, ctype), (c_type, ctype)


def test_the_library_exports_it_and_the_source_is_built_with_the_default_flags():
    from optimal_quad_control_rl_amd import build

    build.build_native()
    assert hasattr(C.CDLL(build.LIB), NAME)
    assert "quadrace_rollout_sensing.hip" in build.SOURCES and "quadrace_rollout_sensing.hip" not in build.PER_SOURCE_FLAGS
    assert "quadrace_sensing.hpp" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "quadrace_sensing.hpp"))
    for flagless in ("quadrace_rollout_cond.hip", "quadrace_rollout_dynamics.hip"):   # "as quadrace_rollout_cond.hip and _dynamics.hip are"
        assert build.PER_SOURCE_FLAGS.get(flagless) is None
    assert _lib.load().qr_abi_version() == 3


def test_a_null_handle_is_refused_by_name_without_a_device():
    test_abi_host.test_null_handles_are_refused_without_a_device(ROW)
    L = _lib.load()
    assert L.qr_rollout_policy_sensing(*NULL_CALL) == _lib.QR_E_INVALID
    assert NAME.encode() in L.qr_last_error() and b"null env handle" in L.qr_last_error()


def test_the_sensor_lives_in_one_header_that_both_units_include():
    """the evaluator and the rollout call the same device functions: they are defined once, in quadrace_sensing.hpp"""
    from optimal_quad_control_rl_amd import build

    read = lambda f: open(os.path.join(build.CSRC, f)).read()
    shared = read("quadrace_sensing.hpp")
    for name in ("struct SensingRegs", "struct SensingStream", "inline SensingStream sensing_stream(", "void load_sensing(", "constexpr int sensing_group(",
                 "void sensing_noise4(", "void sensing_noise_row(", "kSensingTweak0 = 0x6A09E667u", "kSensingTweak1 = 0x3C6EF372u"):
        assert shared.count(name) == 1, name
        for unit in ("quadrace_eval_sensing.hip", "quadrace_rollout_sensing.hip", "quadrace_rollout_group.hpp", "quadrace_eval_body.hpp"):
            assert name not in read(unit), (name, unit)
    assert '#include "quadrace_sensing.hpp"' in read("quadrace_eval_sensing.hip") and '#include "quadrace_sensing.hpp"' in read("quadrace_rollout_group.hpp")
    assert '#include "quadrace_rollout_group.hpp"' in read("quadrace_rollout_sensing.hip") and "static_assert(rollout_sensing_lds_bytes" in read("quadrace_rollout_sensing.hip")


def test_python_exports():
    import optimal_quad_control_rl_amd as pkg

    assert "plan_sensor_mix" in pkg.__all__ and pkg.plan_sensor_mix is M.plan_sensor_mix


# ---- plan_sensor_mix ------------------------------------------------------------------------------------------------------------------------
def _sensors(n):
    return [M.SensingParams("s%d" % k, sigma_pos=0.01 * k, delay_steps=k % 5) for k in range(n)]


def test_plan_sensor_mix_defaults():
    a, b, c = _sensors(3)
    assert M.plan_sensor_mix(1024, 256, [a]) == ([0, 0, 0, 0], ["s0"])
    assert M.plan_sensor_mix(1280, 256, [a, b]) == ([0, 1, 0, 1, 0], ["s0", "s1"])                  # round-robin, g % S
    assert M.plan_sensor_mix(1536, 512, [a, b, c]) == ([0, 1, 2], ["s0", "s1", "s2"])
    assert M.plan_sensor_mix(768, 256, [a, b, c], sensing_of_group=[2, 2, 0]) == ([2, 2, 0], ["s0", "s1", "s2"])   # any order, repeats, one unused
    assert M.plan_sensor_mix(512, 256, (s for s in (a, b)), np.asarray([1, 0]))[0] == [1, 0]       # any iterable, any integers
    assert M.plan_sensor_mix(256, 256, [a, b], [1])[0] == [1]                                      # an explicit map may leave a sensor out


@pytest.mark.parametrize("args", [
    (1024, 128, "a"), (1024, 384, "a"), (1024, 0, "a"),                    # envs_per_group: a multiple of 256, at least 256
    (1000, 256, "a"), (128, 256, "a"),                                     # a whole number of groups
    (1024, 256, []), (1024, 256, "params"), (1024, 256, ["x"]), (1024, 256, [None]),   # a non-empty list of SensingParams
    (512, 256, "abc"),                                                     # fewer groups than sensors
    (1024, 256, "ab", [0, 1, 0]), (1024, 256, "ab", [0, 1, 0, 2]), (1024, 256, "ab", [0, -1, 0, 1]),   # the map: one valid entry per group
])
def test_plan_sensor_mix_refusals(args):
    named = dict(zip("abc", _sensors(3)))
    n, e, sensing, *rest = args
    if sensing == "params":
        sensing = named["a"]
    elif isinstance(sensing, str):
        sensing = [named[k] for k in sensing]
    with pytest.raises(ValueError):
        M.plan_sensor_mix(n, e, sensing, *rest)


# ---- tools/train_ppo.py -----------------------------------------------------------------------------------------------------------------------
def test_train_ppo_parses_the_two_flags():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sensing_sweep
    import train_ppo as T

    assert T.parse_sigma is sensing_sweep.parse_sigma                                              # the sweep tool's parser, not a copy
    assert T.train_sensors() is None and T.train_sensors("", "") is None
    one = T.train_sensors("0.05")
    assert len(one) == 1 and one[0].delay_steps == 0 and np.array_equal(one[0].sigma, np.full(8, 0.05, np.float32))
    eight = T.train_sensors("0.01,0.02,0.03,0.04,0.05,0.06,0.07,0.08", "2")
    assert len(eight) == 1 and eight[0].delay_steps == 2
    assert np.array_equal(eight[0].sigma, np.asarray([0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08], np.float32))
    mix = T.train_sensors("0.02", "0,1,4")
    assert [s.delay_steps for s in mix] == [0, 1, 4] and [s.name for s in mix] == ["d=0", "d=1", "d=4"]
    assert all(np.array_equal(s.sigma, mix[0].sigma) for s in mix)
    late = T.train_sensors("", "3")                                                                # a delay alone: no noise
    assert len(late) == 1 and late[0].delay_steps == 3 and not late[0].sigma.any()
    assert T.train_sensors("0")[0].is_ideal
    assert M.plan_sensor_mix(1024, 256, mix)[0] == [0, 1, 2, 0]                                    # one sensor per value, round-robin over groups
    for noise, delay in (("1,2", ""), ("-1", ""), ("nan", ""), ("x", ""), ("0.1", "5"), ("0.1", "-1"), ("0.1", "1.5"), ("0.1", "1,1"), ("", "x")):
        with pytest.raises(SystemExit):
            T.train_sensors(noise, delay)
    src = open(os.path.join(ROOT, "tools", "train_ppo.py")).read()
    for flag in ('"--obs-noise"', '"--delay"', "sensing=sensors", "evaluate_sensing_grid", "SensingParams.ideal()"):
        assert flag in src, flag


# ---- PPO's argument checks ------------------------------------------------------------------------------------------------------------------
def test_ppo_checks_its_sensing_arguments_before_it_touches_the_env():
    from optimal_quad_control_rl_amd.ppo import PPO

    env = abi_decl.stub_env(512)                                 # two groups of 256; touching the env raises AssertionError
    a, b, c = _sensors(3)
    for kw in (dict(sensing=[a], fused_collect=False),                                   # fused collect only
               dict(sensing_of_group=[0, 0], fused_collect=True),                        # a map without sensors
               dict(sensing_of_group=[0, 0], fused_collect=False),
               dict(sensing=[], fused_collect=True),
               dict(sensing=a, fused_collect=True),                                      # one sensor is still a list
               dict(sensing=[a, b, c], fused_collect=True),                              # fewer groups than sensors
               dict(sensing=[a, b], sensing_of_group=[0, 2], fused_collect=True),
               dict(sensing=[a, b], sensing_of_group=[0], fused_collect=True),
               dict(sensing=[a], envs_per_group=384, fused_collect=True)):
        with pytest.raises(ValueError):
            PPO(env, **kw)
    with pytest.raises(AssertionError):                                                  # valid arguments: the constructor goes on to the env
        PPO(env, sensing=[a, b], fused_collect=True)
