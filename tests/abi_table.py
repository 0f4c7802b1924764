"""What is pinned about single entry points of the C ABI, one row per entry point; tests/test_abi_host.py::test_pinned_entry_points
checks every row against the headers (through tests/abi_decl.py), optimal_quad_control_rl_amd/_lib.py and build.py.  Data only.

A row is row(name, [argument names in order], **pins); every pin is optional:
  types               the declared C types: a full list, or {position: type}
  bound               the ctypes argument types of _lib.SIGNATURES, exactly: a full list, or {position: type}
  optional            the name is in _lib.OPTIONAL_SYMBOLS
  in_version_comment  a string the comment behind #define QR_ABI_VERSION holds
  in_exports          a string csrc/exports.map holds (its qr_*; / q3_*; pattern is checked for every row)
  source              a file of csrc/ that build.SOURCES lists; default_flags: it is absent from build.PER_SOURCE_FLAGS; vgpr_form: it is
                      absent from build.NO_VGPR_FORM
  defines             {#define name: integer value}
  patterns            regular expressions the header's code (comments removed) matches
  contract            (anchor, words): the words stand in the last comment before `anchor` in the header; anchor None = anywhere in it
  same_as             [((start, stop), other entry point, (start, stop))]: the two slices of argument names are equal
  null_call           (arguments, return code or None for "anything but QR_OK", bytes in qr_last_error() or None): runs without a device
A new entry point adds its row here, its row to _lib.SIGNATURES and, while QR_ABI_VERSION stays, its name to _lib.OPTIONAL_SYMBOLS."""
import ctypes as C

from optimal_quad_control_rl_amd import _lib

vp, i32, u64, f32p, i32p, vpp = C.c_void_p, C.c_int32, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_void_p)
WEIGHTS = ["w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4"]
SAMPLING = ["num_steps", "log_std", "noise_seed", "first_step", "flags"]
ROLLOUT_OUT = ["obs_out_dev", "act_out_dev", "logp_out_dev", "rew_out_dev", "done_out_dev", "trunc_out_dev", "last_obs_dev", "stream"]
EVAL_DEFINES = {"QR_EVAL_REC_INTS": 24, "QR_EVAL_MAX_LAPS": 8, "QR_EVAL_REC_FLOATS": 4, "QR_ABI_VERSION": 3}
Q3_DEFINES = {"Q3_EVAL_REC_INTS": 12, "Q3_EVAL_REC_FLOATS": 4}
POP, PREPARE = "quadrace_ppo_population.hip", "quadrace_population_prepare.hip"
POP_CONTRACT = ("typedef struct qr_ppo_population", ["CONTRACT", "bit for bit", "Refused before anything is launched", "captured", "QR_PPO_NO_EPOCH_GRAPH"])
PREPARE_CONTRACT = ("typedef struct {   /* the ONE collect launch's outputs",
                    ["CONTRACT", "bit for bit", "Refused before anything is launched", "captured", "ONE blocking", "qr_policy_bank_set", "no atomic"])
ROLLOUT_WORDS = ["CONTRACT", "bit for bit", "COROLLARY"]
_ONE, _SRC = (C.c_void_p * 1)(None), (C.c_int32 * 1)(0)


def row(name, args, **pins):
    return dict(name=name, args=args, **pins)


ROWS = [
    # the on-device evaluator, the flight recorder, the black box
    row("qr_evaluate_policy", ["env", "policy", "num_steps", "gates_per_lap", "flags", "rec_dev", "recf_dev", "stream"], defines=EVAL_DEFINES),
    row("qr_record_policy", ["env", "policy"] + SAMPLING + ["rec_envs", "rows_dev", "stream"], bound=[vp, vp, i32, f32p, u64, u64, i32, i32, vp, vp],
        optional=True, in_version_comment="qr_record_policy", defines={"QR_RECORD_EXTRA": 8, "QR_ABI_VERSION": 3}),
    row("qr_record_row_len", ["env"], bound=[vp], optional=True, null_call=((None,), _lib.QR_E_INVALID, None)),
    row("qr_blackbox_policy", ["env", "policy"] + SAMPLING + ["trigger", "window", "rec_envs", "ring_dev", "st_dev", "term_dev", "stream"],
        bound=[vp, vp, i32, f32p, u64, u64, i32, i32, i32, i32, vp, vp, vp, vp], optional=True, in_version_comment="qr_blackbox_policy",
        source="quadrace_blackbox.hip", defines={"QR_BLACKBOX_ST_INTS": 4, "QR_ABI_VERSION": 3, "QR_RECORD_EXTRA": 8},
        patterns=[r"QR_BLACKBOX_ON_CRASH\s*=\s*1\s*,\s*QR_BLACKBOX_ON_TIME_LIMIT\s*=\s*2"],
        null_call=((None, None, 1, None, 0, 0, 0, 1, 8, 1, None, None, None, None), None, None)),
    # the policy bank and its evaluator
    row("qr_policy_bank_create", ["obs_len", "device", "capacity", "out"], optional=True, source="quadrace_eval_bank.hip",
        patterns=[r"typedef\s+struct\s+qr_policy_bank\s+qr_policy_bank\s*;"], defines={"QR_ABI_VERSION": 3}),
    row("qr_policy_bank_destroy", ["bank"], optional=True),
    row("qr_policy_bank_capacity", ["bank"], optional=True),
    row("qr_policy_bank_set", ["bank", "slot"] + WEIGHTS, optional=True, same_as=[((2, None), "qr_policy_set_weights", (1, None))]),
    row("qr_evaluate_policy_bank", ["env", "bank", "num_policies", "envs_per_policy", "num_steps", "gates_per_lap", "flags", "rec_dev", "recf_dev",
                                    "stream"], optional=True, contract=(None, ["GROUP-LOCAL RESET STREAM"])),
    # the condition bank and the grid evaluator
    row("qr_condition_bank_create", ["variant", "device", "capacity", "out"], optional=True, in_version_comment="qr_condition_bank_",
        source="quadrace_eval_grid.hip", patterns=[r"typedef\s+struct\s+qr_condition_bank\s+qr_condition_bank\s*;"], defines={"QR_ABI_VERSION": 3}),
    row("qr_condition_bank_destroy", ["bank"], optional=True),
    row("qr_condition_bank_capacity", ["bank"], optional=True),
    row("qr_condition_bank_set", ["bank", "slot", "gate_pos", "gate_yaw", "num_gates", "start_pos", "dist_ranges", "dist_scale", "max_steps",
                                  "gates_per_lap"], optional=True, same_as=[((2, 6), "qr_set_track", (1, None))]),
    row("qr_evaluate_policy_grid", ["env", "policies", "conditions", "num_groups", "envs_per_group", "policy_of_group", "condition_of_group",
                                    "num_steps", "flags", "rec_dev", "recf_dev", "stream"], optional=True, contract=(None, ["bit for bit"])),
    # the closed-loop rollouts across conditions and for a population
    row("qr_rollout_policy_conditions", ["env", "policy", "conditions", "num_groups", "envs_per_group", "condition_of_group"] + SAMPLING + ROLLOUT_OUT,
        bound={5: i32p, 8: u64, 9: u64}, optional=True, in_version_comment="qr_rollout_policy_conditions", source="quadrace_rollout_cond.hip",
        defines={"QR_ABI_VERSION": 3}, contract=("int qr_rollout_policy_conditions", ROLLOUT_WORDS),
        same_as=[((6, 10), "qr_rollout_policy", (2, 6)), ((11, None), "qr_rollout_policy", (7, None))]),
    row("qr_rollout_policy_population", ["env", "policies", "conditions", "num_groups", "envs_per_group", "policy_of_group", "condition_of_group"]
        + SAMPLING + ROLLOUT_OUT,
        types={1: "qr_policy_bank *", 2: "qr_condition_bank *", 5: "const int32_t *", 6: "const int32_t *", 8: "const float *",
               9: "const uint64_t *", 10: "uint64_t", 11: "int32_t"},
        bound={5: i32p, 6: i32p, 8: f32p, 9: C.POINTER(u64), 10: u64, 11: i32}, optional=True, in_version_comment="qr_rollout_policy_population",
        in_exports="qr_rollout_policy_population", source="quadrace_rollout_population.hip", default_flags=True, defines={"QR_ABI_VERSION": 3},
        contract=("int qr_rollout_policy_population", ROLLOUT_WORDS), same_as=[((10, None), "qr_rollout_policy_conditions", (9, None))]),
    # the population update, its prepare and exploit
    row("qr_ppo_population_create", ["members", "num_members", "out"], types=["qr_ppo * const *", "int32_t", "qr_ppo_population * *"],
        bound=[vpp, i32, vpp], optional=True, in_version_comment="qr_ppo_population_create", in_exports="qr_ppo_population_", source=POP,
        default_flags=True, vgpr_form=True, defines={"QR_ABI_VERSION": 3}, contract=POP_CONTRACT,
        patterns=[r"typedef\s+struct\s+qr_ppo_population\s+qr_ppo_population\s*;"]),
    row("qr_ppo_population_destroy", ["pop"], types=["qr_ppo_population *"], bound=[vp], optional=True),
    row("qr_ppo_population_epoch", ["pop", "args", "B", "num_minibatches", "num_epochs", "device_shuffle", "stream"],
        types=["qr_ppo_population *", "const qr_ppo_member_args *", "int32_t", "int32_t", "int32_t", "int32_t", "void *"],
        bound=[vp, C.POINTER(_lib.QrPpoMemberArgs), i32, i32, i32, i32, vp], optional=True),
    row("qr_ppo_population_status", ["pop", "out", "stream"], types=["qr_ppo_population *", "int32_t *", "void *"], bound=[vp, i32p, vp],
        optional=True),
    row("qr_ppo_population_load_bank", ["pop", "theta_dev", "bank", "first_slot", "stream"],
        types=["qr_ppo_population *", "const float * const *", "qr_policy_bank *", "int32_t", "void *"], bound=[vp, vpp, vp, i32, vp],
        optional=True, in_version_comment="qr_ppo_population_load_bank", source=PREPARE, default_flags=True, vgpr_form=True,
        defines={"QR_ABI_VERSION": 3}, contract=PREPARE_CONTRACT),
    row("qr_policy_bank_read", ["bank", "slot", "which", "out_host", "bytes"], types=["const qr_policy_bank *", "int32_t", "int32_t", "void *", "size_t"],
        bound=[vp, i32, i32, vp, C.c_size_t], optional=True, in_version_comment="qr_policy_bank_read"),
    row("qr_ppo_population_prepare", ["pop", "sh", "members", "report_host", "stream"],
        types=["qr_ppo_population *", "const qr_ppo_prepare_shared *", "const qr_ppo_prepare_member *", "double *", "void *"],
        bound=[vp, C.POINTER(_lib.QrPpoPrepareShared), C.POINTER(_lib.QrPpoPrepareMember), C.POINTER(C.c_double), vp], optional=True,
        in_version_comment="qr_ppo_population_prepare"),
    row("qr_ppo_population_exploit", ["pop", "theta_dev", "adam_m_dev", "adam_v_dev", "src_of", "log_std_shift", "stream"],
        types=["qr_ppo_population *", "float * const *", "float * const *", "float * const *", "const int32_t *", "const float *", "void *"],
        bound=[vp, vpp, vpp, vpp, i32p, f32p, vp], optional=True, in_version_comment="qr_ppo_population_exploit", defines={"QR_ABI_VERSION": 3},
        contract=("int qr_ppo_population_exploit", ["CONTRACT", "bit for bit", "Refused before anything is launched", "captured", "no host read",
                                                    "no atomic", "qr_ppo_pack", "qr_ppo_adam_step", "itself a destination"]),
        null_call=((None, _ONE, _ONE, _ONE, _SRC, None, None), _lib.QR_E_INVALID, b"qr_ppo_population_exploit")),
    # the predecessor envs (include/quad3d.h)
    row("q3_rollout_policy", ["env", "policy"] + SAMPLING + ["obs_out_dev", "act_out_dev", "logp_out_dev", "rew_out_dev", "done_out_dev",
                                                             "trunc_out_dev", "term_obs_dev", "last_obs_dev", "states_out_dev", "stream"]),
    row("q3_evaluate_policy", ["env", "policy", "num_steps", "flags", "rec_dev", "recf_dev", "stream"], defines=Q3_DEFINES),
    row("q3_evaluate_policy_bank", ["env", "bank", "num_policies", "envs_per_policy", "num_steps", "flags", "rec_dev", "recf_dev", "stream"],
        defines=Q3_DEFINES),
]
