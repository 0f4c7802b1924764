"""ctypes binding of libquadrace.so (the C ABI declared in include/quadrace.h).

This is the reference's own FFI style (ctypes.CDLL + POINTER(c_float), R:4395-4417).  The library is the
hand-written HIP implementation; there is no Python/NumPy fallback: if it cannot be built or loaded, or no
gfx950 GPU is visible, the caller gets an exception.
"""
import ctypes as C
import os

from . import build as _build

QR_OK, QR_E_INVALID, QR_E_NO_DEVICE, QR_E_HIP, QR_E_STATE = 0, -1, -2, -3, -4
QR_VARIANT_E2E, QR_VARIANT_INDI = 0, 1
QR_MAX_GATES, QR_MAX_GATES_AHEAD, QR_RESIDUAL_FLOATS = 32, 4, 740

_f32p = C.POINTER(C.c_float)
_vp = C.c_void_p


class QrConfig(C.Structure):
    _fields_ = [("variant", C.c_int32), ("num_envs", C.c_int32), ("gates_ahead", C.c_int32), ("device", C.c_int32),
                ("pause_if_collision", C.c_int32), ("reserved0", C.c_int32), ("env_id_base", C.c_uint64)]


class QrPpoMemberArgs(C.Structure):
    """qr_ppo_member_args of include/quadrace.h: one member's arguments of qr_ppo_population_epoch, the ones qr_ppo_epoch takes."""
    _fields_ = ([(n, _vp) for n in ("theta_dev", "adam_m_dev", "adam_v_dev", "obs_dev", "act_dev", "old_logp_dev", "adv_dev", "ret_dev", "perm_dev")] +
                [(n, C.c_float) for n in ("clip", "vf_coef", "ent_coef", "max_grad_norm", "lr", "beta1", "beta2", "eps")] + [("stats_dev", _vp)])


class QrPpoPrepareShared(C.Structure):
    """qr_ppo_prepare_shared of include/quadrace.h: the one collect launch's outputs, [K][N][...]."""
    _fields_ = ([(n, C.c_int32) for n in ("K", "N", "E")] +
                [(n, _vp) for n in ("obs", "act", "logp", "rew", "done", "trunc", "last_obs", "term_obs")])


class QrPpoPrepareMember(C.Structure):
    """qr_ppo_prepare_member of include/quadrace.h: one member's columns, hyper-parameters and own buffers for qr_ppo_population_prepare."""
    _fields_ = ([("first_env", C.c_int32), ("gamma", C.c_float), ("lam", C.c_float)] +
                [(n, _vp) for n in ("obs", "act", "old_logp", "rew", "done", "val", "term_val", "last_val", "adv", "ret", "ep_ret", "ep_len", "ep_gates")])


class QrEsFitnessWeights(C.Structure):
    """qr_es_fitness_weights of include/quadrace.h: the weights of qr_es_fitness's score (passed by reference)."""
    _fields_ = [(n, C.c_double) for n in ("w_gate", "w_crash", "w_timeout", "w_return", "w_lap", "no_lap_steps")] + [("reserved", C.c_int32 * 2)]


QR_ES_SHAPE_CENTERED_RANK, QR_ES_SHAPE_NONE = 0, 1

# name -> (restype, argtypes); must list every symbol of include/quadrace.h and include/quad3d.h, each bound compatibly with its
# declaration: tests/test_abi_host.py::test_every_declared_function_is_bound_compatibly holds every row against the headers
SIGNATURES = {
    "qr_abi_version": (C.c_int, []),
    "qr_last_error": (C.c_char_p, []),
    "qr_create": (C.c_int, [C.POINTER(QrConfig), C.POINTER(_vp)]),
    "qr_destroy": (C.c_int, [_vp]),
    "qr_state_len": (C.c_int, [_vp]),
    "qr_obs_len": (C.c_int, [_vp]),
    "qr_num_envs": (C.c_int, [_vp]),
    "qr_set_track": (C.c_int, [_vp, _f32p, _f32p, C.c_int32, _f32p]),
    "qr_get_track_tables": (C.c_int, [_vp, _f32p, _f32p]),
    "qr_set_residual": (C.c_int, [_vp, _f32p, C.c_size_t]),
    "qr_set_disturbance": (C.c_int, [_vp, _f32p, C.c_float]),
    "qr_set_limits": (C.c_int, [_vp, C.c_int32, C.c_float]),
    "qr_set_pause": (C.c_int, [_vp, C.c_int32]),
    "qr_set_pause_if_collision": (C.c_int, [_vp, C.c_int32]),
    "qr_set_terminal_obs": (C.c_int, [_vp, _vp, C.c_int32]),
    "qr_set_timing": (C.c_int, [_vp, C.c_int32]),
    "qr_rollout_kernel_name": (C.c_char_p, [_vp]),
    "qr_set_rollout_form": (C.c_int, [_vp, C.c_int32]),
    "qr_seed": (C.c_int, [_vp, C.c_uint64]),
    "qr_reset": (C.c_int, [_vp, _vp, _vp, _vp]),
    "qr_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qr_step_many": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qr_step_launches": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qr_observe": (C.c_int, [_vp, _vp, _vp]),
    "qr_probe_residual": (C.c_int, [_vp, _vp, _vp]),
    "qr_get_state": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qr_set_state": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qr_last_step_many_ms": (C.c_int, [_vp, _f32p]),
    "qr_policy_create": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(_vp)]),
    "qr_policy_destroy": (C.c_int, [_vp]),
    "qr_policy_last_error": (C.c_char_p, []),
    "qr_policy_set_weights": (C.c_int, [_vp] + [_f32p] * 8),
    "qr_policy_forward": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp]),
    "qr_policy_forward_f32class": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp]),
    "qr_rollout_policy": (C.c_int, [_vp, _vp, C.c_int32, _f32p, C.c_uint64, C.c_uint64, C.c_int32, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp]),
    "qr_evaluate_policy": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "qr_policy_bank_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp)]),
    "qr_policy_bank_destroy": (C.c_int, [_vp]),
    "qr_policy_bank_capacity": (C.c_int, [_vp]),
    "qr_policy_bank_set": (C.c_int, [_vp, C.c_int32] + [_f32p] * 8),
    "qr_evaluate_policy_bank": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "qr_condition_bank_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp)]),
    "qr_condition_bank_destroy": (C.c_int, [_vp]),
    "qr_condition_bank_capacity": (C.c_int, [_vp]),
    "qr_condition_bank_set": (C.c_int, [_vp, C.c_int32, _f32p, _f32p, C.c_int32, _f32p, _f32p, C.c_float, C.c_int32, C.c_int32]),
    "qr_evaluate_policy_grid": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                                          _vp, _vp, _vp]),
    "qr_dynamics_count": (C.c_int, [C.c_int32]),
    "qr_dynamics_nominal": (C.c_int, [C.c_int32, _f32p, C.c_int32]),
    "qr_dynamics_bank_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp)]),
    "qr_dynamics_bank_destroy": (C.c_int, [_vp]),
    "qr_dynamics_bank_capacity": (C.c_int, [_vp]),
    "qr_dynamics_bank_set": (C.c_int, [_vp, C.c_int32, _f32p, C.c_int32]),
    "qr_dynamics_bank_read": (C.c_int, [_vp, C.c_int32, _f32p, C.c_int32]),
    "qr_evaluate_policy_dynamics_grid": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                   C.POINTER(C.c_int32), C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "qr_sensing_bank_create": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(_vp)]),
    "qr_sensing_bank_destroy": (C.c_int, [_vp]),
    "qr_sensing_bank_capacity": (C.c_int, [_vp]),
    "qr_sensing_bank_set": (C.c_int, [_vp, C.c_int32, _f32p, C.c_int32]),
    "qr_sensing_bank_read": (C.c_int, [_vp, C.c_int32, _f32p, C.POINTER(C.c_int32)]),
    "qr_evaluate_policy_sensing_grid": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                  C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, _vp,
                                                  _vp, _vp, _vp]),
    "qr_sensing_noise": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, _vp, _vp]),
    "qr_rollout_policy_conditions": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, _f32p, C.c_uint64, C.c_uint64,
                                               C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qr_rollout_policy_dynamics": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, _f32p,
                                             C.c_uint64, C.c_uint64, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qr_rollout_policy_sensing": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32), C.c_int32, _f32p, C.c_uint64, C.c_uint64, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _vp, _vp, _vp]),
    "qr_rollout_policy_history": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32), C.c_int32, C.c_int32, _f32p, C.c_uint64, C.c_uint64, C.c_int32, _vp, _vp, _vp, _vp,
                                            _vp, _vp, _vp, _vp, _vp]),
    "qr_evaluate_policy_history_grid": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                  C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64,
                                                  _vp, _vp, _vp, _vp]),
    # qr_rollout_policy_history with critic_obs_out_dev behind obs_out_dev and critic_last_obs_dev behind last_obs_dev
    "qr_rollout_policy_privileged": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                               C.POINTER(C.c_int32), C.c_int32, C.c_int32, _f32p, C.c_uint64, C.c_uint64, C.c_int32, _vp, _vp, _vp, _vp,
                                               _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qr_blackbox_policy_grid": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64,
                                          _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "qr_vehicle_physical_count": (C.c_int, [C.c_int32]),
    "qr_vehicle_bank_sample": (C.c_int, [_vp, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32, C.c_uint64, C.c_uint64,
                                          _vp]),
    "qr_rollout_policy_population": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, _f32p,
                                               C.POINTER(C.c_uint64), C.c_uint64, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qr_record_row_len": (C.c_int, [_vp]),
    "qr_record_policy": (C.c_int, [_vp, _vp, C.c_int32, _f32p, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, _vp, _vp]),
    "qr_blackbox_policy": (C.c_int, [_vp, _vp, C.c_int32, _f32p, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp,
                                     _vp]),
    "qr_profile_steps": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _f32p, _f32p]),
    "qr_ppo_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp)]),
    "qr_ppo_create_ex": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp)]),
    "qr_ppo_destroy": (C.c_int, [_vp]),
    "qr_ppo_num_params": (C.c_int, [_vp]),
    "qr_ppo_pack": (C.c_int, [_vp, _vp, _vp]),
    "qr_ppo_grad": (C.c_int, [_vp] * 8 + [C.c_int32, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp]),
    "qr_ppo_grad_f32class": (C.c_int, [_vp] * 8 + [C.c_int32, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp]),
    "qr_ppo_minibatch": (C.c_int, [_vp] * 10 + [C.c_int32] + [C.c_float] * 8 + [C.c_int32, _vp, _vp]),
    "qr_ppo_forward": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "qr_ppo_gae": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_float, C.c_float] + [_vp] * 7),
    "qr_ppo_apply": (C.c_int, [_vp] * 5 + [C.c_int32] + [C.c_float] * 5 + [C.c_int32, _vp, _vp]),
    "qr_ppo_epoch_begin": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, _vp]),
    "qr_ppo_epoch": (C.c_int, [_vp] * 10 + [C.c_int32] * 4 + [C.c_float] * 8 + [_vp, _vp]),
    # the three update calls with critic_obs_dev directly behind obs_dev (the privileged critic)
    "qr_ppo_grad_privileged": (C.c_int, [_vp] * 9 + [C.c_int32, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp]),
    "qr_ppo_minibatch_privileged": (C.c_int, [_vp] * 11 + [C.c_int32] + [C.c_float] * 8 + [C.c_int32, _vp, _vp]),
    "qr_ppo_epoch_privileged": (C.c_int, [_vp] * 11 + [C.c_int32] * 4 + [C.c_float] * 8 + [_vp, _vp]),
    "qr_ppo_shuffle_state": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.c_int32, _vp]),
    "qr_ppo_adam_step": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int32, _vp]),
    "qr_ppo_control": (C.c_int, [_vp, C.c_float, C.c_int32, _vp]),
    "qr_ppo_status": (C.c_int, [_vp, C.POINTER(C.c_int32), _vp]),
    "qr_ppo_population_create": (C.c_int, [C.POINTER(_vp), C.c_int32, C.POINTER(_vp)]),
    "qr_ppo_population_destroy": (C.c_int, [_vp]),
    "qr_ppo_population_epoch": (C.c_int, [_vp, C.POINTER(QrPpoMemberArgs), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp]),
    "qr_ppo_population_status": (C.c_int, [_vp, C.POINTER(C.c_int32), _vp]),
    "qr_ppo_population_load_bank": (C.c_int, [_vp, C.POINTER(_vp), _vp, C.c_int32, _vp]),
    "qr_policy_bank_read": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, C.c_size_t]),
    "qr_ppo_population_prepare": (C.c_int, [_vp, C.POINTER(QrPpoPrepareShared), C.POINTER(QrPpoPrepareMember), C.POINTER(C.c_double), _vp]),
    "qr_ppo_population_exploit": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int32), _f32p, _vp]),
    "qr_es_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp)]),
    "qr_es_destroy": (C.c_int, [_vp]),
    "qr_es_num_params": (C.c_int, [_vp]),
    "qr_es_noise": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp, _vp]),
    "qr_es_perturb": (C.c_int, [_vp, _vp, C.c_float, C.c_uint64, C.c_uint64, _vp, C.c_int32, _vp, _vp]),
    "qr_es_fitness": (C.c_int, [_vp, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp]),   # w: byref(QrEsFitnessWeights)
    "qr_es_update": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_float, C.c_uint64, C.c_uint64, C.c_int32] + [C.c_float] * 5 + [C.c_int32, _vp, _vp]),
    # include/quad3d.h (predecessor environments of "3D quad.ipynb")
    "q3_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.POINTER(_vp)]),
    "q3_destroy": (C.c_int, [_vp]),
    "q3_num_envs": (C.c_int, [_vp]),
    "q3_elem_size": (C.c_int, [_vp]),
    "q3_set_track": (C.c_int, [_vp, _f32p, _f32p, C.c_int32, _f32p]),
    "q3_set_limits": (C.c_int, [_vp, C.c_int32, C.c_double]),
    "q3_set_thresholds": (C.c_int, [_vp, C.c_double, C.c_double, C.c_double, C.c_double]),
    "q3_seed": (C.c_int, [_vp, C.c_uint64]),
    "q3_reset": (C.c_int, [_vp, _vp, _vp, _vp]),
    "q3_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "q3_step_many": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, _vp, _vp]),
    "q3_rollout": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "q3_get_state": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "q3_set_state": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "q3_rollout_policy": (C.c_int, [_vp, _vp, C.c_int32, _f32p, C.c_uint64, C.c_uint64, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp]),
    "q3_episode_counts": (C.c_int, [_vp, _vp, _vp, _vp]),
    "q3_evaluate_policy": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "q3_evaluate_policy_bank": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
}


OPTIONAL_SYMBOLS = ("qr_set_rollout_form", "qr_ppo_create_ex", "q3_rollout", "qr_policy_forward_f32class", "qr_ppo_grad_f32class", "qr_evaluate_policy",
                    "qr_record_policy", "qr_record_row_len", "qr_policy_bank_create", "qr_policy_bank_destroy", "qr_policy_bank_capacity",
                    "qr_policy_bank_set", "qr_evaluate_policy_bank", "qr_condition_bank_create", "qr_condition_bank_destroy",
                    "qr_condition_bank_capacity", "qr_condition_bank_set", "qr_evaluate_policy_grid",
                    "qr_rollout_policy_conditions", "qr_blackbox_policy", "q3_evaluate_policy",
                    "q3_evaluate_policy_bank", "qr_rollout_policy_population", "qr_ppo_population_create", "qr_ppo_population_destroy",
                    "qr_ppo_population_epoch", "qr_ppo_population_status", "qr_ppo_population_load_bank", "qr_policy_bank_read",
                    "qr_ppo_population_prepare", "qr_ppo_population_exploit", "qr_es_create", "qr_es_destroy", "qr_es_num_params", "qr_es_noise",
                    "qr_es_perturb", "qr_es_fitness", "qr_es_update", "qr_dynamics_count", "qr_dynamics_nominal", "qr_dynamics_bank_create",
                    "qr_dynamics_bank_destroy", "qr_dynamics_bank_capacity", "qr_dynamics_bank_set", "qr_dynamics_bank_read",
                    "qr_evaluate_policy_dynamics_grid", "qr_rollout_policy_dynamics", "qr_vehicle_physical_count",
                    "qr_vehicle_bank_sample", "qr_sensing_bank_create", "qr_sensing_bank_destroy", "qr_sensing_bank_capacity", "qr_sensing_bank_set",
                    "qr_sensing_bank_read", "qr_evaluate_policy_sensing_grid", "qr_sensing_noise",
                    "qr_rollout_policy_sensing", "qr_rollout_policy_history", "qr_evaluate_policy_history_grid",
                    "qr_blackbox_policy_grid", "qr_rollout_policy_privileged", "qr_ppo_grad_privileged", "qr_ppo_minibatch_privileged",
                    "qr_ppo_epoch_privileged")   # added in rounds 5-14 and after: a QR_PROBE_LIB build of older sources may lack them


def require(L, name):
    """The optional entry point `name` of the loaded library, or a QuadraceError that names it (an older library loaded under QR_PROBE_LIB)."""
    try:
        return getattr(L, name)
    except AttributeError:
        raise QuadraceError(QR_E_STATE, "the loaded libquadrace.so does not export %s (built from older sources): rebuild it" % name) from None


class QuadraceError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libquadrace error {code}: {msg}")
        self.code = code


_lib = None


def lib_path():
    return _build.LIB


def load(build_if_missing=True):
    """Load libquadrace.so (building it with hipcc first if it is missing or stale)."""
    global _lib
    if _lib is not None:
        return _lib
    if build_if_missing and _build.needs_build():
        _build.build_native_locked()   # one builder at a time (torchrun starts every rank at once)
    if not os.path.exists(_build.LIB):
        raise RuntimeError(f"{_build.LIB} is missing: run `python -m optimal_quad_control_rl_amd.build`")
    L = C.CDLL(_build.LIB)
    for name, (rt, at) in SIGNATURES.items():
        if name in OPTIONAL_SYMBOLS and not hasattr(L, name) and os.environ.get("QR_PROBE_LIB"):
            continue   # a forensic build of an older source tree (tools/isa_patch.py): ABI 3 is additive, the older library lacks the entry
        fn = getattr(L, name)  # AttributeError here = ABI drift between header and library
        fn.restype, fn.argtypes = rt, at
    if L.qr_abi_version() != 3:
        raise RuntimeError("libquadrace ABI version mismatch")
    _lib = L
    return L


def check(rc):
    if rc != QR_OK:
        raise QuadraceError(rc, load().qr_last_error().decode("utf-8", "replace"))
