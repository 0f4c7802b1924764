"""optimal_quad_control_rl_amd -- MI355X-native vectorised quadrotor race environment.

Drop-in for the `Quadcopter3DGates` VecEnv classes of tudelft/optimal_quad_control_RL (E2E motor-command
model with residual thrust/moment MLPs, and the INDI inner-loop variant).  The hot path is hand-written HIP
for gfx950 behind a C ABI (include/quadrace.h -> libquadrace.so); this package is the thin ctypes adapter.
"""
from .tracks import TRAIN_DISTURBANCE_RANGES, square_track, zigzag_track  # noqa: F401

__all__ = ["Quadcopter3DGates", "Quadcopter3DGatesINDI", "zigzag_track", "square_track", "TRAIN_DISTURBANCE_RANGES",
           "default_residual_blob", "ShardedRaceEnv", "Quadcopter3DVec", "Quadcopter3DVecGates", "PPO", "VecMonitor",
           "evaluate_policy", "summarize_eval", "record_policy", "FlightRecord", "evaluate_policies", "rank_policies", "MfmaPolicyBank",
           "evaluate_grid", "Condition", "ConditionBank", "disturbance_sweep", "plan_condition_groups", "blackbox_policy", "CrashLog",
           "evaluate_q3_policy", "evaluate_q3_policies", "summarize_q3_eval", "PopulationPPO", "PBT", "EvolutionStrategy",
           "evaluate_dynamics_grid", "DynamicsParams", "DynamicsBank", "physical_sweep", "VehicleRanges",
           "evaluate_sensing_grid", "SensingParams", "SensingBank", "noise_sweep", "delay_sweep", "plan_sensor_mix",
           "blackbox_grid", "record_grid"]


def __getattr__(name):  # lazy: importing the package must not require torch / a GPU
    if name in ("Quadcopter3DGates", "Quadcopter3DGatesINDI", "default_residual_blob", "Box"):
        from . import vec_env

        return getattr(vec_env, name)
    if name in ("Quadcopter3DVec", "Quadcopter3DVecGates"):  # predecessor envs of "3D quad.ipynb"
        from . import quad3d

        return getattr(quad3d, name)
    if name in ("PPO", "VecMonitor"):  # SB3-shaped model object around the on-device PPO (R:783-831, R:3985-3996)
        from . import sb3

        return getattr(sb3, name)
    if name in ("evaluate_policy", "summarize_eval", "evaluate_policies", "rank_policies", "evaluate_grid", "evaluate_dynamics_grid", "evaluate_sensing_grid"):  # on-device lap times / crash rate of a policy (qr_evaluate_policy)
        from . import evaluation

        return getattr(evaluation, name)
    if name in ("evaluate_q3_policy", "evaluate_q3_policies", "summarize_q3_eval"):  # the same for the predecessor envs: how episodes end (q3_evaluate_policy)
        from . import evaluation

        return getattr(evaluation, name)
    if name in ("record_policy", "FlightRecord", "record_grid"):  # on-device flight recorder: the trajectory a policy flew (qr_record_policy; per grid cell: qr_blackbox_policy_grid)
        from . import recording

        return getattr(recording, name)
    if name in ("blackbox_policy", "CrashLog", "blackbox_grid"):  # on-device black box: the last steps before each crash (qr_blackbox_policy; per grid cell: qr_blackbox_policy_grid)
        from . import blackbox

        return getattr(blackbox, name)
    if name in ("Condition", "ConditionBank", "disturbance_sweep", "plan_condition_groups"):  # flight conditions of the grid evaluator (qr_condition_bank_*)
        from . import conditions

        return getattr(conditions, name)
    if name in ("DynamicsParams", "DynamicsBank", "physical_sweep", "VehicleRanges"):  # vehicles of the dynamics-grid evaluator (qr_dynamics_*)
        from . import dynamics

        return getattr(dynamics, name)
    if name in ("SensingParams", "SensingBank", "noise_sweep", "delay_sweep", "plan_sensor_mix"):  # sensors of the sensing-grid evaluator (qr_sensing_*) and of PPO(sensing=...)
        from . import sensing

        return getattr(sensing, name)
    if name == "MfmaPolicyBank":  # a bank of policies for one-launch evaluation (qr_policy_bank_*, qr_evaluate_policy_bank)
        from . import policy

        return policy.MfmaPolicyBank
    if name in ("PopulationPPO", "PBT"):  # P PPO learners on one env, one collect launch per round (qr_rollout_policy_population); PBT: their selection schedule
        from . import population

        return getattr(population, name)
    if name == "EvolutionStrategy":  # evolution strategies on the policy bank: optimise measured lap time and crash rate (qr_es_*)
        from . import es

        return es.EvolutionStrategy
    if name == "ShardedRaceEnv":
        from . import sharded

        return sharded.ShardedRaceEnv
    raise AttributeError(name)
