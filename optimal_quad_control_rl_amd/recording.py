"""On-device flight recorder: the trajectory a policy flew (`qr_record_policy`, csrc/quadrace_record.hip).

The third thing a user of the reference does with a trained policy, after reading lap times and watching it fly: log the flown
trajectory (the logging cell of the INDI notebook, I:666-695, writes world_states, the commanded actions and step_counts * dt per step
into an .npz that the analysis notebooks plot against real flights).  Here the closed loop runs in one kernel and one packed row per
env-step comes back:

    from optimal_quad_control_rl_amd import record_policy
    rec = record_policy(model, eval_env, n_steps=2000, envs=16, seed=99)
    rec.counts()                     # per-env gate passes, crashes, time-limit ends (the evaluator's definitions)
    rec.save_npz("flight.npz", 0)    # env 0 with the reference's keys: t x y z vx vy vz V phi theta psi u1 u2 u3 u4 u

One difference from the reference's logging cell: a row pairs the state with the command applied IN that state, at t = steps * dt; the
cell appends world_states AFTER env.step(actions), i.e. it pairs the state after the step with that command (and its t is one dt
later).  Shift `world` by one row to get the cell's pairing.
"""
import numpy as np

from ._closed_loop import _host, flying_policy, model_log_std

RECORD_EXTRA = 8   # QR_RECORD_EXTRA of include/quadrace.h
LOG_KEYS = ("t", "x", "y", "z", "vx", "vy", "vz", "V", "phi", "theta", "psi", "u1", "u2", "u3", "u4", "u")   # the reference's log_dict
END_RUNNING, END_CRASH, END_TIME_LIMIT = 0.0, 1.0, 2.0


class FlightRecord:
    """Host view of recorder rows [K][M][R] (float32; R = S + 8, S = 16 E2E / 13 INDI; layout in include/quadrace.h).
    Named views (no copies), all [K, M, ...]: world [.., S], command [.., 4], reward, end (0 running / 1 crash / 2 time limit), target
    (gate index before the step), steps (the env's step count before the step; 0 = first row of an episode), t = steps * dt."""

    def __init__(self, rows, dt, final_target=None):
        """final_target [M] (optional): the target gate of each env AFTER the last recorded step (qr_get_state), which stands in for the
        "next row" of the last row, so that a pass on the last step is seen; without it that step cannot show a pass."""
        rows = _host(rows)
        if rows.dtype != np.float32 or rows.ndim != 3 or rows.shape[2] - RECORD_EXTRA not in (13, 16):
            raise ValueError("rows must be float32 [K][M][S + %d] with S = 13 or 16, got %s %s" % (RECORD_EXTRA, rows.dtype, rows.shape))
        self.rows, self.dt = rows, np.float32(dt)
        self.state_len = s = rows.shape[2] - RECORD_EXTRA
        self.world, self.command = rows[:, :, :s], rows[:, :, s:s + 4]
        self.reward, self.end, self.target, self.steps = rows[:, :, s + 4], rows[:, :, s + 5], rows[:, :, s + 6], rows[:, :, s + 7]
        self.final_target = None
        if final_target is not None:
            self.final_target = _host(final_target).astype(np.float32).reshape(rows.shape[1])

    @property
    def num_steps(self):
        return self.rows.shape[0]

    @property
    def num_envs(self):
        return self.rows.shape[1]

    @property
    def t(self):
        return self.steps * self.dt

    def episodes(self, i):
        """Row ranges [(start, stop), ...] of env i's episodes: split after every row with end != 0; the last range is open (its
        episode was still running when the record stopped) unless the last row ended one."""
        cuts = (np.nonzero(self.end[:, i] != 0)[0] + 1).tolist()
        starts = [0] + cuts
        if starts[-1] == self.num_steps:
            starts.pop()
        return [(a, b) for a, b in zip(starts, cuts + [self.num_steps])] if self.num_steps else []

    def _passed(self):
        """bool [K or K - 1, M]: the step did not end the episode and the target gate after it differs"""
        if self.final_target is None:
            return (self.end[:-1] == 0) & (self.target[1:] != self.target[:-1])
        after = np.concatenate([self.target[1:], self.final_target[None, :]], axis=0)
        return (self.end == 0) & (after != self.target)

    def gate_passes(self, i):
        """Indices of the steps on which env i passed a gate -- the evaluator's definition: the step did not end the episode and the
        next row's target gate differs (for the record's last row: `final_target`, without which it cannot show a pass)."""
        return np.nonzero(self._passed()[:, i])[0]

    def counts(self):
        """int64 [M, 3]: per env gate passes, crashes, time-limit ends."""
        passes = self._passed().sum(axis=0)
        return np.stack([passes, (self.end == END_CRASH).sum(axis=0), (self.end == END_TIME_LIMIT).sum(axis=0)], axis=1).astype(np.int64)

    def _range(self, i, episode):
        if episode is None:
            return 0, self.num_steps
        return self.episodes(i)[episode]

    def log_dict(self, i, episode=None):
        """The reference's log_dict (I:672-686) for env i -- the whole record or one of episodes(i): t, x, y, z, vx, vy, vz,
        V = sqrt(vx^2 + vy^2 + vz^2), phi, theta, psi, u1..u4 = (command + 1) / 2, u = [u1 u2 u3 u4]; float32 throughout.  The state of
        a row is the one the command was applied IN (module docstring)."""
        a, b = self._range(i, episode)
        w, c = self.world[a:b, i], self.command[a:b, i]
        d = {"t": self.steps[a:b, i] * self.dt, "x": w[:, 0], "y": w[:, 1], "z": w[:, 2], "vx": w[:, 3], "vy": w[:, 4], "vz": w[:, 5]}
        d["V"] = np.sqrt(w[:, 3] ** 2 + w[:, 4] ** 2 + w[:, 5] ** 2)
        d["phi"], d["theta"], d["psi"] = w[:, 6], w[:, 7], w[:, 8]
        for k in range(4):
            d["u%d" % (k + 1)] = (c[:, k] + 1) / 2
        d["u"] = np.stack([d["u1"], d["u2"], d["u3"], d["u4"]], axis=1)
        assert tuple(d) == LOG_KEYS
        return d

    def save_npz(self, path, i, episode=None):
        """np.savez of log_dict(i, episode): opens in the reference's analysis cells."""
        np.savez(path, **self.log_dict(i, episode))
        return path


def record_policy(model, env, n_steps, envs=None, deterministic=True, seed=None, precision=None):
    """Fly `model`'s current policy on `env` (a race env of this package, possibly inside a VecMonitor) for `n_steps` in ONE kernel
    launch and return the FlightRecord of envs [0, envs) (None: all; every env flies either way).  `deterministic=False` samples
    actions with the model's log_std (noise keyed by `seed` or 0).  `seed`: reseed and reset the env first, so that a record and an
    evaluate_policy with the same seed see the same flights; None continues from the env's current state.  `precision` as in
    evaluate_policy.  `env` keeps flying from where the record left it."""
    with flying_policy(model, env, precision, seed) as (core, policy, precision, owner):
        rows = core.record_policy_device(policy, int(n_steps), model_log_std(owner), noise_seed=0 if seed is None else int(seed),
                                         deterministic=deterministic, rec_envs=envs, precision=precision)
        host = rows.cpu().numpy()
        final_target = core.get_state_tensors()[2][:host.shape[1]].cpu().numpy()
    return FlightRecord(host, core.dt, final_target)


def record_grid(policies, conditions, sensing, env, dynamics=None, envs_per_cell=256, n_steps=2000, rec_per_cell=None, precision=None, seed=0,
                noise_seed=0, command_history=0):
    """The flight recorder of evaluate_sensing_grid: blackbox_grid's launch with a black box that never freezes and a ring as long as the
    call (trigger 0, window = n_steps), so slot k holds the row of step k.  Returns records[p][c][s], each the FlightRecord [n_steps][M][R]
    of the first `rec_per_cell` envs of that cell (None: all), with `.evaluation` = summarize_eval of the cell over the same steps.  Rows
    hold the TRUE state before the step and the command FLOWN, as blackbox_grid's."""
    from .blackbox import fly_grid_cells

    def make(ring, status, terminal, evaluation, dt):
        record = FlightRecord(ring, dt)
        record.evaluation = evaluation
        return record

    return fly_grid_cells(policies, conditions, sensing, env, dynamics, envs_per_cell, n_steps, int(n_steps), 0, rec_per_cell, precision, seed,
                          noise_seed, command_history, make)
