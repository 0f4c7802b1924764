"""On-device black box: the last steps before each crash (`qr_blackbox_policy`, csrc/quadrace_blackbox.hip).

The question that follows every evaluation -- why does the policy crash, and where?  All N envs fly closed-loop in one kernel; each
keeps only its last `window` recorder rows in a ring and stops overwriting them when its episode ends the way `trigger` says:

    from optimal_quad_control_rl_amd import blackbox_policy
    log = blackbox_policy(model, eval_env, n_steps=2000, window=64, trigger="crash", seed=99)
    log.by_gate()                    # crash counts per cause x target gate of the trigger row
    log.flight(int(log.frozen_envs()[0]))   # that env's last rows, oldest -> newest, ending at the row that crashed
    log.save_npz("crashes.npz")

Rows have the flight recorder's layout (recording.FlightRecord; include/quadrace.h): a row pairs the state with the command applied IN
that state, so the trigger row is the state and command of the step that ended the episode; `terminal_state` is the state that step
produced (after the integration, before the auto-reset).
"""
import numpy as np

from ._closed_loop import _host, flying_policy, model_log_std

from .recording import RECORD_EXTRA, FlightRecord

ST_INTS = 4   # QR_BLACKBOX_ST_INTS of include/quadrace.h
TRIGGERS = {"none": 0, "crash": 1, "time_limit": 2, "any": 3}   # QR_BLACKBOX_ON_CRASH | QR_BLACKBOX_ON_TIME_LIMIT
CAUSE_GROUND, CAUSE_OOB, CAUSE_TIME_LIMIT, CAUSE_GATE = 1, 2, 4, 8
CAUSE_NAMES = ((CAUSE_GROUND, "ground"), (CAUSE_OOB, "out_of_bounds"), (CAUSE_GATE, "gate"), (CAUSE_TIME_LIMIT, "time_limit"))


class CrashLog:
    """Host view of a black-box ring [W][M][R] (float32, recorder rows), its status [M][4] (int32) and the terminal states [M][S] or None,
    after calls that covered steps first_step .. last_step (the absolute step index of the last call's last step)."""

    def __init__(self, ring, status, terminal, last_step, dt, evaluation=None):
        """evaluation (optional; blackbox_grid): summarize_eval's dict of the flight the log was taken from"""
        self.evaluation = evaluation
        ring, status = _host(ring), _host(status)
        if ring.dtype != np.float32 or ring.ndim != 3 or ring.shape[2] - RECORD_EXTRA not in (13, 16):
            raise ValueError("ring must be float32 [W][M][S + %d] with S = 13 or 16, got %s %s" % (RECORD_EXTRA, ring.dtype, ring.shape))
        if status.dtype != np.int32 or status.shape != (ring.shape[1], ST_INTS):
            raise ValueError("status must be int32 [M][%d] with the ring's M, got %s %s" % (ST_INTS, status.dtype, status.shape))
        self.ring, self.status, self.dt = ring, status, np.float32(dt)
        self.window, self.num_envs, self.row_len = ring.shape
        self.state_len = self.row_len - RECORD_EXTRA
        self.last_step = int(last_step)
        self.terminal = None
        if terminal is not None:
            terminal = _host(terminal)
            if terminal.dtype != np.float32 or terminal.shape != (self.num_envs, self.state_len):
                raise ValueError("terminal must be float32 [M][S], got %s %s" % (terminal.dtype, terminal.shape))
            self.terminal = terminal

    # ---- status
    @property
    def frozen(self):
        """bool [M]: the env's window is frozen at a trigger row"""
        return self.status[:, 0] != 0

    def frozen_envs(self):
        return np.nonzero(self.frozen)[0]

    @property
    def valid(self):
        """int [M]: number of valid rows of each env, min(rows stored, W)"""
        return np.minimum(self.status[:, 1], self.window).astype(np.int64)

    @property
    def cause(self):
        """int32 [M]: cause bits of the trigger step (1 ground, 2 out of bounds, 4 time limit, 8 gate collision), 0 for armed envs"""
        return self.status[:, 3]

    @property
    def terminal_state(self):
        """float32 [M][S]: the world state at the end of each frozen env's trigger step (NaN rows for armed envs), or None"""
        if self.terminal is None:
            return None
        out = self.terminal.copy()
        out[~self.frozen] = np.nan
        return out

    # ---- rows
    def slots(self, i):
        """Ring slots of env i's valid rows, oldest first: they end at the trigger slot if the env is frozen, at the last flown step's
        slot if it is still armed."""
        n, w = int(self.valid[i]), self.window
        end = int(self.status[i, 2]) if self.status[i, 0] else self.last_step % w
        return [(end - n + 1 + j) % w for j in range(n)]

    def flight(self, i):
        """float32 [valid[i]][R]: env i's rows oldest -> newest, unrolled from the ring"""
        return self.ring[self.slots(i), i]

    def flights(self):
        """(rows [m][W][R] NaN-padded at the end, valid [m], envs [m]) for the m frozen envs"""
        envs = self.frozen_envs()
        out = np.full((len(envs), self.window, self.row_len), np.nan, np.float32)
        for j, i in enumerate(envs):
            f = self.flight(i)
            out[j, :len(f)] = f
        return out, self.valid[envs], envs

    def trigger_rows(self):
        """float32 [m][R]: the trigger row of each frozen env (frozen_envs() order)"""
        envs = self.frozen_envs()
        return self.ring[self.status[envs, 2], envs]

    def as_flight_record(self, i):
        """FlightRecord of env i's rows alone ([valid][1][R]): its named views and log_dict"""
        return FlightRecord(np.ascontiguousarray(self.flight(i)[:, None, :]), self.dt)

    # ---- tables
    def cause_counts(self):
        """{name: number of frozen envs with that cause bit} for ground, out_of_bounds, gate, time_limit (an end can carry two bits)"""
        c = self.cause[self.frozen]
        return {name: int(((c & bit) != 0).sum()) for bit, name in CAUSE_NAMES}

    def by_gate(self, num_gates=None):
        """int64 [4][G]: frozen envs per cause (rows: ground, out_of_bounds, gate, time_limit) x target gate of the trigger row"""
        rows = self.trigger_rows()
        gate = rows[:, self.state_len + 6].astype(np.int64) if len(rows) else np.zeros(0, np.int64)
        g = int(num_gates) if num_gates is not None else (int(gate.max()) + 1 if len(gate) else 0)
        c = self.cause[self.frozen]
        out = np.zeros((len(CAUSE_NAMES), g), np.int64)
        for r, (bit, _) in enumerate(CAUSE_NAMES):
            np.add.at(out[r], gate[(c & bit) != 0], 1)
        return out

    def save_npz(self, path):
        """ring, status, terminal (if kept), last_step, dt, and the unrolled flights of the frozen envs (flights, valid, envs)"""
        rows, valid, envs = self.flights()
        d = dict(ring=self.ring, status=self.status, last_step=np.int64(self.last_step), dt=self.dt, flights=rows, valid=valid, envs=envs)
        if self.terminal is not None:
            d["terminal"] = self.terminal
        np.savez(path, **d)
        return path


def blackbox_policy(model, env, n_steps, window=64, trigger="crash", rec_envs=None, deterministic=True, seed=None, precision=None):
    """Fly `model`'s current policy on `env` (as record_policy: a race env of this package, possibly inside a VecMonitor; an SB3-style
    model or the native trainer) for `n_steps` in ONE kernel launch and return the CrashLog of envs [0, rec_envs) (None: all): each
    env's last `window` rows, frozen at the first step that ends an episode by `trigger` ("crash", "time_limit", "any"; "none" never
    freezes).  `deterministic`, `seed`, `precision` as in record_policy.  `env` keeps flying from where the call left it."""
    if trigger not in TRIGGERS:
        raise ValueError("trigger must be one of %s, got %r" % (sorted(TRIGGERS), trigger))
    with flying_policy(model, env, precision, seed) as (core, policy, precision, owner):
        ring, st, term = core.blackbox_policy_device(policy, int(n_steps), model_log_std(owner), window=int(window), trigger=TRIGGERS[trigger],
                                                     noise_seed=0 if seed is None else int(seed), deterministic=deterministic,
                                                     rec_envs=rec_envs, precision=precision)
        ring, st, term = ring.cpu().numpy(), st.cpu().numpy(), term.cpu().numpy()
    return CrashLog(ring, st, term, int(n_steps) - 1, core.dt)


def cell_columns(ring, status, terminal, group, rec_per_group):
    """The columns of group `group` in the buffers of qr_blackbox_policy_grid: env g E + j, j < M = rec_per_group, owns column g M + j of
    ring [W][G M][R], status [G M][4] and terminal [G M][S] (or None).  Returns contiguous copies (ring [W][M][R], status [M][4],
    terminal [M][S] or None) of host arrays."""
    g, m = int(group), int(rec_per_group)
    ring, status = _host(ring), _host(status)
    if m < 1 or g < 0 or (g + 1) * m > ring.shape[1] or status.shape[0] != ring.shape[1]:
        raise ValueError("group %d of %d columns each lies outside ring %s / status %s" % (g, m, ring.shape, status.shape))
    cols = slice(g * m, (g + 1) * m)
    term = None if terminal is None else np.ascontiguousarray(_host(terminal)[cols])
    return np.ascontiguousarray(ring[:, cols]), np.ascontiguousarray(status[cols]), term


def fly_grid_cells(policies, conditions, sensing, env, dynamics, envs_per_cell, n_steps, window, trigger, rec_per_cell, precision, seed, noise_seed,
                   command_history, make):
    """The launches of blackbox_grid / record_grid: evaluate_sensing_grid's banks, starts and batching with ONE phase of n_steps through
    env.blackbox_grid_device; make(ring, status, terminal, evaluation) [one cell's columns, host arrays] -> logs[p][c][s]."""
    import torch

    from ._closed_loop import fly_batches, group_size
    from .conditions import ConditionBank
    from .dynamics import DynamicsBank
    from .evaluation import REC_FLOATS, REC_INTS, _as_actor, _model_precision, _sync_and_close, check_command_history, plan_dynamics_batches, summarize_eval
    from .policy import MfmaPolicyBank
    from .sb3 import _unwrap
    from .sensing import QUEUE_FLOATS, SensingBank

    core = _unwrap(env)
    H = check_command_history(command_history, core.gates_ahead)
    E, slots = group_size(envs_per_cell, core.num_envs, "envs_per_cell", "cell")
    n_steps, window = int(n_steps), int(window)
    M = E if rec_per_cell is None else int(rec_per_cell)
    if n_steps < 1 or window < 1 or not 1 <= M <= E:
        raise ValueError("need n_steps >= 1, window >= 1 and 1 <= rec_per_cell <= envs_per_cell")
    conditions, policies, sensing = list(conditions), list(policies), list(sensing)
    plan = plan_dynamics_batches(len(policies), len(conditions), len(sensing), slots)   # cells (policy, condition, sensor)
    if dynamics is not None and dynamics.variant != core.VARIANT:
        raise ValueError("DynamicsParams of another variant than the env")
    actors = [_as_actor(p) for p in policies]
    if precision is None:
        precision = _model_precision([m for _, m in actors])
    logs = [[[None] * len(sensing) for _ in conditions] for _ in actors]
    pbank = MfmaPolicyBank(core.state_len + 4 * H, len(actors), core.device.index)
    cbank = ConditionBank(core.VARIANT, len(conditions), core.device.index)
    dbank = DynamicsBank(core.VARIANT, 1, core.device.index)
    sbank = SensingBank(len(sensing), core.device.index)
    pending = torch.zeros((core.num_envs, QUEUE_FLOATS), dtype=torch.float32, device=core.device)
    box = [None]   # the batch's (ring, status, terminal) on the host

    def start(cells):
        core.condition_starts(conditions, [c for _, c, _ in cells], E, seed=seed)
        pending.zero_()

    def launch(cells, steps, rec, recf):
        maps = ([p for p, _, _ in cells], [c for _, c, _ in cells], [0] * len(cells), [s for _, _, s in cells])
        out = core.blackbox_grid_device(pbank, cbank, dbank, sbank, *maps, H, E, steps, pending, rec, recf, precision=precision,
                                        noise_seed=noise_seed, first_step=0, window=window, trigger=trigger, rec_per_group=M)
        box[0] = tuple(t.cpu().numpy() for t in out[2:])

    def summarise(cell, rec, recf):
        return summarize_eval(rec, recf, core.dt, conditions[cell[1]].gates_per_lap)

    try:
        for p, (actor, _) in enumerate(actors):
            pbank.load_torch(p, actor)
        for c, cond in enumerate(conditions):
            cbank.set(c, cond)
        dbank.set(0, dynamics)
        for s, sen in enumerate(sensing):
            sbank.set(s, sen)
        # one batch at a time: the batch's buffers are split into its cells before the next batch overwrites them
        for members, kept in plan:
            flown = fly_batches([(members, kept)], start, launch, [n_steps], (REC_INTS, REC_FLOATS), summarise, core.num_envs, E, core.device)
            for g, ((p, c, s), summaries) in enumerate(flown):
                logs[p][c][s] = make(*cell_columns(*box[0], g, M), summaries[0], core.dt)
    finally:
        _sync_and_close(core, pbank, cbank, dbank, sbank)
    return logs


def blackbox_grid(policies, conditions, sensing, env, dynamics=None, envs_per_cell=256, n_steps=2000, window=64, trigger="crash", rec_per_cell=None,
                  precision=None, seed=0, noise_seed=0, command_history=0):
    """The black box of evaluate_sensing_grid (qr_blackbox_policy_grid): every cell of `policies` x `conditions` x `sensing` flies exactly
    what that evaluator flies -- its starts, restarts and noise draws, deterministic actions, the vehicle `dynamics`, the optional
    `command_history` -- for `n_steps` in one launch per `env.num_envs // envs_per_cell` cells, and the first `rec_per_cell` envs of each
    cell (None: all) keep their last `window` rows, frozen by `trigger` as in blackbox_policy.  A row holds the TRUE state before the step
    and the command FLOWN (under a delay, the one computed that many steps earlier; zeros at an episode's start).  Returns logs[p][c][s],
    each a CrashLog of that cell's columns whose `.evaluation` is summarize_eval of the cell over the same n_steps: the dict
    evaluate_sensing_grid(..., n_eval_steps=n_steps, window_steps=n_steps) returns as "total"."""
    if trigger not in TRIGGERS:
        raise ValueError("trigger must be one of %s, got %r" % (sorted(TRIGGERS), trigger))
    last = int(n_steps) - 1

    def make(ring, status, terminal, evaluation, dt):
        return CrashLog(ring, status, terminal, last, dt, evaluation=evaluation)

    return fly_grid_cells(policies, conditions, sensing, env, dynamics, envs_per_cell, n_steps, window, TRIGGERS[trigger], rec_per_cell, precision,
                          seed, noise_seed, command_history, make)
