"""Case tables for the predecessor envs at their edges (Quadcopter3DVec / Quadcopter3DVecGates; oracle/quad3d_oracle.c is the
statement they are built against).  Plain NumPy, no GPU: tests/test_q3_edges_host.py runs them through the oracle alone and asserts
that every row ends the way it was built to; tests/test_gpu_q3_edges.py runs the same rows through the HIP kernels.

    circle_track(G)            tracks of any length with distinct rows and yaws that are no multiple of pi/2
    pass_table(track)          per gate: one env through the centre of the gate, one 0.6 m above the window
    threshold_tables()         one triple (on the threshold, one ulp to either side) per strict comparison of step_wait, the override
                               order, and every one of them again on the last step before the time limit
    nonfinite_table(kind)      NaN / +inf / -inf in every state and action column, and finite actions far outside [-1, 1]

Why the on-threshold rows are exact.  Hover tests the state AFTER the Euler step, so a tested column must survive the step unchanged:
its derivative is exactly zero (x with vx = 0; phi, theta with p = q = r = 0; p, q with equal rotor speeds, equal actions and vy = vx =
0 -- the four rotor terms of f_func then cancel in the order they are summed: ((a - a) - a) + a and ((a + a) - a) - a).  r is left
out: its derivative holds -0.3958 r, which is never zero for r != 0.  The velocity threshold is left out as well (gravity changes vz in
every step); the tables set it to 50 so that it never decides.  Gates tests ground and bounds on the state BEFORE the step, which is
injected bit for bit, and the plane / window on p_new - gate: the gate used for those rows sits at the origin with yaw 0 (normal exactly
(1, 0), differences exact), and x_new = x + float32(dt) * vx is exact for the values chosen (checked in the host test)."""
import numpy as np

X, Y, Z, VX, VY, VZ, PHI, THETA, PSI, P, Q, R, W1 = range(13)
PI = 3.141592653589793

# ---- tracks ------------------------------------------------------------------------------------------------------------------------
TRACK_SIZES = (1, 2, 31, 32)


def circle_track(G, radius=5.0, z=-1.5):
    """G gates on a spiral inside the 6 m circle at z = -1.5: every row differs from every other in x, y and yaw."""
    k = np.arange(G, dtype=np.float64)
    ang = 2.0 * np.pi * (k + 0.37) / G
    r = radius - 0.9 * k / max(G - 1, 1)
    gp = np.stack([r * np.cos(ang), r * np.sin(ang), np.full(G, z)], axis=1).astype(np.float32)
    gy = (ang + np.pi / 2 + 0.2 + 0.003 * k).astype(np.float32)      # roughly along the direction of flight
    sp = np.array([0.3, -0.2, z], np.float32)
    return gp, gy, sp


def gate_normals(gate_yaw):
    """cos / sin of the float32 yaw in float32, as the oracle's cosf / sinf (to within NumPy's own ulp: only used to PLACE envs)."""
    y = np.asarray(gate_yaw, np.float32)
    return np.cos(y).astype(np.float32), np.sin(y).astype(np.float32)


def pass_table(track):
    """Two envs per gate g, target g, 5 mm before the gate plane at 1 m/s along the normal (dt = 0.01: 5 mm behind it afterwards):
    row 2 g on centre (passes), row 2 g + 1 0.6 m above the centre (collides).  -> states [2G,16] f32, target, steps, actions, passes"""
    gp, gy, _ = track
    G = gp.shape[0]
    n0, n1 = gate_normals(gy)
    st = np.zeros((2 * G, 16), np.float32)
    tg = np.repeat(np.arange(G, dtype=np.int32), 2)
    for g in range(G):
        for j, dz in enumerate((0.0, -0.6)):
            row = st[2 * g + j]
            row[X], row[Y], row[Z] = gp[g, 0] - 0.005 * n0[g], gp[g, 1] - 0.005 * n1[g], gp[g, 2] + dz
            row[VX], row[VY] = n0[g], n1[g]
    rng = np.random.default_rng(11)
    act = (0.1 * rng.uniform(-1, 1, size=(2 * G, 4))).astype(np.float32)
    passes = np.arange(2 * G) % 2 == 0
    return st, tg, np.zeros(2 * G, np.int32), act, passes


# ---- exact-threshold tables ----------------------------------------------------------------------------------------------------------
EDGE_ACTION = 0.25          # every row flies (0.25, 0.25, 0.25, 0.25): a constant policy can command it in the closed-loop kernels
EDGE_MAX_STEPS = 7
EDGE_DT = 0.01
HOVER_EDGE_THR = (0.25, 50.0, 0.125, 0.125)     # exactly representable; vel = 50 keeps gravity out
HOVER_WIDE_THR = (0.25, 50.0, 4.0, 0.125)       # an angle threshold beyond pi: goal and out of bounds can hold together


def edge_track():
    """gate 0 at the origin (plane / window rows: differences exact), gate 1 and the final gate 2 at z = +0.2 (override rows: the
    window reaches below the ground plane z = 0; z points down); all yaws 0."""
    gp = np.array([[0.0, 0.0, 0.0], [3.0, 1.5, 0.2], [-3.0, -1.5, 0.2]], np.float32)
    return gp, np.zeros(3, np.float32), np.array([1.5, 0.75, -1.0], np.float32)


class Table:
    """Rows of one env kind with the outcome each was built for.
        done, trunc     bool
        reward          the exact value where step_wait overrides it (100, -1, 10, -10), NaN where it is the shaping term
        target_after    gates, rows that live: the target after the step
        cause           None (lives) or "success" / "timeout" / "oob" / "ground" / "collision" (tests/q3_eval_spec.py's classes)
        triples         (name, (i_below, i_on, i_above)): a threshold row and its two neighbours"""

    def __init__(self, kind, thresholds=None, track=None):
        self.kind, self.thresholds, self.track = kind, thresholds, track
        self.dtype = np.float64 if kind == "hover" else np.float32
        self.names, self._rows, self._tg, self._sc = [], [], [], []
        self._done, self._trunc, self._rew, self._tga, self.cause = [], [], [], [], []
        self.triples = []

    def add(self, name, row, target=0, steps=0, cause=None, reward=np.nan, target_after=-1):
        row = np.asarray(row, self.dtype)
        assert row.shape == (16,)
        limit = steps + 1 >= EDGE_MAX_STEPS
        if self.kind == "hover":
            trunc = limit or cause == "oob"
            if limit:
                cause = "timeout"                      # hover: a goal on the last step is truncated, hence no SUCCESS
        else:
            trunc = limit
            if limit and cause != "success":
                cause = "timeout"
        if cause is not None:
            target_after = -1                          # the reset replaces the target
        self.names.append(name); self._rows.append(row); self._tg.append(target); self._sc.append(steps)
        self._done.append(cause is not None); self._trunc.append(bool(trunc)); self._rew.append(reward)
        self._tga.append(target_after); self.cause.append(cause)
        return len(self.names) - 1

    def add_both(self, name, row, **kw):
        """The row, and the same row on the last step before the time limit."""
        i = self.add(name, row, steps=0, **kw)
        self.add(name + "+limit", row, steps=EDGE_MAX_STEPS - 1, **kw)
        return i

    def finish(self):
        self.states = np.stack(self._rows)
        self.target = np.asarray(self._tg, np.int32)
        self.steps = np.asarray(self._sc, np.int32)
        self.done, self.trunc = np.asarray(self._done, bool), np.asarray(self._trunc, bool)
        self.reward, self.target_after = np.asarray(self._rew, np.float64), np.asarray(self._tga, np.int32)
        self.n = len(self.names)
        self.actions = np.full((self.n, 4), EDGE_ACTION, np.float32)
        return self


def _ulp_triple(v, dtype):
    """(towards zero, v, away from zero) in `dtype`."""
    v = dtype(v)
    big = dtype(np.inf) if v > 0 else dtype(-np.inf)
    return np.nextafter(v, dtype(0), dtype=dtype), v, np.nextafter(v, big, dtype=dtype)


def hover_edge_table():
    t = Table("hover", thresholds=HOVER_EDGE_THR)
    z = np.zeros(16)

    def triple(name, col, value, base, outcomes):
        idx = []
        for v, (cause, reward) in zip(_ulp_triple(value, np.float64), outcomes):
            row = base.copy(); row[col] = v
            idx.append(t.add_both(name, row, cause=cause, reward=reward))
        t.triples.append((name, tuple(idx)))

    alive, oob, goal = (None, np.nan), ("oob", -1.0), ("success", 100.0)
    # out of bounds: fabs(.) > 10 and fabs(.) > pi are strict, so the threshold itself stays inside
    for col, nm in ((X, "x"), (Y, "y"), (Z, "z")):
        for sgn in (1.0, -1.0):
            triple(f"{nm}={sgn * 10:+.0f}", col, sgn * 10.0, z, (alive, alive, oob))
    for col, nm in ((PHI, "phi"), (THETA, "theta")):
        for sgn in (1.0, -1.0):
            triple(f"{nm}={'+' if sgn > 0 else '-'}pi", col, sgn * PI, z, (alive, alive, oob))
    # goal: every comparison is a strict <, so the threshold itself is outside
    for col, nm in ((X, "x"), (Y, "y"), (Z, "z")):
        for sgn in (1.0, -1.0):
            triple(f"|pos| {nm}={sgn * 0.25:+.2f}", col, sgn * 0.25, z, (goal, alive, alive))
    for col, nm in ((PHI, "phi"), (THETA, "theta"), (PSI, "psi"), (P, "p"), (Q, "q")):
        for sgn in (1.0, -1.0):
            triple(f"{nm}={sgn * 0.125:+.3f}", col, sgn * 0.125, z, (goal, alive, alive))
    t.add_both("goal at the origin", z, cause="success", reward=100.0)
    far = z.copy(); far[X] = 1.0
    t.add_both("calm, 1 m away", far)
    return t.finish()


def hover_wide_table():
    """ang_threshold = 4 > pi: |phi| in (pi, 4) is a goal AND out of bounds; the later override wins (reward -1, truncated)."""
    t = Table("hover", thresholds=HOVER_WIDE_THR)
    z = np.zeros(16)
    for col, nm in ((PHI, "phi"), (THETA, "theta")):
        for v in (3.5, -3.5):
            row = z.copy(); row[col] = v
            t.add_both(f"goal and oob, {nm}={v}", row, cause="oob", reward=-1.0)
        row = z.copy(); row[col] = 3.0
        t.add_both(f"goal alone, {nm}=3", row, cause="success", reward=100.0)
    row = z.copy(); row[X] = 1.0; row[PHI] = 3.5
    t.add_both("oob alone, phi=3.5", row, cause="oob", reward=-1.0)
    return t.finish()


def _f32_dt_times(v):
    return np.float32(np.float32(EDGE_DT) * np.float32(v))


def _x_reaching(nx_target, vx):
    """x (float32) with x + float32(dt) * vx == nx_target exactly, and the nearest x on either side whose x_new differs."""
    step = _f32_dt_times(vx)
    x = np.float32(np.float32(nx_target) - step)
    assert np.float32(x + step) == np.float32(nx_target)
    lo, hi = x, x
    for _ in range(16):
        lo = np.nextafter(lo, np.float32(-np.inf))
        if np.float32(lo + step) != np.float32(nx_target):
            break
    for _ in range(16):
        hi = np.nextafter(hi, np.float32(np.inf))
        if np.float32(hi + step) != np.float32(nx_target):
            break
    assert np.float32(lo + step) < np.float32(nx_target) < np.float32(hi + step)
    return lo, x, hi


def gates_edge_table():
    trk = edge_track()
    gp = trk[0]
    t = Table("gates", track=trk)
    f32 = np.float32
    calm = np.zeros(16, np.float32)
    calm[X], calm[Y], calm[Z] = 1.5, 0.75, -1.0          # behind gate 0's plane, at rest: no crossing, nothing else either

    def rows(name, make, values, outcomes, target=0, as_triple=True):
        idx = []
        for v, (cause, reward, tga) in zip(values, outcomes):
            idx.append(t.add_both(name, make(v), target=target, cause=cause, reward=reward, target_after=tga))
        if as_triple:
            t.triples.append((name, tuple(idx)))

    def setcol(base, col):
        def make(v):
            row = base.copy(); row[col] = v
            return row
        return make

    stay, ground, oob = (None, np.nan, 0), ("ground", -10.0, -1), ("oob", np.nan, -1)
    passed, collision = (None, np.nan, 1), ("collision", -10.0, -1)
    tiny = np.nextafter(f32(0), f32(1))                    # the smallest subnormal
    # ---- pre-step predicates: ground z > 0, bounds |x|, |y| > 10 and |p|, |q|, |r| > 1000
    rows("z in (-0, +0, subnormal)", setcol(calm, Z), (f32(-0.0), f32(0.0), tiny), (stay, stay, ground))
    for col, nm, lim in ((X, "x", 10.0), (Y, "y", 10.0), (P, "p", 1000.0), (Q, "q", 1000.0), (R, "r", 1000.0)):
        for sgn in (1.0, -1.0):
            rows(f"{nm}={sgn * lim:+.0f}", setcol(calm, col), _ulp_triple(sgn * lim, f32), (stay, stay, oob))
    # ---- the plane of gate 0 (origin, normal (1, 0)): crossed = proj_old < 0 and proj_new > 0, at vx = 1 m/s, inside the window
    fly = np.zeros(16, np.float32)
    fly[VX], fly[Z] = 1.0, -0.25
    rows("proj_old in (-0.005, -subnormal, 0)", setcol(fly, X), (f32(-0.005), -tiny, f32(0.0)), (passed, passed, stay))
    rows("proj_old = -0", setcol(fly, X), (f32(-0.0),), (stay,), as_triple=False)
    lo, on, hi = _x_reaching(0.0, 1.0)
    rows("proj_new in (<0, 0, >0)", setcol(fly, X), (lo, on, hi), (stay, stay, passed))
    # ---- the 0.5 m window: inside = every |.| < 0.5, outside = any |.| > 0.5; exactly 0.5 is crossed and neither
    near = fly.copy(); near[X] = -0.005
    for sgn in (1.0, -1.0):
        rows(f"y-gy={sgn * 0.5:+.1f}", setcol(near, Y), _ulp_triple(sgn * 0.5, f32), (passed, stay, collision))
    rows("z-gz=-0.5", setcol(near, Z), _ulp_triple(-0.5, f32), (passed, stay, collision))
    fast = fly.copy(); fast[VX] = 64.0                     # float32(dt) * 64 is exact: x_new = 0.5 exactly, crossing from x < 0
    lo, on, hi = _x_reaching(0.5, 64.0)
    rows("x_new-gx=0.5", setcol(fast, X), (lo, on, hi), (passed, stay, collision))
    # ---- override order: collision -> ground -> final pass (reward), bounds without an override; gates 1 and 2 at z = +0.2
    def at(g, dy=0.0, z=-0.1, p=0.0):
        row = np.zeros(16, np.float32)
        row[X], row[Y], row[Z], row[VX], row[P] = gp[g, 0] - f32(0.005), gp[g, 1] + f32(dy), z, 1.0, p
        return row
    G = gp.shape[0]
    one = lambda name, row, target, out: rows(name, lambda v: row, (0,), (out,), target=target, as_triple=False)
    one("pass alone", at(1), 1, (None, np.nan, 2))
    one("collision alone", at(1, dy=0.6), 1, collision)
    one("final pass alone", at(2), G - 1, ("success", 10.0, -1))
    one("collision and ground", at(1, dy=0.6, z=0.1), 1, ground)
    one("pass and ground", at(1, z=0.1), 1, ground)
    one("final pass and ground", at(2, z=0.1), G - 1, ("success", 10.0, -1))
    one("oob at rest", setcol(calm, P)(1001.0), 1, oob)                   # no crossing: the shaping reward stays, the env ends
    one("oob and pass", at(1, p=1001.0), 1, oob)                          # the shaping reward stays too
    one("oob and collision", at(1, dy=0.6, p=1001.0), 1, ("oob", -10.0, -1))
    one("oob and final pass", at(2, p=1001.0), G - 1, ("success", 10.0, -1))
    one("oob and ground", at(1, z=0.1, p=1001.0), 1, ground)
    # z = +0 is NOT the ground (strict >): an env that ends there ends for its other reason (the evaluator restates the predicate)
    one("oob on the plane z=+0", at(1, z=0.0, p=1001.0), 1, oob)
    one("collision on the plane z=+0", at(1, dy=0.6, z=0.0), 1, collision)
    return t.finish()


def threshold_tables():
    return {"hover": hover_edge_table(), "hover_wide": hover_wide_table(), "gates": gates_edge_table()}


# ---- NaN, infinities, actions outside [-1, 1] ------------------------------------------------------------------------------------------
NONFINITE_MAX_STEPS = 3


def nonfinite_table(kind, track=None):
    """16 x 3 + 4 x 3 + 8 rows on a calm base state -> (states, target, steps, actions)."""
    dtype = np.float64 if kind == "hover" else np.float32
    n = 16 * 3 + 4 * 3 + 8
    rng = np.random.default_rng(5)
    st = (0.2 * rng.uniform(-1, 1, size=(n, 16))).astype(dtype)
    st[:, Z] -= 1.0
    act = (0.5 * rng.uniform(-1, 1, size=(n, 4))).astype(np.float32)
    bad = (np.nan, np.inf, -np.inf)
    i = 0
    for col in range(16):
        for v in bad:
            st[i, col] = v
            i += 1
    for col in range(4):
        for v in bad:
            act[i, col] = v
            i += 1
    for v in (3.0, -3.0, 1e6, -1e6):
        act[i] = v
        act[i + 1, i % 4] = v
        i += 2
    assert i == n
    G = 1 if track is None else track[0].shape[0]
    tg = (np.arange(n) % G).astype(np.int32)
    return st, tg, np.zeros(n, np.int32), act


# ---- the oracle, configured --------------------------------------------------------------------------------------------------------
def oracle_env(kind, n, track=None, thresholds=None, max_steps=None, dt=0.01, **kw):
    from oracle import quad3d as q3

    o = q3.Quad3DOracle(q3.HOVER, n, **kw) if kind == "hover" else q3.Quad3DOracle(q3.GATES, n, *track, **kw)
    if max_steps is not None:
        o.set_limits(max_steps, dt)
    if thresholds is not None:
        o.set_thresholds(*thresholds)
    return o


def oracle_trace(o, states, target, steps, actions, force_steps=False):
    """Inject (states, target, steps) and step the oracle freely through actions [K,N,4] -> dict of [K, ...] arrays: the state, target
    and step counter before and after every step, reward, done, trunc.  force_steps: every env's step counter is set to k before step
    k, whatever happened to it (an env that was reset early still meets the time limit together with the others)."""
    o.states[:] = states
    if target is not None:
        o.target[:] = target
    o.steps[:] = steps
    keys = ("pre_states", "pre_target", "pre_steps", "states", "target", "steps", "rew", "done", "trunc")
    out = {k: [] for k in keys}
    for k, a in enumerate(np.asarray(actions, np.float32)):
        if force_steps:
            o.steps[:] = k
        out["pre_states"].append(o.states.copy()); out["pre_target"].append(o.target.copy()); out["pre_steps"].append(o.steps.copy())
        st, rew, done, trunc = o.step(a)
        out["states"].append(st); out["rew"].append(rew); out["done"].append(done); out["trunc"].append(trunc)
        out["target"].append(o.target.copy()); out["steps"].append(o.steps.copy())
    return {k: np.stack(v) for k, v in out.items()}
