"""The equations of motion as a function of their coefficient TABLE, in float64 NumPy: one forward-Euler step of both variants, the
folding of the physical parameters into the table, and the injected states the host and GPU tests of the dynamics grid share.
Written from the mathematics of R:57-152 / I:43-110 (R = "3D quad race.ipynb", I = "3D quad race INDI inner loop.ipynb"; SURVEY
Appendix A, table layout: include/quadrace.h); tests/test_gpu_dynamics_grid.py holds eval_policy_dynamics_grid_kernel against it and
tests/test_dynamics_host.py holds it against the C oracle at nominal coefficients.  A plain module: nothing at import, no GPU."""
import numpy as np

E2E, INDI = 0, 1
COUNT = {E2E: 22, INDI: 12}
DT = float(np.float32(0.01))          # the step the kernels take: float32(0.01) (R:346, 512)
# biases of the constant-action policy: distinct components, exact in f16 (so every precision of the policy forward returns them)
ACTION = {E2E: (0.25, -0.125, 0.5, 0.375), INDI: (0.25, -0.125, 0.5, 0.375)}
STATE_SEED = 20
PERTURB = 1.25
# The float32 C oracle's one step against step() below at nominal coefficients, on injected_states(): the measured maxima of
# parity.rel_err (tests/test_dynamics_host.py prints and bounds them) are 5.272e-7 for E2E -- in p, whose derivative holds the difference
# of four squared rotor speeds of 1e8 -- and 1.198e-7 for INDI; held here rounded up in the third digit.
ORACLE_ERR = {E2E: 5.28e-7, INDI: 1.20e-7}


def tolerance(variant):
    """parity.rel_err bound of the kernel's one step against step(): the project's teacher-forced one-step bound of 1e-6,
    or four times the oracle's own error against this restatement where that error exceeds a quarter of it; never above the project's
    1e-5 state bound.  E2E: 4 x 5.28e-7 = 2.112e-6; INDI: 1e-6."""
    m = ORACLE_ERR[variant]
    return min(1e-5, 1e-6 if m <= 0.25e-6 else 4.0 * m)


def rotation(phi, theta, psi):
    """body -> world, ZYX Euler (R:97-100): rows as tuples of arrays"""
    sph, cph, sth, cth, sps, cps = np.sin(phi), np.cos(phi), np.sin(theta), np.cos(theta), np.sin(psi), np.cos(psi)
    return ((cps * cth, cps * sth * sph - sps * cph, cps * sth * cph + sps * sph),
            (sps * cth, sps * sth * sph + cps * cph, sps * sth * cph - cps * sph),
            (-sth, cth * sph, cth * cph))


def derivative(variant, table, state, action, dist=None):
    """ds/dt [n, S] (float64) of `state` [n, S] under `action` [n, 4] or [4], the table's coefficients and, for E2E, the constant
    external moments and forces `dist` [n, 6] = (M_x, M_y, M_z, F_x, F_y, F_z)."""
    c = np.asarray(table, np.float64)
    s = np.asarray(state, np.float64)
    u = np.broadcast_to(np.asarray(action, np.float64), (s.shape[0], 4))
    assert c.shape == (COUNT[variant],)
    vx, vy, vz, phi, theta, psi, p, q, r = (s[:, k] for k in range(3, 12))
    R = rotation(phi, theta, psi)
    vbx, vby, vbz = (R[0][j] * vx + R[1][j] * vy + R[2][j] * vz for j in range(3))       # R^T v
    ds = np.zeros_like(s)
    ds[:, 0], ds[:, 1], ds[:, 2] = vx, vy, vz
    ds[:, 6] = p + (q * np.sin(phi) + r * np.cos(phi)) * np.tan(theta)
    ds[:, 7] = q * np.cos(phi) - r * np.sin(phi)
    ds[:, 8] = (q * np.sin(phi) + r * np.cos(phi)) / np.cos(theta)
    if variant == E2E:
        d = np.asarray(dist, np.float64)
        w = s[:, 12:16]
        W = c[0] * w + c[1]
        total, sq = W.sum(axis=1), W * W
        fx = c[2] * vbx * total + d[:, 3]
        fy = c[3] * vby * total + d[:, 4]
        t = c[4] * sq.sum(axis=1) + c[5] * vbz * total + c[6] * (vbx * vbx + vby * vby) + d[:, 5]
        g = c[7]
        ds[:, 9] = c[8] * d[:, 0] + c[9] * q * r + c[10] * vby + c[11] * (sq[:, 0] - sq[:, 1] - sq[:, 2] + sq[:, 3])
        ds[:, 10] = c[12] * d[:, 1] + c[13] * p * r + c[14] * vbx + c[15] * (sq[:, 0] + sq[:, 1] - sq[:, 2] - sq[:, 3])
        ds[:, 11] = (c[16] * d[:, 2] + c[17] * p * q + c[18] * r + c[19] * (u[:, 0] - u[:, 1] + u[:, 2] - u[:, 3])
                     + c[20] * (w[:, 0] - w[:, 1] + w[:, 2] - w[:, 3]))
        ds[:, 12:16] = c[21] * (u - w)
    else:
        tn = s[:, 12]
        fx, fy, t, g = c[0] * vbx, c[1] * vby, c[2] * tn + c[3], c[4]
        ds[:, 9] = c[5] * p + c[6] * u[:, 0]
        ds[:, 10] = c[7] * q + c[8] * u[:, 1]
        ds[:, 11] = c[9] * r + c[10] * u[:, 2]
        ds[:, 12] = c[11] * (u[:, 3] - tn)
    for i in range(3):
        ds[:, 3 + i] = R[i][0] * fx + R[i][1] * fy + R[i][2] * t + (g if i == 2 else 0.0)
    return ds


def step(variant, table, state, action, dist=None, dt=DT):
    """one forward-Euler step (R:512 / I:304), float64"""
    return np.asarray(state, np.float64) + dt * derivative(variant, table, state, action, dist)


def fold_e2e(Ixx, Iyy, Izz, k_x, k_y, k_z, k_w, k_h, k_p, k_pv, k_q, k_qv, k_r1, k_r2, k_rr, tau, w_min, w_max, g):
    """the 22 table entries of the physical parameters.  With W = (w + 1)/2 (w_max - w_min) + w_min (R:106-109) = a w + b and
    W' = a (u - w)/tau (R:112-121), the yaw moment k_r1 (-W1 + W2 - W3 + W4) + k_r2 (-W1' + W2' - W3' + W4') - k_rr r (R:131) is
    -(k_r2 a/tau) (u1 - u2 + u3 - u4) + (k_r2 a/tau - k_r1 a) (w1 - w2 + w3 - w4) - k_rr r."""
    a = (w_max - w_min) / 2.0
    b = a + w_min
    return np.array([a, b, -k_x, -k_y, -k_w, -k_z, -k_h, g,
                     1.0 / Ixx, (Iyy - Izz) / Ixx, k_pv / Ixx, k_p / Ixx,
                     1.0 / Iyy, (Izz - Ixx) / Iyy, k_qv / Iyy, k_q / Iyy,
                     1.0 / Izz, (Ixx - Iyy) / Izz, -k_rr / Izz, -(k_r2 * a / tau) / Izz, (k_r2 * a / tau - k_r1 * a) / Izz,
                     1.0 / tau], np.float64)


def fold_indi(k_x, k_y, T_max, tau_p, tau_q, tau_r, tau_T, p_max, q_max, r_max, g):
    """the 12 table entries: T = (T_norm + 1)/2 T_max (T_min = 0, I:94); rate' = (cmd max - rate)/tau for a symmetric range (I:101-103)"""
    return np.array([-k_x, -k_y, -T_max / 2.0, -T_max / 2.0, g, -1.0 / tau_p, p_max / tau_p, -1.0 / tau_q, q_max / tau_q, -1.0 / tau_r,
                     r_max / tau_r, 1.0 / tau_T], np.float64)


# which table entries hold each physical parameter (read off fold_e2e / fold_indi)
MOVES = {E2E: dict(Ixx=[8, 9, 10, 11, 13, 17], Iyy=[9, 12, 13, 14, 15, 17], Izz=[9, 13, 16, 17, 18, 19, 20], k_x=[2], k_y=[3], k_z=[5], k_w=[4],
                   k_h=[6], k_p=[11], k_pv=[10], k_q=[15], k_qv=[14], k_r1=[20], k_r2=[19, 20], k_rr=[18], tau=[19, 20, 21],
                   w_min=[0, 1, 19, 20], w_max=[0, 1, 19, 20], g=[7]),
         INDI: dict(k_x=[0], k_y=[1], T_max=[2, 3], tau_p=[5, 6], tau_q=[7, 8], tau_r=[9, 10], tau_T=[11], p_max=[6], q_max=[8], r_max=[10], g=[4])}


def injected_states(variant, n=256, seed=STATE_SEED):
    """(world [n, S] float32, disturbances [n, 6] float32 or None): position within 2 m of the scenario track's mid-point and 1-5 m
    above the ground (z points down), velocity within 5 m/s, phi and theta within 1 rad, psi within 3, rates within 5 rad/s, motor
    speeds / T_norm within 1, disturbances inside the training ranges.  Reset-box states leave k_h, the three gyroscopic terms and
    k_rr invisible (rates of 0.1 rad/s, half a metre per second): these do not."""
    import eval_spec

    pos, _, _ = eval_spec.scenario_track()
    mid = pos.mean(axis=0)
    rng = np.random.default_rng(seed + variant)
    S = 16 if variant == E2E else 13
    w = np.empty((n, S), np.float64)
    w[:, 0] = mid[0] + rng.uniform(-2, 2, n)
    w[:, 1] = mid[1] + rng.uniform(-2, 2, n)
    w[:, 2] = rng.uniform(-5, -1, n)
    w[:, 3:6] = rng.uniform(-5, 5, (n, 3))
    w[:, 6:8] = rng.uniform(-1, 1, (n, 2))
    w[:, 8] = rng.uniform(-3, 3, n)
    w[:, 9:12] = rng.uniform(-5, 5, (n, 3))
    w[:, 12:] = rng.uniform(-1, 1, (n, S - 12))
    if variant == INDI:
        return w.astype(np.float32), None
    from optimal_quad_control_rl_amd import TRAIN_DISTURBANCE_RANGES

    r = np.asarray(TRAIN_DISTURBANCE_RANGES, np.float64)
    d = r[:, 0] + (r[:, 1] - r[:, 0]) * rng.uniform(0, 1, (n, 6))
    return w.astype(np.float32), d.astype(np.float32)


def perturbed_tables(nominal, factor=PERTURB):
    """[nominal] + one table per entry with that entry x factor (float32): 23 tables for E2E, 13 for INDI"""
    nominal = np.asarray(nominal, np.float32)
    out = [nominal.copy()]
    for k in range(nominal.shape[0]):
        t = nominal.copy()
        t[k] = np.float32(t[k]) * np.float32(factor)
        out.append(t)
    return out
