"""The closed-loop rollout kernel's action noise and log-probs (qr_rollout_policy, stochastic mode) against the plain NumPy
restatement of the noise spec in tests/action_noise.py, and the PPO trainers' old log-probs against the update that consumes them.

Tolerance of eps (kernel) against eps64 (float64 from the same exact float32 uniforms and the same float32 angle product):
  * u1, u2 are exact and the angle product is restated with the kernel's rounding: no error there;
  * r = fast_sqrt(-2 __logf(u1)): v_log_f32 (log2) times ln 2, relative error <= ~3 * 2^-24 of ln u1 where |ln u1| is not tiny, so
    <= 1.5 * 2^-24 relative in r; fast_sqrt (hardware sqrt + one Newton step) <= 1 ulp = 2^-23;
  * qr_sincos: absolute error <= 7.3e-8 (quadrace_device.hpp), multiplied by r <= sqrt(-2 ln 2^-24) = 5.77 -> <= 4.2e-7;
  * the final float32 product r * cos: 2^-24 relative.
  Sum: |eps - eps64| <= 2.7e-7 |eps| + 4.2e-7 <= 0.7e-6 max(1, |eps|).  The tests allow EPS_TOL = 1e-6 max(1, |eps|); measured on
  MI355X: <= 2.6e-7 over 4.2M draws (every instantiation gives the same bits), at u1 ~ 0.05 - 0.25 where r ~ 1.7 - 2.4.
  Where ln u1 -> 0 (u1 -> 1, r small) the log's ABSOLUTE error dominates: dr = d(ln u1) / r.  Those pairs (-ln u1 < 2^-7, about 1 in
  130) are checked in the r^2 = -2 ln u1 domain instead (|r_k^2 - r64^2| <= R2_TOL absolute; measured <= 4e-9) plus the direction
  (eps / r; measured <= 9e-8), and every component, these included, stays within the 1e-4 absolute ceiling.
Every wrong counter, key or pairing moves eps by O(1) (test_eps_neighbours_are_rejected): the tolerance cannot absorb one."""
import functools
import math

import numpy as np
import pytest
import torch

import action_noise as N
from test_gpu_policy import _make, _policy_for

pytestmark = pytest.mark.gpu

EPS_TOL = 1e-6            # x max(1, |eps64|), away from u1 -> 1
NEAR_LN = 2.0 ** -7       # -ln u1 below this: the r^2-domain check
R2_TOL = 2.0 ** -24       # |r_k^2 - r64^2| = 2 |d ln u1| + the float32 products of eps^2; measured <= 4e-9 (2^-28)
DIR_TOL = 5e-7            # |eps / r - eps64 / r64| of those pairs (qr_sincos: 7.3e-8)
CEILING = 1e-4            # absolute, every component


@functools.lru_cache(maxsize=8)
def _restated(n, K, seed, base=0, first=0):
    return N.action_noise(n, K, seed, env_id_base=base, first_step=first)


def _env(variant, n, ga=1, seed=5, env_id_base=0, max_steps=30):
    from optimal_quad_control_rl_amd import (Quadcopter3DGates, Quadcopter3DGatesINDI, TRAIN_DISTURBANCE_RANGES,
                                             square_track, zigzag_track)

    if variant == "e2e":
        env = Quadcopter3DGates(n, *zigzag_track(), gates_ahead=ga, seed=seed, infos_mode="none", env_id_base=env_id_base)
        env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    else:
        env = Quadcopter3DGatesINDI(n, *square_track(), gates_ahead=ga, seed=seed, infos_mode="none", env_id_base=env_id_base)
    env.max_steps = max_steps
    env.reset_device()
    return env


def _zero_policy(L):
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    z = lambda *s: np.zeros(s, np.float32)
    return MfmaPolicy(L).set_weights([(z(120, L), z(120)), (z(120, 120), z(120)), (z(120, 120), z(120)), (z(4, 120), z(4))])


def _pair_mask(u, shape):
    """[K, n, 4] bool: the component's pair has -ln u1 < NEAR_LN."""
    u1a, _, u1b, _ = u
    na, nb = -np.log(u1a.astype(np.float64)) < NEAR_LN, -np.log(u1b.astype(np.float64)) < NEAR_LN
    return np.broadcast_to(np.stack([na, na, nb, nb], -1), shape)


def eps_errors(eps_k, eps64, u):
    """(max |d eps| / max(1, |eps64|) away from u1 -> 1, its (u1, u2), max |d r^2| and max direction error near u1 = 1,
    max absolute |d eps| overall)."""
    eps_k = np.asarray(eps_k, np.float64)
    d = np.abs(eps_k - eps64)
    near = _pair_mask(u, d.shape)
    rel = np.where(near, 0.0, d / np.maximum(1.0, np.abs(eps64)))
    j = np.unravel_index(np.argmax(rel), rel.shape)
    pair = 0 if j[2] < 2 else 2
    where = (float(u[pair][j[:2]]), float(u[pair + 1][j[:2]]))
    r2_err = dir_err = 0.0
    for p, un in ((0, u[0]), (2, u[2])):
        m = -np.log(un.astype(np.float64)) < NEAR_LN
        if not m.any():
            continue
        ek, e64 = eps_k[..., p:p + 2][m], eps64[..., p:p + 2][m]
        rk2, r642 = (ek ** 2).sum(-1), -2.0 * np.log(un[m].astype(np.float64))
        r2_err = max(r2_err, float(np.abs(rk2 - r642).max()))
        ok = (rk2 > 0) & (r642 >= 1e-4)     # (below r = 0.01 the direction of a 1e-9 rounding is meaningless; r^2 covers it)
        if ok.any():
            dk = ek[ok] / np.sqrt(rk2[ok])[:, None]
            d64 = e64[ok] / np.sqrt(r642[ok])[:, None]
            dir_err = max(dir_err, float(np.abs(dk - d64).max()))
    return float(rel.max()), where, r2_err, dir_err, float(d.max())


def assert_eps(eps_k, eps64, u, label):
    rel, where, r2_err, dir_err, absmax = eps_errors(eps_k, eps64, u)
    print("%s: max |eps - eps64| / max(1, |eps|) = %.3e at (u1, u2) = (%.9g, %.9g); u1 -> 1: |d r^2| %.3e, direction %.3e; "
          "max abs %.3e" % (label, rel, where[0], where[1], r2_err, dir_err, absmax))
    assert rel <= EPS_TOL, (label, rel, where)
    assert r2_err <= R2_TOL and dir_err <= DIR_TOL, (label, r2_err, dir_err)
    assert absmax <= CEILING, (label, absmax)
    return rel


def logp_error(logp_k, eps64, log_std):
    lp64 = N.log_prob(eps64, np.asarray(log_std, np.float32).astype(np.float64))
    return float((np.abs(np.asarray(logp_k, np.float64) - lp64) / np.maximum(1.0, np.abs(lp64))).max())


# log-prob: 0.5 sum(eps^2) carries 2 EPS_TOL relative of each eps^2 term, plus the float32 fma chain (five roundings of |logp|)
LOGP_TOL = 2e-6           # x max(1, |logp64|); measured <= 3.9e-7


# ---- 3a: the raw stream of every instantiation -------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
@pytest.mark.parametrize("ga", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("n", [1000, 65536, 262144])
def test_raw_noise_stream_matches_restatement(variant, ga, n):
    """Zero network (mean == 0 exactly) and log_std = 0 (std == 1): act == eps.  Both forwards of the (variant, gates_ahead)
    template: 20 kernel instantiations over the three n (ragged last wave; 65 536; several waves per SIMD).  Catches: a wrong
    counter word or key, a wrong pairing of uniforms, a Box-Muller slice that one instantiation's schedule misplaces (its eps
    would be computed from partial Philox state), and noise that depends on the forward (f16-operand vs f32-class bits differ)."""
    K, seed, first = 16, 0xC0FFEE, 3
    eps64, u = _restated(n, K, seed, 0, first)
    outs = {}
    for precision in ("f16-operands", "f32"):
        env = _env(variant, n, ga)
        pol = _zero_policy(env.state_len)
        obs, act, logp, *_ = env.rollout_policy_device(pol, K, torch.zeros(4), noise_seed=seed, first_step=first, precision=precision)
        torch.cuda.synchronize()
        a, lp = act.cpu().numpy(), logp.cpu().numpy()
        label = "%s ga=%d L=%d n=%d %s" % (variant, ga, env.state_len, n, precision)
        assert np.isfinite(a).all() and np.isfinite(lp).all()
        assert_eps(a, eps64, u, label)
        e_lp = logp_error(lp, eps64, np.zeros(4))
        print("%s: max |logp - logp64| / max(1, |logp|) = %.3e" % (label, e_lp))
        assert e_lp <= LOGP_TOL, (label, e_lp)
        outs[precision] = (a, lp)
        del env, pol, obs, act, logp
    assert np.array_equal(outs["f16-operands"][0].view(np.uint32), outs["f32"][0].view(np.uint32))
    assert np.array_equal(outs["f16-operands"][1].view(np.uint32), outs["f32"][1].view(np.uint32))


# ---- 3b: the tolerance rejects every neighbouring stream ---------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16-operands", "f32"])
def test_eps_neighbours_are_rejected(precision):
    """The kernel's eps must NOT pass against the restatement at step + 1, gid + 1, the seed with only its top bit flipped, or the
    pairing (x0, x1) <-> (x2, x3): each of those is off by O(1) in most components, so none of them fits the tolerance."""
    n, K, seed, first = 65536, 16, 0xC0FFEE, 3
    env = _env("e2e", n, 1)
    _, act, *_ = env.rollout_policy_device(_zero_policy(env.state_len), K, torch.zeros(4), noise_seed=seed, first_step=first,
                                           precision=precision)
    a = act.cpu().numpy().astype(np.float64)
    eps64, u = _restated(n, K, seed, 0, first)
    assert_eps(a, eps64, u, "e2e ga=1 " + precision)
    wrong = {
        "step + 1": N.action_noise(n, K, seed, first_step=first + 1),
        "gid + 1": N.action_noise(n + 1, K, seed, first_step=first)[0][:, 1:],
        "seed ^ 2^63": N.action_noise(n, K, seed ^ (1 << 63), first_step=first),
        "seed ^ 2^31": N.action_noise(n, K, seed ^ (1 << 31), first_step=first),
        "swapped pairs": N.action_noise(n, K, seed, first_step=first, swap_pairs=True),
    }
    for name, w in wrong.items():
        w = w[0] if isinstance(w, tuple) else w
        d = np.abs(a - w)
        frac = float((d > 0.1).mean())
        print("%s vs %s: %.3f of components off by > 0.1, max %.3f" % (precision, name, frac, d.max()))
        assert frac > 0.8 and d.max() > 1.0, (name, frac)
        assert (d / np.maximum(1.0, np.abs(w))).max() > 100 * EPS_TOL and d.max() > 100 * CEILING


# ---- 3c: carries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16-operands", "f32"])
def test_noise_counter_and_key_carries(precision):
    """gid carry inside one handle (env_id_base = 2^32 - 300, n = 1000), step carry inside one launch (first_step = 2^32 - 5,
    K = 12), and the seed's high word (7 vs 2^32 + 7).  Catches a dropped carry into gid_hi / step_hi and a key that ignores
    seed_hi."""
    def run(n, K, base, first, seed):
        env = _env("indi", n, 1, env_id_base=base)
        _, act, logp, *_ = env.rollout_policy_device(_zero_policy(env.state_len), K, torch.zeros(4), noise_seed=seed,
                                                     first_step=first, precision=precision)
        a, lp = act.cpu().numpy(), logp.cpu().numpy()
        eps64, u = N.action_noise(n, K, seed, env_id_base=base, first_step=first)
        assert_eps(a, eps64, u, "%s base=%d first=%d seed=%d" % (precision, base, first, seed))
        assert logp_error(lp, eps64, np.zeros(4)) <= LOGP_TOL
        return a

    a = run(1000, 4, 2 ** 32 - 300, 0, 7)
    # the envs past the carry are NOT the stream of gid 0.. (what a dropped carry into gid_hi would give)
    low, _ = N.action_noise(700, 4, 7, env_id_base=0, first_step=0)
    assert (np.abs(a[:, 300:] - low) > 0.1).mean() > 0.8
    b = run(1000, 12, 0, 2 ** 32 - 5, 7)
    low, _ = N.action_noise(1000, 7, 7, env_id_base=0, first_step=0)
    assert (np.abs(b[5:] - low) > 0.1).mean() > 0.8
    c = run(1000, 4, 0, 0, 7)
    d = run(1000, 4, 0, 0, 2 ** 32 + 7)
    assert (np.abs(c - d) > 0.1).mean() > 0.8


# ---- 3d: a real policy, small sigma, and the env stepping clip(a) -------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
@pytest.mark.parametrize("precision", ["f16-operands", "f32"])
def test_stochastic_rollout_equals_mean_plus_noise_and_replays(variant, precision):
    """act[k] == fmaf(std, eps, mean_k) with mean_k = pol.forward(obs[k]) (bit-equal to the in-kernel mean) and eps the restated stream;
    logp against the float64 formula with log_std = (0, -0.5, 0.3, -3); a second handle stepped with clip(act[k]) reproduces obs,
    rew, done, trunc and the final state bit for bit through auto-resets.  Catches: the env stepping the mean or the unclipped action,
    a std / log_std component mix-up, a wrong log-prob constant, noise scaled by the wrong std."""
    n, K, seed, first = 65536, 40, 99, 1234
    log_std = np.array([0.0, -0.5, 0.3, -3.0], np.float32)
    std = np.exp(log_std.astype(np.float64)).astype(np.float32)
    net, pol = _policy_for(_make(variant, 8))
    ea, eb = _env(variant, n), _env(variant, n)
    obs, act, logp, rew, done, trunc, last = ea.rollout_policy_device(pol, K, torch.as_tensor(log_std), noise_seed=seed,
                                                                      first_step=first, precision=precision)
    eps64, u = _restated(n, K, seed, 0, first)
    # the raw stream of the same (seed, gid, step) from a zero network: the kernel's own eps, exactly
    ez = _env(variant, n)
    _, raw, *_ = ez.rollout_policy_device(_zero_policy(ez.state_len), K, torch.zeros(4), noise_seed=seed, first_step=first,
                                          precision=precision)
    raw = raw.cpu().numpy()
    assert_eps(raw, eps64, u, "%s %s raw" % (variant, precision))
    o = eb.states_tensor.clone()
    worst_ulp = 0
    for k in range(K):
        assert torch.equal(obs[k], o), k
        mean = pol.forward(o, precision=precision).cpu().numpy()
        a = act[k].cpu().numpy()
        # fmaf(std, eps_kernel, mean): std * eps is exact in float64; the sum rounded once more to float32 (a double rounding can
        # differ by one ulp, once in ~2^29 draws)
        want = (std.astype(np.float64) * raw[k] + mean).astype(np.float32)
        ulp = np.abs(a.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        worst_ulp = max(worst_ulp, int(ulp.max()))
        assert ulp.max() <= 1 and (ulp == 0).mean() > 0.9999, k
        ref = mean.astype(np.float64) + std.astype(np.float64) * eps64[k]
        tol = std * (EPS_TOL * np.maximum(1.0, np.abs(eps64[k])) + np.where(_pair_mask(tuple(x[k:k + 1] for x in u), (1, n, 4))[0], CEILING, 0.0)) \
            + 2.0 ** -23 * np.abs(ref)
        assert (np.abs(a - ref) <= tol).all(), k
        o2, r2, d2, t2 = eb.step_device(act[k].clamp(-1, 1).contiguous())
        assert torch.equal(rew[k], r2) and torch.equal(done[k], d2) and torch.equal(trunc[k], t2), k
        o = o2.clone()
    assert torch.equal(last, o)
    for sa, sb in zip(ea.get_state_tensors(), eb.get_state_tensors()):
        assert sa is None or torch.equal(sa, sb)
    assert int(done.sum()) >= n                       # max_steps = 30 inside K = 40
    assert float((act.abs() > 1).float().mean()) > 0.01  # the clip is exercised
    e_lp = logp_error(logp.cpu().numpy(), eps64, log_std)
    print("%s %s: max |logp - logp64| / max(1, |logp|) = %.3e (log_std %s); act vs fmaf(std, eps_kernel, mean) <= %d ulp"
          % (variant, precision, e_lp, log_std.tolist(), worst_ulp))
    assert e_lp <= LOGP_TOL


# ---- 3e: shards --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_sharded_stochastic_rollout_equals_unsharded(variant):
    """Four handles of n/4 envs with env_id_base = r n / 4 reproduce one handle of n envs bit for bit (same env seed, noise seed and
    first step): obs, act, logp, rew, done.  Catches noise keyed by the local env index instead of the global one (every shard
    would repeat shard 0's noise) and reset draws keyed likewise."""
    n, K, seed, first = 16384, 40, 4242, 77
    net, pol = _policy_for(_make(variant, 8))
    ls = torch.tensor([0.0, -0.5, 0.3, -1.0])
    full = _env(variant, n, seed=13)
    ref = [t.clone() for t in full.rollout_policy_device(pol, K, ls, noise_seed=seed, first_step=first)[:5]]
    m = n // 4
    parts = []
    for r in range(4):
        e = _env(variant, m, seed=13, env_id_base=r * m)
        parts.append([t.clone() for t in e.rollout_policy_device(pol, K, ls, noise_seed=seed, first_step=first)[:5]])
    for j, name in enumerate(("obs", "act", "logp", "rew", "done")):
        cat = torch.cat([p[j] for p in parts], dim=1)
        assert torch.equal(cat, ref[j]), name
    assert int(ref[4].sum()) > 0
    assert not torch.equal(parts[0][1], parts[1][1])


# ---- 3f: the trainer's position in the stream ---------------------------------------------------------------------------------
def _eps_from(model, precision="f16-operands"):
    T, n = model.n_steps, model.n_envs
    std = model.policy.log_std.detach().exp()
    mean = torch.stack([model._mfma.forward(model.buf_obs[t].contiguous(), precision=precision) for t in range(T)])
    return ((model.buf_act - mean) / std).cpu().numpy().astype(np.float64), std.cpu().numpy()


def _assert_stream(eps_k, n, T, seed, first, label):
    eps64, u = N.action_noise(n, T, seed, first_step=first)
    # (act - mean) / std: the float32 rounding of act = fmaf(std, eps, mean) adds ~2^-24 |act| / std; with std = 1 and |mean| << 1
    # that stays inside EPS_TOL
    assert_eps(eps_k, eps64, u, label)


def test_ppo_fused_collect_draws_consecutive_stream_positions_and_resumes():
    """Three consecutive collect() calls draw steps 0, T, 2T of the stream keyed by `seed`; a checkpoint round trip continues at
    noise_step.  Catches a collect that restarts the stream each rollout (every rollout would train on the same noise), one that
    advances it by the wrong amount, and a checkpoint that drops noise_step."""
    from optimal_quad_control_rl_amd import Quadcopter3DGatesINDI, square_track
    from optimal_quad_control_rl_amd.ppo import PPO

    n, T, seed = 4096, 16, 31

    def make():
        env = Quadcopter3DGatesINDI(n, *square_track(), gates_ahead=1, infos_mode="none", seed=1)
        return PPO(env, n_steps=T, n_epochs=1, batch_size=n * T // 4, seed=seed, fused_collect=True)

    model = make()
    seen = []
    for c in range(3):
        model.collect()
        eps_k, _ = _eps_from(model)
        _assert_stream(eps_k, n, T, seed, c * T, "collect %d" % c)
        seen.append(eps_k)
        if c == 1:
            sd = model.state_dict()
            theta = {k: v.clone() for k, v in model.policy.state_dict().items()}
    assert (np.abs(seen[1] - seen[0]) > 0.1).mean() > 0.8 and (np.abs(seen[2] - seen[1]) > 0.1).mean() > 0.8
    assert model.noise_step == 3 * T
    resumed = make()
    resumed.policy.load_state_dict(theta)
    resumed.load_state_dict(sd)
    assert resumed.noise_step == 2 * T
    resumed.collect()
    eps_r, _ = _eps_from(resumed)
    _assert_stream(eps_r, n, T, seed, 2 * T, "resumed")
    assert resumed.noise_step == 3 * T


# ---- 4: the old log-probs are those of the update that consumes them ----------------------------------------------------------
PAIRINGS = {
    "torch collect + torch update": dict(),
    "fused f16 + native f16": dict(fused_collect=True, native_update=True),
    "fused f32class + native f32": dict(fused_collect=True, native_update=True, policy_forward="f32class", update_precision="f32"),
    "fused f32class + native f16 (f32-collect)": dict(fused_collect=True, native_update=True, policy_forward="f32class"),
}
# mean approx-KL per row at the first minibatch.  A mean offset dmu gives ~0.5 (dmu / sigma)^2 per component (4e-4 per row for
# dmu = 7e-4 at sigma = 0.05); measured on MI355X with this network: 6.4e-6 per row for the f32-class collect forward's log-probs
# against the f16-operand update, <= 4e-11 for every consistent pairing.
KL_ROW_TOL = 1e-8


@pytest.mark.parametrize("pairing", list(PAIRINGS))
def test_first_minibatch_ratio_is_one(pairing):
    """Before any optimiser step the PPO ratio is 1 up to float32 rounding for every collect / update pairing: the approx-KL sum over
    the buffer is at the float32 level per row and no sample is clipped (clip 0.2), with 120-unit nets, a non-trivial output head and
    sigma = 0.05, where a mean offset dmu between the collect forward and the update forward shows as z dmu / sigma.  Catches old
    log-probs taken from a forward whose arithmetic differs from the update's (the f32-class collect + f16-operand update pairing
    stored the f32-class kernel's log-probs)."""
    from optimal_quad_control_rl_amd import Quadcopter3DGatesINDI, square_track
    from optimal_quad_control_rl_amd.ppo import PPO

    n, T = 4096, 16
    env = Quadcopter3DGatesINDI(n, *square_track(), gates_ahead=1, infos_mode="none", seed=1)
    env.max_steps = 30
    model = PPO(env, n_steps=T, n_epochs=1, batch_size=n * T // 8, seed=2, log_std_init=math.log(0.05), **PAIRINGS[pairing])
    with torch.no_grad():
        for m in model.policy.pi:
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
        model.policy.pi[-1].weight.mul_(30.0)
    if model._updater is not None:
        model._updater.pack()
    model.collect()
    B = n * T
    obs, act, old_lp = model.buf_obs.view(B, -1), model.buf_act.view(B, 4), model.buf_lp.view(B).contiguous()
    kl, clipped = _first_minibatch_kl(model, obs, act, old_lp)
    print("%s: first-minibatch approx-KL per row %.3e, clipped %d of %d" % (pairing, kl / B, clipped, B))
    if model.fused_collect:
        # what the buffer held before the f32-collect fix: the log-probs of the COLLECT kernel's forward (the rollout kernel's own
        # log-probs are these up to float32 rounding)
        precision = "f32" if model.policy_forward == "f32class" else "f16-operands"
        with torch.no_grad():
            lp_c = model.policy.log_prob_from_mean(model._mfma.forward(obs, precision=precision), act).contiguous()
        kl_c, clipped_c = _first_minibatch_kl(model, obs, act, lp_c)
        print("%s: with the collect forward's log-probs: approx-KL per row %.3e, clipped %d" % (pairing, kl_c / B, clipped_c))
        if "f32-collect" in pairing:
            assert kl_c / B > 100 * KL_ROW_TOL   # the test sees the offset the fix removes
    assert clipped == 0, (pairing, clipped)
    assert abs(kl) / B <= KL_ROW_TOL, (pairing, kl / B)


def _first_minibatch_kl(model, obs, act, old_lp):
    """(approx-KL sum, clipped count) over minibatches covering the buffer, before any optimiser step, as the update computes them."""
    B = obs.shape[0]
    if model._updater is None:
        with torch.no_grad():
            lp, _ = model.policy.log_prob_entropy(obs, act)
        log_ratio = (lp - old_lp).double()
        return float(((log_ratio.exp() - 1.0) - log_ratio).sum()), int(((log_ratio.exp() - 1.0).abs() > 0.2).sum())
    up = model._updater
    up.stats.zero_()
    g = torch.Generator(device=model.dev)
    g.manual_seed(0)
    adv = torch.randn(B, device=model.dev, generator=g)
    ret = torch.zeros(B, device=model.dev)
    perm = torch.randperm(B, device=model.dev, generator=g).to(torch.int32)
    out = None
    for s in range(0, B, model.batch_size):
        out = up.grad(obs, act, old_lp, adv, ret, perm[s:s + model.batch_size].contiguous(), clip=0.2, stats=True, out=out)
    st = up.stats.tolist()
    return st[2], int(st[3])
