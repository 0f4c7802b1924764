"""GPU: the evolution-strategies kernels (csrc/quadrace_es.hip, qr_es_*) against the NumPy restatement tests/es_spec.py, and
EvolutionStrategy.step() against the hand-composed sequence of existing calls.

The noise is held against the float64 restatement with the tolerance tests/test_gpu_action_noise.py derives for the same three
functions (fast_sqrt(-2 __logf), qr_sincos, one float32 product): EPS_TOL = 1e-6 max(1, |eps|), the r^2-domain rule near u1 = 1 and the
1e-4 ceiling.  Everything after the noise -- members, bank images, summary, score, utilities, update -- has NO tolerance: the restatement
is fed with the device's own eps (qr_es_noise) and int32 / int64 views are compared (NaN positions must agree; a NaN's payload is not
compared)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import es_spec as S
from optimal_quad_control_rl_amd import _lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = -123.25
W = dict(w_gate=0.3, w_crash=-100.0, w_timeout=-7.5, w_return=0.01, w_lap=-1.0, no_lap_steps=1200.0)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


class Handle:
    """a bare qr_es handle"""

    def __init__(self, L, pairs):
        self.lib, self.L, self.pairs, self.P = _lib.load(), L, pairs, 2 * pairs
        h = C.c_void_p()
        _lib.check(self.lib.qr_es_create(L, 0, pairs, C.byref(h)))
        self.h, self.n = h, self.lib.qr_es_num_params(h)
        assert self.n == S.num_params(L)

    def noise(self, seed, generation):
        eps = torch.full((self.pairs, self.n), SENTINEL, device=DEV)
        _lib.check(self.lib.qr_es_noise(self.h, seed, generation, _p(eps), _stream()))
        return eps

    def close(self):
        self.lib.qr_es_destroy(self.h)


def _bits_equal(a, b, what):
    """no tolerance: equal bits wherever neither is a NaN, and NaNs in the same places"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), (what, "NaN positions", int((na != nb).sum()))
    view = np.int32 if a.dtype == np.float32 else np.int64
    diff = (a.view(view) != b.view(view)) & ~na
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def _layers(flat, L):
    """a flat actor block (NumPy) as [(w1, b1), ..., (w4, b4)] in torch Linear layout"""
    out, off = [], 0
    for rows, cols in ((120, L), (120, 120), (120, 120), (4, 120)):
        w = flat[off:off + rows * cols].reshape(rows, cols)
        off += rows * cols
        out.append((w, flat[off:off + rows]))
        off += rows
    assert off == flat.size
    return out


def _image_bytes(L):
    return (4 * ((L + 1 + 15) // 16) * 64 + 2 * 4 * 8 * 64 + 8 * 64) * 16


def _read(bank, slot, which):
    out = np.zeros(_image_bytes(bank.obs_len) // 2, dtype=np.uint16)
    _lib.check(_lib.load().qr_policy_bank_read(bank._h, slot, which, out.ctypes.data_as(C.c_void_p), out.nbytes))
    return out


def _marked_bank(L, capacity):
    """a bank whose every slot holds a recognisable policy (weights = slot + 1)"""
    from optimal_quad_control_rl_amd.policy import MfmaPolicyBank

    bank = MfmaPolicyBank(L, capacity, 0)
    for s in range(capacity):
        bank.set_weights(s, _layers(np.full(S.num_params(L), float(s + 1), np.float32), L))
    return bank


def _theta(n, seed, planted=True):
    theta = (np.random.default_rng(seed).normal(size=n) * 0.1).astype(np.float32)
    if planted:   # beyond the f16 range both ways, below its subnormals, inf and NaN: in every layer's weights and in biases
        for k, val in enumerate((7e4, -7e4, 1e-9, np.inf, np.nan, -np.inf)):
            for at in (3, n // 3, n // 2, n - 5 - 7 * k, n - 500):
                theta[at + k] = val
    return theta


# ---- the noise -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generation", [0, 2 ** 33 + 3])
def test_noise_matches_the_restatement_and_rejects_its_neighbours(generation):
    """L = 13, 2 pairs, seed with both words in use.  Catches a wrong counter word, key word or tweak, a dropped generation high word, and
    a wrong pairing of the uniforms: each neighbouring stream is off by O(1) in most components."""
    from test_gpu_action_noise import CEILING, EPS_TOL, assert_eps

    seed, pairs = 0xC0FFEE + (0x5EED << 32), 2
    h = Handle(13, pairs)
    eps = h.noise(seed, generation).cpu().numpy()
    h.close()
    assert np.isfinite(eps).all() and not (eps == SENTINEL).any()
    shape = (pairs, h.n // 4, 4)
    eps64, u = S.noise(h.n, pairs, seed, generation)
    rel = assert_eps(eps.reshape(shape), eps64.reshape(shape), u, "qr_es_noise generation %d" % generation)
    print("qr_es_noise: measured max |eps - eps64| / max(1, |eps|) = %.3e (tolerance %.1e)" % (rel, EPS_TOL))
    wrong = {
        "pair + 1": S.noise(h.n, pairs, seed, generation, first_pair=1),
        "pair - 1": S.noise(h.n, pairs, seed, generation, first_pair=-1),
        "generation + 1": S.noise(h.n, pairs, seed, generation + 1),
        "generation - 1": S.noise(h.n, pairs, seed, (generation - 1) % 2 ** 64),
        "generation without its high word": S.noise(h.n, pairs, seed, generation % 2 ** 32 + (1 << 40)),
        "seed ^ 2^31": S.noise(h.n, pairs, seed ^ (1 << 31), generation),
        "seed ^ 2^63": S.noise(h.n, pairs, seed ^ (1 << 63), generation),
        "swapped pairs": S.noise(h.n, pairs, seed, generation, swap_pairs=True),
    }
    for name, (w, _) in wrong.items():
        d = np.abs(eps.astype(np.float64) - w)
        frac = float((d > 0.1).mean())
        assert frac > 0.8 and d.max() > 1.0, (name, frac)
        assert (d / np.maximum(1.0, np.abs(w))).max() > 100 * EPS_TOL and d.max() > 100 * CEILING, name


# ---- perturb ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_slot", [0, 2])
@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("L", [13, 24])
def test_perturb_writes_the_members_and_their_bank_slots(L, pairs, first_slot):
    """theta_pop == the restated members of the emitted eps; every slot, both images, == qr_policy_bank_set of theta_pop's rows; the slots
    outside [first_slot, first_slot + P) keep their marks.  theta holds 7e4, -7e4, 1e-9, +-inf and NaN."""
    from optimal_quad_control_rl_amd.policy import MfmaPolicyBank

    seed, gen, sigma = 77, 5, 0.05
    h = Handle(L, pairs)
    P, n = h.P, h.n
    theta = _theta(n, seed=L + pairs)
    th = torch.as_tensor(theta, device=DEV)
    eps = h.noise(seed, gen).cpu().numpy()
    got = _marked_bank(L, P + 2)
    before = {s: [_read(got, s, w) for w in (0, 1)] for s in range(P + 2)}
    pop = torch.full((P, n), SENTINEL, device=DEV)
    _lib.check(h.lib.qr_es_perturb(h.h, _p(th), sigma, seed, gen, got._h, first_slot, _p(pop), _stream()))
    pop = pop.cpu().numpy()
    _bits_equal(pop, S.members(theta, sigma, eps), "theta_pop")
    assert np.array_equal(th.cpu().numpy().view(np.int32), theta.view(np.int32))
    ref = MfmaPolicyBank(L, P, 0)
    for p in range(P):
        ref.set_weights(p, _layers(pop[p], L))
    for p in range(P):
        for which in (0, 1):
            assert np.array_equal(_read(got, first_slot + p, which), _read(ref, p, which)), (p, which)
    for s in [s for s in range(P + 2) if not first_slot <= s < first_slot + P]:
        for which in (0, 1):
            assert np.array_equal(_read(got, s, which), before[s][which]), ("slot outside the range", s, which)
    # without theta_pop_dev the slots are the same, and a never-set bank's slots become readable
    fresh = MfmaPolicyBank(L, P + 2, 0)
    _lib.check(h.lib.qr_es_perturb(h.h, _p(th), sigma, seed, gen, fresh._h, first_slot, None, _stream()))
    for p in range(P):
        for which in (0, 1):
            assert np.array_equal(_read(fresh, first_slot + p, which), _read(ref, p, which)), (p, which)
    out = np.zeros(_image_bytes(L) // 2, dtype=np.uint16)
    unset = [s for s in range(P + 2) if not first_slot <= s < first_slot + P]
    assert all(h.lib.qr_policy_bank_read(fresh._h, s, 0, out.ctypes.data_as(C.c_void_p), out.nbytes) == _lib.QR_E_INVALID for s in unset)
    for b in (got, ref, fresh):
        b.close()
    h.close()


# ---- fitness ---------------------------------------------------------------------------------------------------------------------------
def _records(P, E, seed):
    rng = np.random.default_rng(seed)
    rec = rng.integers(0, 40, size=(P * E, S.REC_INTS)).astype(np.int32)
    rec[:, 6:14] = rng.integers(0, 3000, size=(P * E, 8))
    rec[2 * E:3 * E, 15:22] = 0            # policy 2: no flying lap
    rec[3 * E:, 1] = 0                     # policy 3: never crashes
    recf = (rng.normal(size=(P * E, S.REC_FLOATS)) * 300.0).astype(np.float32)
    recf[:E, :2] = -np.abs(recf[:E, :2])   # policy 0: negative returns only
    return rec, recf


@pytest.mark.parametrize("E", [256, 512])
def test_fitness_summary_and_score_equal_the_restatement(E):
    """P = 4: a policy without a flying lap (no_lap_steps), negative returns, recf NULL; two chunks at E = 512 (the order of s7)."""
    h = Handle(13, 2)
    P = h.P
    rec, recf = _records(P, E, seed=E)
    d_rec, d_recf = torch.as_tensor(rec, device=DEV), torch.as_tensor(recf, device=DEV)
    w = _lib.QrEsFitnessWeights(*[W[k] for k in ("w_gate", "w_crash", "w_timeout", "w_return", "w_lap", "no_lap_steps")])
    for with_recf in (True, False):
        summ = torch.full((P, 8), SENTINEL, dtype=torch.float64, device=DEV)
        fit = torch.full((P,), SENTINEL, dtype=torch.float64, device=DEV)
        _lib.check(h.lib.qr_es_fitness(h.h, _p(d_rec), _p(d_recf) if with_recf else None, E, C.byref(w), _p(summ), _p(fit), _stream()))
        s = S.summary(rec, recf if with_recf else None, E)
        _bits_equal(summ.cpu().numpy(), s, "summary recf=%s" % with_recf)
        _bits_equal(fit.cpu().numpy(), S.score(s, W, E), "score recf=%s" % with_recf)
        assert s[2, 5] == 0 and s[0, 5] > 0 and (not with_recf or s[0, 7] < 0)
        fit2 = torch.full((P,), SENTINEL, dtype=torch.float64, device=DEV)   # summary_dev NULL: the same scores
        _lib.check(h.lib.qr_es_fitness(h.h, _p(d_rec), _p(d_recf) if with_recf else None, E, C.byref(w), None, _p(fit2), _stream()))
        assert torch.equal(fit.view(torch.int64), fit2.view(torch.int64))
    h.close()


# ---- update ----------------------------------------------------------------------------------------------------------------------------
def _scores(P, shaping, rng):
    F = rng.normal(size=P) * 50.0
    if P > 2:
        F[P // 2] = F[0]                   # ties
        F[1] = F[P - 2]
    elif shaping == S.SHAPE_CENTERED_RANK:
        F[1] = F[0]                        # (under QR_ES_SHAPE_NONE a tied single pair is d = 0: no update at all)
    if shaping == S.SHAPE_CENTERED_RANK:   # (a NaN under QR_ES_SHAPE_NONE is a NaN utility and a NaN theta everywhere: nothing left to compare)
        F[P - 1] = np.nan
        if P > 4:
            F[2] = np.nan
    return F


@pytest.mark.parametrize("step_wd", [(1, 0.0), (7, 1e-3)])
@pytest.mark.parametrize("shaping", [S.SHAPE_CENTERED_RANK, S.SHAPE_NONE])
@pytest.mark.parametrize("pairs", [1, 2, 128])
def test_update_equals_the_restatement(pairs, shaping, step_wd):
    """theta, m, v and u bit for bit == the float32 restatement fed with qr_es_noise's eps: scores with ties (and NaNs under ranks), the first
    and a later Adam step, with and without weight decay."""
    adam_step, wd = step_wd
    seed, gen, sigma, lr, b1, b2, ae = 2 ** 40 + 9, 2 ** 32 + 1, 0.03, 0.01, 0.9, 0.999, 1e-8
    h = Handle(13, pairs)
    P, n = h.P, h.n
    rng = np.random.default_rng(100 * pairs + 10 * shaping + adam_step)
    theta = _theta(n, seed=pairs, planted=False)
    m = np.zeros(n, np.float32) if adam_step == 1 else (rng.normal(size=n) * 0.05).astype(np.float32)
    v = np.zeros(n, np.float32) if adam_step == 1 else (rng.normal(size=n) * 0.05).astype(np.float32) ** 2
    F = _scores(P, shaping, rng)
    eps = h.noise(seed, gen).cpu().numpy()
    d = [torch.as_tensor(a, device=DEV) for a in (theta, m, v)]
    d_F = torch.as_tensor(F, device=DEV)
    util = torch.full((P,), SENTINEL, device=DEV)
    _lib.check(h.lib.qr_es_update(h.h, _p(d[0]), _p(d[1]), _p(d[2]), _p(d_F), sigma, seed, gen, shaping, lr, b1, b2, ae, wd, adam_step, _p(util),
                                  _stream()))
    want = S.update(theta, m, v, F, eps, sigma, shaping, lr, b1, b2, ae, wd, adam_step)
    for name, got, ref in zip(("theta", "m", "v"), d, want[:3]):
        _bits_equal(got.cpu().numpy(), ref, "%s pairs=%d shaping=%d step=%d" % (name, pairs, shaping, adam_step))
    _bits_equal(util.cpu().numpy(), want[3], "u")
    assert np.isfinite(want[0]).all() and not np.array_equal(want[0], theta)
    if shaping == S.SHAPE_CENTERED_RANK:
        assert sorted(np.rint((want[3].astype(np.float64) + 0.5) * (P - 1)).astype(int).tolist()) == list(range(P))
    # util_dev NULL: the same update
    d2 = [torch.as_tensor(a, device=DEV) for a in (theta, m, v)]
    _lib.check(h.lib.qr_es_update(h.h, _p(d2[0]), _p(d2[1]), _p(d2[2]), _p(d_F), sigma, seed, gen, shaping, lr, b1, b2, ae, wd, adam_step, None, _stream()))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(d, d2))
    h.close()


# ---- one generation end to end -------------------------------------------------------------------------------------------------------------
def _race_env(n, max_steps=30):
    from optimal_quad_control_rl_amd import Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, zigzag_track

    env = Quadcopter3DGates(n, *zigzag_track(), gates_ahead=1, seed=5, infos_mode="none")
    env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    env.max_steps = max_steps
    return env


def _actor(L, seed=0):
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    torch.manual_seed(seed)
    return ActorCritic(L, 4).pi.to(DEV)


E2E = dict(pairs=2, envs_per_policy=256, sigma=0.05, lr=0.01, fitness={k: v for k, v in W.items() if k != "no_lap_steps"}, n_eval_steps=64,
           seed=21, weight_decay=1e-3)


def test_step_equals_the_hand_composed_generation():
    """E2E, gates_ahead 1, N = 1024 = 4 x 256, 64 evaluation steps (time limit 30: episodes end inside them).  step() leaves theta, m, v
    where: restated members of the emitted eps -> qr_policy_bank_set -> evaluate_bank_device on the same starts -> the restated summary,
    score and update leave them."""
    from optimal_quad_control_rl_amd import EvolutionStrategy
    from optimal_quad_control_rl_amd.evaluation import default_gates_per_lap
    from optimal_quad_control_rl_amd.policy import MfmaPolicyBank

    env, actor = _race_env(1024), _actor(24)
    es = EvolutionStrategy(env, actor, **E2E)
    theta0 = es.theta.cpu().numpy().copy()
    stats = es.step()
    assert stats["generation"] == 0 and es.generation == 1 and stats["worst"] <= stats["mean"] <= stats["best"]
    # by hand
    h = Handle(24, 2)
    eps = h.noise(E2E["seed"], 0).cpu().numpy()
    h.close()
    pop = S.members(theta0, E2E["sigma"], eps)
    _bits_equal(es.members.cpu().numpy(), pop, "members")
    bank = MfmaPolicyBank(24, 4, 0)
    for p in range(4):
        bank.set_weights(p, _layers(pop[p], 24))
    env.seed(E2E["seed"])
    env.reset_device()
    env.share_starts(256)
    rec = torch.zeros((1024, S.REC_INTS), dtype=torch.int32, device=DEV)
    recf = torch.zeros((1024, S.REC_FLOATS), device=DEV)
    env.evaluate_bank_device(bank, 4, 256, 64, default_gates_per_lap(env), rec, recf, precision=es.precision)
    assert torch.equal(rec, es.rec) and torch.equal(recf.view(torch.int32), es.recf.view(torch.int32))
    w = dict(E2E["fitness"], no_lap_steps=64.0)
    s = S.summary(rec.cpu().numpy(), recf.cpu().numpy(), 256)
    F = S.score(s, w, 256)
    _bits_equal(es.summary.cpu().numpy(), s, "summary")
    _bits_equal(es.scores.cpu().numpy(), F, "scores")
    assert s[:, 1].sum() + s[:, 2].sum() > 0 and len(set(F.tolist())) > 1      # episodes ended, and the members differ
    z = np.zeros_like(theta0)
    want = S.update(theta0, z, z, F, eps, E2E["sigma"], S.SHAPE_CENTERED_RANK, E2E["lr"], 0.9, 0.999, 1e-8, E2E["weight_decay"], 1)
    for name, got, ref in zip(("theta", "m", "v"), (es.theta, es.m, es.v), want[:3]):
        _bits_equal(got.cpu().numpy(), ref, name)
    assert stats["best"] == float(np.max(F)) and stats["best_crashes_per_env"] == s[int(np.argmax(F)), 1] / 256
    bank.close()
    es.close()


def test_two_steps_equal_a_step_a_state_round_trip_and_a_step():
    from optimal_quad_control_rl_amd import EvolutionStrategy

    env = _race_env(1024)
    a = EvolutionStrategy(env, _actor(24), eval_seeds="per_generation", **E2E)
    a.step()
    a.step()
    b = EvolutionStrategy(env, _actor(24), eval_seeds="per_generation", **E2E)
    b.step()
    sd = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}
    c = EvolutionStrategy(env, _actor(24, seed=9), eval_seeds="fixed", **{**E2E, "sigma": 0.5, "lr": 1.0, "seed": 1})   # everything comes from the state
    c.load_state_dict(sd)
    assert c.generation == 1 and c.eval_seed() == E2E["seed"] + 1
    c.step()
    for name in ("theta", "m", "v"):
        _bits_equal(getattr(a, name).cpu().numpy(), getattr(c, name).cpu().numpy(), name)
    # write_back: the actor a model keeps is theta
    target = _actor(24, seed=3)
    a.write_back(target)
    flat = torch.cat([p.detach().reshape(-1) for lin in target if isinstance(lin, torch.nn.Linear) for p in (lin.weight, lin.bias)])
    assert torch.equal(flat.view(torch.int32), a.theta.view(torch.int32))
    for x in (a, b, c):
        x.close()


# ---- the synthetic ascent on the device ------------------------------------------------------------------------------------------------------
def test_device_ascends_the_synthetic_score():
    """tests/test_es_host.py's problem and settings with the callable fitness: the distance of theta[:K] to the target decreases."""
    from optimal_quad_control_rl_amd import EvolutionStrategy, Quadcopter3DGatesINDI, square_track

    A = S.ASCENT
    K = A["K"]
    env = Quadcopter3DGatesINDI(2 * A["pairs"] * 256, *square_track(), gates_ahead=0, seed=1, infos_mode="none")
    holder = {}

    def score(rec, recf):
        pop = holder["es"].members[:, :K].double()
        return -((pop - holder["target"]) ** 2).sum(1)

    es = EvolutionStrategy(env, _actor(13), pairs=A["pairs"], envs_per_policy=256, sigma=A["sigma"], lr=A["lr"], betas=A["betas"], eps=A["eps"],
                           fitness=score, n_eval_steps=4, seed=A["seed"])
    holder["es"], holder["target"] = es, (es.theta[:K].double() + torch.as_tensor(S.ascent_offset(), device=DEV).double())
    dist = lambda: float((es.theta[:K].double() - holder["target"]).norm())
    d0 = dist()
    es.learn(A["generations"])
    d1 = dist()
    print("device ascent: |theta[:K] - target| %.3f -> %.3f in %d generations" % (d0, d1, A["generations"]))
    assert es.generation == A["generations"] and d1 < d0
    es.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_and_the_bank_untouched():
    from optimal_quad_control_rl_amd.policy import MfmaPolicyBank

    lib = _lib.load()
    out = C.c_void_p()
    for obs_len, pairs in ((14, 2), (13, 0), (13, 129)):
        assert lib.qr_es_create(obs_len, 0, pairs, C.byref(out)) == _lib.QR_E_INVALID and not out.value
    assert lib.qr_es_create(13, 0, 2, None) == _lib.QR_E_INVALID
    h = Handle(13, 2)
    P, n, E, st = h.P, h.n, 256, _stream()
    bank, other = _marked_bank(13, P + 1), MfmaPolicyBank(20, P + 1, 0)
    images = {s: [_read(bank, s, w) for w in (0, 1)] for s in range(P + 1)}
    f32 = lambda *shape: torch.full(shape, SENTINEL, device=DEV)
    f64 = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device=DEV)
    eps, pop, theta, m, v, util, summ, fit = f32(h.pairs, n), f32(P, n), f32(n), f32(n), f32(n), f32(P), f64(P, 8), f64(P)
    rec = torch.full((P * E + 1, S.REC_INTS), 7, dtype=torch.int32, device=DEV)
    recf = f32(P * E, S.REC_FLOATS)
    w = _lib.QrEsFitnessWeights(0, 0, 0, 0, -1, 1200)
    nan, inf = float("nan"), float("inf")
    odd = lambda t: C.c_void_p(t.data_ptr() + 4)
    perturb = lambda es=h.h, th=_p(theta), sigma=0.1, bk=bank._h, first=0, tp=_p(pop): lib.qr_es_perturb(es, th, sigma, 1, 0, bk, first, tp, st)
    fitness = lambda es=h.h, r=_p(rec), e=E, ww=C.byref(w), f=_p(fit): lib.qr_es_fitness(es, r, _p(recf), e, ww, _p(summ), f, st)
    update = lambda es=h.h, th=_p(theta), mm=_p(m), vv=_p(v), f=_p(fit), sigma=0.1, shaping=0, lr=0.01, t=1: lib.qr_es_update(
        es, th, mm, vv, f, sigma, 1, 0, shaping, lr, 0.9, 0.999, 1e-8, 0.0, t, _p(util), st)
    cases = {
        "noise: NULL handle": lambda: lib.qr_es_noise(None, 1, 0, _p(eps), st),
        "noise: NULL eps": lambda: lib.qr_es_noise(h.h, 1, 0, None, st),
        "noise: misaligned eps": lambda: lib.qr_es_noise(h.h, 1, 0, odd(eps), st),
        "perturb: NULL handle": lambda: perturb(es=None), "perturb: NULL theta": lambda: perturb(th=None), "perturb: NULL bank": lambda: perturb(bk=None),
        "perturb: sigma 0": lambda: perturb(sigma=0.0), "perturb: sigma < 0": lambda: perturb(sigma=-0.1), "perturb: sigma NaN": lambda: perturb(sigma=nan),
        "perturb: sigma inf": lambda: perturb(sigma=inf), "perturb: first_slot < 0": lambda: perturb(first=-1),
        "perturb: first_slot + P > capacity": lambda: perturb(first=2), "perturb: another obs_len": lambda: perturb(bk=other._h),
        "perturb: misaligned theta": lambda: perturb(th=odd(theta)), "perturb: misaligned theta_pop": lambda: perturb(tp=odd(pop)),
        "fitness: NULL handle": lambda: fitness(es=None), "fitness: NULL rec": lambda: fitness(r=None), "fitness: NULL weights": lambda: fitness(ww=None),
        "fitness: NULL fitness": lambda: fitness(f=None), "fitness: E < 256": lambda: fitness(e=128), "fitness: E not a multiple": lambda: fitness(e=300),
        "fitness: E 0": lambda: fitness(e=0), "fitness: misaligned rec": lambda: fitness(r=odd(rec)),
        "update: NULL handle": lambda: update(es=None), "update: NULL theta": lambda: update(th=None), "update: NULL m": lambda: update(mm=None),
        "update: NULL v": lambda: update(vv=None), "update: NULL fitness": lambda: update(f=None), "update: sigma 0": lambda: update(sigma=0.0),
        "update: sigma NaN": lambda: update(sigma=nan), "update: sigma inf": lambda: update(sigma=inf), "update: sigma < 0": lambda: update(sigma=-1.0),
        "update: lr < 0": lambda: update(lr=-1e-3), "update: lr NaN": lambda: update(lr=nan), "update: adam_step 0": lambda: update(t=0),
        "update: adam_step < 0": lambda: update(t=-3), "update: shaping 2": lambda: update(shaping=2), "update: shaping -1": lambda: update(shaping=-1),
    }
    for what, call in cases.items():
        assert call() == _lib.QR_E_INVALID, what
        assert len(lib.qr_last_error()) > 0, what
    torch.cuda.synchronize()
    for name, t in (("eps", eps), ("theta_pop", pop), ("theta", theta), ("m", m), ("v", v), ("util", util), ("summary", summ), ("fitness", fit),
                    ("recf", recf)):
        assert bool((t == SENTINEL).all()), name
    assert bool((rec == 7).all())
    for s in range(P + 1):
        for which in (0, 1):
            assert np.array_equal(_read(bank, s, which), images[s][which]), (s, which)
    buf = np.zeros(_image_bytes(20) // 2, dtype=np.uint16)
    assert lib.qr_policy_bank_read(other._h, 0, 0, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == _lib.QR_E_INVALID   # still unset
    bank.close()
    other.close()
    h.close()


# ---- time ------------------------------------------------------------------------------------------------------------------------------
def test_perturb_is_no_slower_than_the_bank_set_loop_and_the_split_of_a_generation():
    """P = 256, L = 24.  qr_es_perturb (two launches, synchronised) against what the tree offered for the same 256 filled slots before:
    256 qr_policy_bank_set calls from host copies of theta_pop (DESIGN section 8 measured 0.93 ms per slot).  Medians of 9, alternating;
    asserted <= 1 x, the ratio printed.  Then the split of one generation at 65 536 envs x 1200 steps, printed without a bound (no number
    existed for it)."""
    from optimal_quad_control_rl_amd import EvolutionStrategy
    from optimal_quad_control_rl_amd.policy import MfmaPolicyBank

    L, pairs = 24, 128
    h = Handle(L, pairs)
    P, n = h.P, h.n
    th = torch.as_tensor(_theta(n, seed=1, planted=False), device=DEV)
    pop = torch.empty((P, n), device=DEV)
    got, ref = MfmaPolicyBank(L, P, 0), MfmaPolicyBank(L, P, 0)

    def device_route():
        _lib.check(h.lib.qr_es_perturb(h.h, _p(th), 0.05, 3, 0, got._h, 0, _p(pop), _stream()))
        torch.cuda.synchronize()

    device_route()
    rows = [_layers(r, L) for r in pop.cpu().numpy()]

    def host_route():
        for p in range(P):
            ref.set_weights(p, rows[p])
        torch.cuda.synchronize()

    host_route()
    ta, tb = [], []
    for _ in range(9):
        t0 = time.perf_counter(); device_route(); t1 = time.perf_counter(); host_route(); t2 = time.perf_counter()
        ta.append(t1 - t0); tb.append(t2 - t1)
    a, b = float(np.median(ta)), float(np.median(tb))
    print("qr_es_perturb P=256 L=24: %.3f ms; 256 x qr_policy_bank_set: %.3f ms (%.3f ms per slot); ratio %.4f" % (a * 1e3, b * 1e3, b * 1e3 / P, a / b))
    for p in (0, 1, 128, 255):
        assert np.array_equal(_read(got, p, 0), _read(ref, p, 0)) and np.array_equal(_read(got, p, 1), _read(ref, p, 1))
    assert a <= b, (a, b)
    for x in (got, ref):
        x.close()
    h.close()
    # the split of one generation: perturb / evaluate / fitness / update
    env = _race_env(P * 256, max_steps=1200)
    es = EvolutionStrategy(env, _actor(L), pairs=pairs, envs_per_policy=256, n_eval_steps=1200, seed=0)
    es.step()   # warm-up
    lib, st, g = es._L, es._stream(), es.generation
    w = es._weights_struct()
    marks = [time.perf_counter()]

    def mark():
        torch.cuda.synchronize()
        marks.append(time.perf_counter())

    _lib.check(lib.qr_es_perturb(es._h, _p(es.theta), es.sigma, es.seed, g, es.bank._h, 0, _p(es.members), st)); mark()
    env.seed(es.eval_seed()); env.reset_device(); env.share_starts(256); es.rec.zero_(); es.recf.zero_(); mark()
    env.evaluate_bank_device(es.bank, P, 256, 1200, es.gates_per_lap, es.rec, es.recf, precision=es.precision); mark()
    _lib.check(lib.qr_es_fitness(es._h, _p(es.rec), _p(es.recf), 256, C.byref(w), _p(es.summary), _p(es.scores), st)); mark()
    _lib.check(lib.qr_es_update(es._h, _p(es.theta), _p(es.m), _p(es.v), _p(es.scores), es.sigma, es.seed, g, 0, es.lr, 0.9, 0.999, 1e-8, 0.0, g + 1, None, st)); mark()
    d = np.diff(marks) * 1e3
    print("one generation, P=256 x 256 envs x 1200 steps (one run): perturb %.3f ms, starts %.3f ms, evaluate %.3f ms, fitness %.3f ms, update %.3f ms"
          % tuple(d))
    es.close()
