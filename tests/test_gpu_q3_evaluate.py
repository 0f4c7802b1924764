"""GPU: on-device evaluation of the predecessor envs (q3_evaluate_policy, q3_evaluate_policy_bank; include/quad3d.h).

Contract: handle A runs K steps in ONE kernel and writes one record per env; its twin B -- same kind, seed, env_id_base, track, limits,
thresholds and state -- does K x [float32 cast, qr_policy_forward, clamp, q3_step, q3_get_state] and hands what those launches returned
to tests/q3_eval_spec.py.  rec is equal, recf bit-equal, and A's state, targets, step and episode counters equal B's and those of a
third handle after q3_rollout_policy(QR_ROLLOUT_DETERMINISTIC).

Scenario: tests/test_gpu_q3_rollout_policy.py's (special rows that force goal / out of bounds / ground / pass / final pass / collision
inside the first step whatever the policy commands, max_steps = 20 inside K = 48 so every env meets the time limit at least twice) plus
one gates row at x = 10.5, which is out of bounds at the first step.  Every class is reached by construction; the tests assert that on
the SPEC's output before they compare anything."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import q3_eval_spec as spec
import test_gpu_q3_rollout_policy as rp

pytestmark = pytest.mark.gpu

K, MAX_STEPS = rp.K, rp.MAX_STEPS
KINDS, PRECISIONS = rp.KINDS, rp.PRECISIONS
SENT_I = -12345


def _oob_rows(n):
    return (7, n - 8)


def _start(kind, env):
    """The scenario state: rp._set_start, and for gates one more row (twice: first wave, tail wave) that is out of bounds before the step."""
    rp._set_start(kind, env)
    if kind == "gates":
        st, tg, sc = (x.cpu().numpy() for x in env.get_state_tensors())
        row = np.zeros(16)
        row[0], row[2] = 10.5, -1.5          # |x| > 10, above the ground (z points down), at rest: no plane crossing
        for i in _oob_rows(st.shape[0]):
            st[i], tg[i], sc[i] = row, 0, 0
        env.set_state_tensors(st, tg, sc)


def _full_state(env):
    return tuple(env.get_state_tensors()) + (env.get_episode_counts(),)


def _records(env, n=None):
    n = env.num_envs if n is None else n
    fr, rec = rp._tailed((n, 12), torch.int32, env.device)
    ff, recf = rp._tailed((n, 4), torch.float32, env.device)
    rec.zero_(); recf.zero_()
    return dict(rec=(fr, rec), recf=(ff, recf)), rec, recf


def _twin_inputs(kind, precision, pol, b, Kc):
    """K x [cast, forward, clamp, q3_step, q3_get_state] on handle b -> the spec's inputs."""
    keys = ("pre_state", "pre_target", "pre_steps", "post_target", "rew", "done", "trunc")
    out = {k: [] for k in keys}
    st, tg, sc = b.get_state_tensors()
    for _ in range(Kc):
        o = st.to(torch.float32).contiguous()
        u = pol.forward(o, precision=precision).clamp(-1.0, 1.0).contiguous()
        _, r2, d2, t2 = b.step_device(u)
        out["pre_state"].append(st); out["pre_target"].append(tg); out["pre_steps"].append(sc)
        out["rew"].append(r2.to(torch.float32, copy=True)); out["done"].append(d2.clone()); out["trunc"].append(t2.clone())
        st, tg, sc = b.get_state_tensors()
        out["post_target"].append(tg)
    return {k: torch.stack(v).cpu().numpy() for k, v in out.items()}


def _assert_every_class_reached(kind, rec):
    tot = rec.astype(np.int64).sum(axis=0)
    cols = [spec.STEPS, spec.SUCCESS, spec.TIMEOUT, spec.OOB, spec.SUCCESS_LEN, spec.ALL_LEN, spec.BEST]
    if kind == "gates":
        cols += [spec.GROUND, spec.COLLISION, spec.PASSES]
    for c in cols:
        assert tot[c] > 0, (kind, c, tot)
    if kind == "hover":
        assert tot[spec.GROUND] == 0 and tot[spec.COLLISION] == 0 and tot[spec.PASSES] == 0
    assert tot[10] == 0 and tot[11] == 0


@functools.lru_cache(maxsize=None)
def _single(kind, precision, n):
    """One evaluate_device call on A, the twin's launches on B and the spec on them, the deterministic rollout on C: shared below."""
    pol = rp._policy()
    a, b, c = rp._make(kind, n), rp._make(kind, n), rp._make(kind, n)
    for env in (a, b, c):
        _start(kind, env)
    flats, rec, recf = _records(a)
    a.evaluate_device(pol, K, rec, recf, precision=precision)
    inputs = _twin_inputs(kind, precision, pol, b, K)
    want = spec.evaluate(kind, max_steps=MAX_STEPS, **inputs)
    c.rollout_policy_device(pol, K, torch.zeros(4), deterministic=True, precision=precision)
    torch.cuda.synchronize()
    return dict(a=a, b=b, c=c, flats=flats, rec=rec, recf=recf, want=want, inputs=inputs)


@pytest.mark.parametrize("n", [100, 293, 1024])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_records_equal_the_spec_and_state_equals_the_twin(kind, precision, n):
    r = _single(kind, precision, n)
    want_rec, want_recf = r["want"]
    _assert_every_class_reached(kind, want_rec)
    # the special rows end the way they were built to (spec output, first full wave and tail wave)
    idx = rp._row_index(kind, n)
    i0 = r["inputs"]
    first = spec.classify(kind, i0["pre_state"][0], i0["pre_steps"][0], i0["rew"][0], i0["done"][0], i0["trunc"][0], MAX_STEPS)
    if kind == "hover":
        assert all(first[0][i] for i in idx["goal"]) and all(first[2][i] for i in idx["oob"])
    else:
        assert all(first[0][i] for i in idx["final"]) and all(first[3][i] for i in idx["ground"]) and all(first[4][i] for i in idx["collision"])
        assert all(first[2][i] for i in _oob_rows(n))
        assert all(want_rec[i, spec.PASSES] >= 1 for i in idx["pass"])
    assert first[1][n // 2]                                             # a time-limit end at the first step
    got_rec, got_recf = r["rec"].cpu().numpy(), r["recf"].cpu().numpy()
    assert np.array_equal(got_rec, want_rec), np.argwhere(got_rec != want_rec)[:8]
    assert np.array_equal(got_recf.view(np.uint32), want_recf.view(np.uint32))
    assert (got_rec[:, spec.STEPS] == K).all()
    for sa, sb, sc in zip(_full_state(r["a"]), _full_state(r["b"]), _full_state(r["c"])):
        assert torch.equal(sa, sb) and torch.equal(sa, sc)
    assert torch.equal(r["a"].states_tensor, r["a"].get_state_tensors()[0])   # the env's own buffer was refreshed
    rp._tails_intact(r["flats"])


@pytest.mark.parametrize("kind", KINDS)
def test_continuation(kind):
    """48 steps in one call equal 20 + 28 and 1 + 47 on the same record buffers."""
    n = 293
    whole = _single(kind, "f16-operands", n)
    for first in (20, 1):
        e = rp._make(kind, n)
        _start(kind, e)
        flats, rec, recf = _records(e)
        e.evaluate_device(rp._policy(), first, rec, recf)
        assert int(rec[:, spec.STEPS].max()) == first
        e.evaluate_device(rp._policy(), K - first, rec, recf)
        assert torch.equal(rec, whole["rec"]) and torch.equal(recf.view(torch.int32), whole["recf"].view(torch.int32)), first
        for sa, sb in zip(_full_state(whole["a"]), _full_state(e)):
            assert torch.equal(sa, sb)
        rp._tails_intact(flats)


@functools.lru_cache(maxsize=None)
def _layers(which):
    """Weights of the three bank policies: rp._policy(20.0), rp._zero_policy() and rp._policy(5.0), as arrays (same recipes)."""
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    if which == "zero":
        z = lambda *s: np.zeros(s, np.float32)
        return [(z(120, 16), z(120)), (z(120, 120), z(120)), (z(120, 120), z(120)), (z(4, 120), z(4))]
    torch.manual_seed(3)
    net = ActorCritic(16, 4).cuda()
    with torch.no_grad():
        net.pi[-1].weight.mul_(float(which))
    lin = [m for m in net.pi if isinstance(m, torch.nn.Linear)]
    return [(m.weight.detach().cpu().numpy().copy(), m.bias.detach().cpu().numpy().copy()) for m in lin]


BANK_POLICIES = (20.0, "zero", 5.0)


@functools.lru_cache(maxsize=None)
def _standalone(kind, precision, E, which):
    """evaluate_device of one bank policy on an E-env handle from the scenario state."""
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    pol = MfmaPolicy(16).set_weights(_layers(which))
    env = rp._make(kind, E)
    _start(kind, env)
    start = _full_state(env)
    _, rec, recf = _records(env)
    env.evaluate_device(pol, K, rec, recf, precision=precision)
    torch.cuda.synchronize()
    return dict(start=[x.clone() for x in start], rec=rec, recf=recf, end=_full_state(env))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P,E,precision", [(3, 256, "f16-operands"), (2, 512, "f16-operands"), (3, 256, "f32")])
def test_bank_groups_equal_standalone_evaluations(kind, P, E, precision):
    from optimal_quad_control_rl_amd.policy import MfmaPolicyBank

    alone = [_standalone(kind, precision, E, BANK_POLICIES[p]) for p in range(P)]
    if precision == "f16-operands" and E == 256:     # the first bank policy on the scenario is rp._policy() itself
        ref = rp._policy()
        from optimal_quad_control_rl_amd.policy import MfmaPolicy
        o = torch.randn(64, 16, device="cuda")
        assert torch.equal(ref.forward(o), MfmaPolicy(16).set_weights(_layers(20.0)).forward(o))
    _assert_every_class_reached(kind, alone[0]["rec"].cpu().numpy())
    n = P * E
    big = rp._make(kind, n)
    st, tg, sc = big.get_state_tensors()
    s0 = alone[0]["start"]
    st[:E], tg[:E], sc[:E] = s0[0], s0[1], s0[2]
    big.set_state_tensors(st, tg, sc)
    ep = big.get_episode_counts()
    ep[:E] = s0[3]
    big.set_episode_counts(ep)
    big.share_starts(E)
    for g in range(P):
        for x, y in zip(_full_state(big), s0):
            assert torch.equal(x[g * E:(g + 1) * E], y), g
    bank = MfmaPolicyBank(16, P)
    for p in range(P):
        bank.set_weights(p, _layers(BANK_POLICIES[p]))
    flats, rec, recf = _records(big)
    big.evaluate_bank_device(bank, P, E, K, rec, recf, precision=precision)
    torch.cuda.synchronize()
    end = _full_state(big)
    for p in range(P):
        rows = slice(p * E, (p + 1) * E)
        assert torch.equal(rec[rows], alone[p]["rec"]), p
        assert torch.equal(recf[rows].view(torch.int32), alone[p]["recf"].view(torch.int32)), p
        for x, y in zip(end, alone[p]["end"]):
            assert torch.equal(x[rows], y), p
    assert not torch.equal(recf[:E], recf[E:2 * E])    # the policies do fly differently
    rp._tails_intact(flats)
    bank.close()


def _p(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_leave_everything_untouched(kind):
    from optimal_quad_control_rl_amd import _lib
    from optimal_quad_control_rl_amd.policy import MfmaPolicy, MfmaPolicyBank

    INV, STATE = _lib.QR_E_INVALID, _lib.QR_E_STATE
    pol, pol24, empty = rp._policy(), MfmaPolicy(24).load_torch(rp._net(24)), MfmaPolicy(16)
    multi = torch.cuda.device_count() > 1

    def check(env, flats, before, call, cases, who):
        for name, kw, want in cases:
            rc = call(**kw)
            text = env._L.qr_last_error()
            assert rc == want, (name, rc, text)
            assert who in text, (name, text)
        torch.cuda.synchronize()
        for name, (flat, _) in flats.items():
            assert bool((flat == SENT_I).all()), name
        for x, y in zip(before, _full_state(env)):
            assert torch.equal(x, y)

    def sentinel_records(env):
        flats, rec, recf = _records(env)
        for flat, _ in flats.values():
            flat.fill_(SENT_I)
        return flats, rec, recf

    def trackless(n, dev):
        h = C.c_void_p()
        _lib.check(_lib.load().q3_create(1, n, dev.index or 0, 0, C.byref(h)))
        return h

    # ---- q3_evaluate_policy
    n = 100
    env = rp._make(kind, n)
    L = env._L
    flats, rec, recf = sentinel_records(env)
    before = [x.clone() for x in _full_state(env)]

    def single(env_h="own", pol_h=pol._h, Kc=4, flags=0, rec_p="own", recf_p="own"):
        return L.q3_evaluate_policy(env._h if env_h == "own" else env_h, pol_h, Kc, flags, _p(rec) if rec_p == "own" else rec_p,
                                    _p(recf) if recf_p == "own" else recf_p, None)

    cases = [("null env", dict(env_h=None), INV), ("null policy", dict(pol_h=None), INV), ("null rec", dict(rec_p=None), INV),
             ("num_steps 0", dict(Kc=0), INV), ("deterministic bit", dict(flags=1), INV), ("another flag bit", dict(flags=4), INV),
             ("negative flags", dict(flags=-1), INV), ("policy obs_len 24", dict(pol_h=pol24._h), INV),
             ("misaligned rec", dict(rec_p=_p(rec, 4)), INV), ("misaligned recf", dict(recf_p=_p(recf, 4)), INV),
             ("policy without weights", dict(pol_h=empty._h), STATE)]
    if multi:
        cases.append(("policy on another device", dict(pol_h=MfmaPolicy(16, 1).load_torch(rp._net(16))._h), INV))
    if kind == "gates":
        h = trackless(n, env.device)
        cases.append(("gates env without a track", dict(env_h=h), STATE))
    check(env, flats, before, single, cases, b"q3_evaluate_policy: ")
    if kind == "gates":
        L.q3_destroy(h)
    assert single(recf_p=None, flags=2) == _lib.QR_OK          # and the same arguments without a fault are accepted (recf may be NULL)
    torch.cuda.synchronize()
    assert bool((rec[:, 0] == SENT_I + 4).all()) and bool((recf == SENT_I).all())

    # ---- q3_evaluate_policy_bank
    P, E = 2, 256
    n = P * E
    env = rp._make(kind, n)
    flats, rec, recf = sentinel_records(env)
    before = [x.clone() for x in _full_state(env)]
    full, half, one, bank24 = MfmaPolicyBank(16, 2), MfmaPolicyBank(16, 2), MfmaPolicyBank(16, 1), MfmaPolicyBank(24, 2)
    for slot in range(2):
        full.set_weights(slot, _layers(20.0))
        bank24.load_torch(slot, rp._net(24))
    half.set_weights(0, _layers(20.0))
    one.set_weights(0, _layers(20.0))

    def banked(env_h="own", bank_h=full._h, Pc=P, Ec=E, Kc=4, flags=0, rec_p="own", recf_p="own"):
        return L.q3_evaluate_policy_bank(env._h if env_h == "own" else env_h, bank_h, Pc, Ec, Kc, flags, _p(rec) if rec_p == "own" else rec_p,
                                         _p(recf) if recf_p == "own" else recf_p, None)

    cases = [("null env", dict(env_h=None), INV), ("null bank", dict(bank_h=None), INV), ("null rec", dict(rec_p=None), INV),
             ("num_steps 0", dict(Kc=0), INV), ("deterministic bit", dict(flags=1), INV), ("another flag bit", dict(flags=4), INV),
             ("bank obs_len 24", dict(bank_h=bank24._h), INV), ("misaligned rec", dict(rec_p=_p(rec, 4)), INV),
             ("misaligned recf", dict(recf_p=_p(recf, 4)), INV), ("envs_per_policy 0", dict(Pc=2, Ec=0), INV),
             ("envs_per_policy negative", dict(Pc=2, Ec=-256), INV), ("envs_per_policy 128", dict(Pc=4, Ec=128), INV),
             ("envs_per_policy 384", dict(Pc=1, Ec=384), INV), ("P E != N", dict(Pc=1, Ec=256), INV), ("P E != N (more)", dict(Pc=2, Ec=512), INV),
             ("num_policies 0", dict(Pc=0, Ec=256), INV), ("num_policies above the capacity", dict(bank_h=one._h), INV),
             ("unset slot", dict(bank_h=half._h), STATE)]
    if multi:
        other = MfmaPolicyBank(16, 2, 1)
        for slot in range(2):
            other.set_weights(slot, _layers(20.0))
        cases.append(("bank on another device", dict(bank_h=other._h), INV))
    if kind == "gates":
        h = trackless(n, env.device)
        cases.append(("gates env without a track", dict(env_h=h), STATE))
    check(env, flats, before, banked, cases, b"q3_evaluate_policy_bank: ")
    assert banked(bank_h=half._h) == STATE and b"slot 1" in L.qr_last_error()
    if kind == "gates":
        L.q3_destroy(h)
    assert banked(recf_p=None) == _lib.QR_OK
    torch.cuda.synchronize()
    assert bool((rec[:, 0] == SENT_I + 4).all()) and bool((recf == SENT_I).all())
    rp._tails_intact({"rec": flats["rec"]})


def _actor(which):
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    torch.manual_seed(3)
    net = ActorCritic(16, 4).cuda()
    with torch.no_grad():
        if which == "zero":
            for p in net.pi.parameters():
                p.zero_()
        else:
            net.pi[-1].weight.mul_(float(which))
    return net.pi


@pytest.mark.parametrize("kind", KINDS)
def test_python_surface(kind):
    from optimal_quad_control_rl_amd import evaluate_q3_policies, evaluate_q3_policy, summarize_q3_eval
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    actors = [_actor(w) for w in BANK_POLICIES]
    env = rp._make(kind, 256)
    s1 = evaluate_q3_policy(actors[0], env, n_eval_steps=K, seed=11)
    s2 = evaluate_q3_policy(actors[0], env, n_eval_steps=K, seed=11)
    assert s1 == s2 and s1["envs"] == 256 and s1["steps"] == K and s1["episodes"] >= 2 * 256 - 16
    assert s1["episodes"] == s1["successes"] + s1["timeouts"] + s1["out_of_bounds"] + s1["ground"] + s1["collisions"]
    env.seed(11)
    env.reset_device()
    rec = torch.zeros((256, 12), dtype=torch.int32, device=env.device)
    recf = torch.zeros((256, 4), dtype=torch.float32, device=env.device)
    assert env.evaluate_device(MfmaPolicy(16).load_torch(actors[0]), K, rec, recf)[0] is rec
    assert summarize_q3_eval(rec, recf, env.dt) == s1
    assert evaluate_q3_policy(actors[0], env, n_eval_steps=K) != s1          # seed=None continues from where the env is
    with pytest.raises(ValueError):
        env.evaluate_device(MfmaPolicy(16).load_torch(actors[0]), K, rec[:, :8].contiguous(), recf)
    with pytest.raises(ValueError):
        env.evaluate_device(MfmaPolicy(16).load_torch(actors[0]), K, rec, recf, precision="f64")
    # three policies on a 512-env handle: two launches, the second padded; each equals a single evaluation on a 256-env handle
    big = rp._make(kind, 512)
    many = evaluate_q3_policies(actors, big, envs_per_policy=256, n_eval_steps=K, seed=0)
    assert len(many) == 3
    for p in range(3):
        assert many[p] == evaluate_q3_policy(actors[p], rp._make(kind, 256), n_eval_steps=K, seed=0), p
    assert many[0] != many[1]


def test_evaluator_not_slower_than_the_rollout_kernel():
    """N = 65 536, K = 200: launches of evaluate_device and of rollout_policy_device(deterministic=True) alternate in one process from the
    same state, timed with events; medians of 5 after a warm-up of each.  The yardstick is q3_rollout_policy, which this change leaves
    untouched.  Bound (hover, f16 operands): evaluator <= 1.03 x rollout, the allowance DESIGN.md section 8 gives the race evaluators over
    their rollout kernel; the evaluator does strictly less (no stores, no noise).  The other three forms and the 16 x 4096 bank launch
    are printed.  Measured on MI355X: see DESIGN.md section 8."""
    from optimal_quad_control_rl_amd.policy import MfmaPolicyBank

    n, Kt, reps = 65536, 200, 5
    pol = rp._policy()
    figures = {}
    dev = torch.device("cuda", torch.cuda.current_device())
    out = (torch.empty((Kt, n, 16), device=dev), torch.empty((Kt, n, 4), device=dev), torch.empty((Kt, n), device=dev),
           torch.empty((Kt, n), device=dev), torch.empty((Kt, n), dtype=torch.uint8, device=dev),
           torch.empty((Kt, n), dtype=torch.uint8, device=dev))
    rec = torch.zeros((n, 12), dtype=torch.int32, device=dev)
    recf = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    bank = MfmaPolicyBank(16, 16)
    for slot in range(16):
        bank.set_weights(slot, _layers(20.0))
    zeros4 = torch.zeros(4)

    def timed(prepare, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        prepare(); a.record(); fn(); b.record()
        return a, b

    for kind in KINDS:
        env = rp._make(kind, n, max_steps=1000)
        start = [x.clone() for x in env.get_state_tensors()]
        same_start = lambda: env.set_state_tensors(*start)   # (synchronises: every timed run starts on an idle device)
        for precision in PRECISIONS:
            evaluate = lambda: env.evaluate_device(pol, Kt, rec, recf, precision=precision)
            rollout = lambda: env.rollout_policy_device(pol, Kt, zeros4, deterministic=True, precision=precision, out=out)
            same_start(); evaluate(); same_start(); rollout()                     # one warm-up of each
            ev = [(timed(same_start, evaluate), timed(same_start, rollout)) for _ in range(reps)]
            torch.cuda.synchronize()
            a = float(np.median([x.elapsed_time(y) for (x, y), _ in ev]))
            b = float(np.median([x.elapsed_time(y) for _, (x, y) in ev]))
            figures[(kind, precision)] = (a, b)
            print("%s %s: evaluator %.3f ms, rollout %.3f ms, ratio %.3f" % (kind, precision, a, b, a / b))
        banked = lambda: env.evaluate_bank_device(bank, 16, 4096, Kt, rec, recf)
        same_start(); banked()
        ev = [timed(same_start, banked) for _ in range(reps)]
        torch.cuda.synchronize()
        print("%s f16-operands: bank 16 x 4096 %.3f ms" % (kind, float(np.median([x.elapsed_time(y) for x, y in ev]))))
    a, b = figures[("hover", "f16-operands")]
    assert a <= 1.03 * b, (a, b)
