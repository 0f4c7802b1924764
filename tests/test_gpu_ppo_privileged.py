"""GPU: the update half of the PRIVILEGED CRITIC -- qr_ppo_grad_privileged / qr_ppo_minibatch_privileged / qr_ppo_epoch_privileged
(ppo_grad_kernel<L, PT, false, true>, csrc/quadrace_ppo_device.hpp: the value network's workgroups gather their rows from a second array)
and PPO(privileged_critic=True).  Model: include/quadrace.h.  Every comparison is bit for bit.

P1 (the split)   grad_privileged(obs = A, critic_obs = C): the actor's entries (log_std included) and stats 0, 2, 3 are qr_ppo_grad(obs = A)'s,
                 the critic's entries and stat 1 are qr_ppo_grad(obs = C)'s -- and NOT qr_ppo_grad(obs = A)'s: the select is reached.
P2 (the twin)    with critic_obs a different buffer of the same content every _privileged call leaves grad_out, theta, both Adam moments, both
                 operand images (through qr_ppo_forward), status, stats, the Adam step count and the shuffle state where its twin does.
P3               epoch_privileged as a replayed graph = the handle created with QR_PPO_NO_EPOCH_GRAPH; two epochs with device_shuffle = the
                 per-minibatch calls on the permutation the buffer holds; minibatch_privileged = grad_privileged + qr_ppo_apply.
                 The last one is asserted with the norm clip inactive (max_grad_norm = 1e30, where the update is elementwise) and under the
                 default clip of 0.5, one step from a fresh state.  (tests/test_gpu_ppo_kernel.py holds the TWIN pair to 2e-7 over three
                 steps, because the two apply forms sum the squared norm over different thread layouts; at these shapes one run on an MI355X
                 printed a largest difference of 0.0 in theta and both moments for the privileged pair and for the twin pair alike, which
                 the test prints next to each other before it asserts.)
Shapes: L in {13, 24, 36}; B = 64, 100 (a partial last group of 64) and B2 = 16 385: the launcher runs min(ceil(ceil(B / 64) / 2), 128)
workgroups per network (PpoOps::grad, qr_ppo::kFusedChunks = 128), so 129 passes of 128 rows = 257 groups of 64 = 64 * 256 + 1 rows is the
smallest minibatch at which a workgroup (workgroup 0) runs a second pass."""
import pytest
import torch

from test_gpu_ppo_kernel import _setup
from test_gpu_rollout_conditions import E, _force_rows
from test_gpu_command_history import _ppo_env, _theta
from test_gpu_sensing_grid import NOISY, _bits

pytestmark = pytest.mark.gpu

B2 = 64 * 2 * 128 + 1          # pairs = ceil(ceil(B / 64) / 2) = 129 > kFusedChunks = 128
assert (((B2 + 63) // 64) + 1) // 2 == 129 and ((((B2 - 1) + 63) // 64) + 1) // 2 == 128
HP = dict(clip=0.2, vf_coef=0.5, ent_coef=0.0)


def _net_params(L, O):
    return 120 * L + 120 + 2 * (120 * 120 + 120) + O * 120 + O


def _split(g, L):
    """grad_out [n + 4] -> (actor entries with log_std and stats 0, 2, 3; critic entries with stat 1)"""
    n_pi, n_vf = _net_params(L, 4), _net_params(L, 1)
    n = n_pi + n_vf + 4
    assert g.numel() == n + 4
    actor = torch.cat([g[:n_pi], g[n_pi + n_vf:n], g[n:n + 1], g[n + 2:n + 4]])
    critic = torch.cat([g[n_pi:n_pi + n_vf], g[n + 1:n + 2]])
    return actor, critic


def _other_rows(obs, seed):
    """rows that differ from `obs` in every entry"""
    gen = torch.Generator(device=obs.device).manual_seed(seed)
    other = (0.7 * obs + 0.9 * torch.randn(obs.shape, device=obs.device, generator=gen) + 0.25).contiguous()
    assert bool((other != obs).all())
    return other


# ---- P1 --------------------------------------------------------------------------------------------------------------------------------------
_P1 = [(L, B, f) for L in (13, 24, 36) for B in (64, 100, B2) for f in (0, 1)]


@pytest.mark.parametrize("L,B,flags", _P1, ids=["L%d-B%d-%s" % (L, B, "f32partials" if f else "bf16partials") for L, B, f in _P1])
def test_the_value_network_reads_its_own_rows(L, B, flags):
    pol, ref, up, A, act, old_lp, adv, ret = _setup(L, rows=B, seed=L + B, max_minibatch=B, flags=flags)
    Cr = _other_rows(A, 5)
    idx = torch.randperm(B, device=A.device, generator=torch.Generator(device=A.device).manual_seed(1)).to(torch.int32)
    args = (act, old_lp, adv, ret, idx)
    g_priv = up.grad(A, *args, **HP, critic_obs=Cr).clone()
    g_a = up.grad(A, *args, **HP).clone()
    g_c = up.grad(Cr, *args, **HP).clone()
    g_again = up.grad(A, *args, **HP, critic_obs=Cr).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g_priv).all()) and bool(g_priv[:-4].any())
    assert torch.equal(_bits(g_priv), _bits(g_again)), "the call repeats itself"
    (pa, pc), (aa, ac), (ca, cc) = _split(g_priv, L), _split(g_a, L), _split(g_c, L)
    assert torch.equal(_bits(pa), _bits(aa)), ("actor entries, log_std, stats 0 2 3 = qr_ppo_grad(obs = A)", int((pa != aa).sum()))
    assert torch.equal(_bits(pc), _bits(cc)), ("critic entries, stat 1 = qr_ppo_grad(obs = C)", int((pc != cc).sum()))
    assert float((pc != ac).float().mean()) > 0.9 and pc[-1] != ac[-1], "the critic entries are NOT those of qr_ppo_grad(obs = A): the select is reached"
    assert not torch.equal(aa, ca), "(and A and C give different actor gradients: the actor did not read C)"
    up.close()


# ---- P2, P3 ----------------------------------------------------------------------------------------------------------------------------------
def _state(up, obs, perm):
    torch.cuda.synchronize()
    return dict(theta=up.theta.clone(), m=up.m.clone(), v=up.v.clone(), pi=up.forward(0, obs).clone(), vf=up.forward(1, obs).clone(),
                stats=up.stats.clone(), perm=perm.clone(), status=up.status(), step=up.step, shuffle=up.shuffle_state())


def _same_states(x, y, what):
    for k in x:
        if isinstance(x[k], torch.Tensor):
            same = torch.equal(_bits(x[k]), _bits(y[k])) if x[k].dtype == torch.float32 else torch.equal(x[k], y[k])
            assert same, (what, k, int((x[k] != y[k]).sum()))
        else:
            assert x[k] == y[k], (what, k, x[k], y[k])


def _sequence(setup, critic, kl, B, lr=3e-4):
    """grad, two minibatches, one minibatch with a non-finite advantage (the guard), one epoch on the caller's permutation, two epochs
    with device_shuffle in one call; returns the gradient and the state after every phase"""
    pol, ref, up, obs, act, old_lp, adv, ret = setup
    dev = obs.device
    rows = 4 * B
    kw = {} if critic is None else dict(critic_obs=critic)
    gen = torch.Generator(device=dev).manual_seed(7)
    perm0 = torch.randperm(rows, device=dev, generator=gen).to(torch.int32)
    perm1 = torch.randperm(rows, device=dev, generator=gen).to(torch.int32)
    buf = torch.empty(rows, dtype=torch.int32, device=dev)
    out = []
    up.set_shuffle(99, 0)
    up.control(kl, clear=True); up.stats.zero_()
    g = up.grad(obs, act, old_lp, adv, ret, perm0[:B].contiguous(), **HP, stats=True, **kw).clone()
    out.append(_state(up, obs, buf.zero_()))
    for k in (1, 2):
        up.minibatch(obs, act, old_lp, adv, ret, perm0[k * B:(k + 1) * B].contiguous(), lr, **kw)
    out.append(_state(up, obs, buf))
    bad = adv.clone()
    bad[int(perm0[3 * B])] = float("nan")       # the minibatch's advantage mean, every normalised advantage and d log_std become NaN
    up.control(kl, clear=True)
    up.minibatch(obs, act, old_lp, bad, ret, perm0[3 * B:].contiguous(), lr, **kw)
    out.append(_state(up, obs, buf))
    assert torch.equal(out[-1]["theta"], out[-2]["theta"]) and (kl is not None or out[-1]["status"][1:3] == (0, 1)), "the non-finite guard dropped the update"
    up.control(kl, clear=True)
    buf.copy_(perm1)
    up.epoch(obs, act, old_lp, adv, ret, buf, B, lr, **kw)
    out.append(_state(up, obs, buf))
    up.control(kl, clear=True)
    up.epoch(obs, act, old_lp, adv, ret, buf, B, lr, num_epochs=2, device_shuffle=True, **kw)
    out.append(_state(up, obs, buf))
    assert out[-1]["shuffle"] == (99, 2) and out[-1]["status"][3] == 0
    return g, out, up


# target_kl = 2e-3: _setup's old log-probs carry noise of 0.15, an approximate KL of ~0.011 > 1.5 target_kl, so the early stop is reached
_P23 = [(B, f, kl) for B in (100, 1024) for f in (0, 1) for kl in (None, 2e-3)]


@pytest.mark.parametrize("B,flags,kl", _P23, ids=["B%d-%s-%s" % (B, "f32partials" if f else "bf16partials", "kl" if kl else "nokl") for B, f, kl in _P23])
def test_twin_and_composition(B, flags, kl):
    from optimal_quad_control_rl_amd.ppo import MfmaPpoUpdater

    L, lr = 24, 3e-4
    fresh = lambda fl=flags: _setup(L, rows=4 * B, seed=17, max_minibatch=B, flags=fl)
    # P2: the same content in another buffer
    t = fresh()
    g_t, s_t, up_t = _sequence(t, None, kl, B)
    p = fresh()
    copy = p[3].clone()
    assert copy.data_ptr() != p[3].data_ptr()
    g_p, s_p, up_p = _sequence(p, copy, kl, B)
    assert torch.equal(_bits(g_t), _bits(g_p)), "grad_out"
    for k, (x, y) in enumerate(zip(s_t, s_p)):
        _same_states(x, y, ("P2, phase", k))
    applied = [s["status"][1] for s in s_t]
    print("B", B, "flags", flags, "kl", kl, "applied per phase", applied, "stopped", [s["status"][0] for s in s_t])
    assert kl is not None or (applied[1], applied[3], applied[4]) == (2, 4, 8)
    assert kl is None or (s_t[3]["status"][0] or s_t[4]["status"][0]), "the early stop is reached with this target_kl"
    up_t.close(); up_p.close()
    # P3 with rows of its own: the graph against plain launches of the same handle form
    a, n = fresh(), fresh(flags | 8)
    Cr = _other_rows(a[3], 3)
    g_a, s_a, up_a = _sequence(a, Cr, kl, B)
    g_n, s_n, up_n = _sequence(n, Cr, kl, B)
    assert torch.equal(_bits(g_a), _bits(g_n))
    for k, (x, y) in enumerate(zip(s_a, s_n)):
        _same_states(x, y, ("P3, graph against QR_PPO_NO_EPOCH_GRAPH, phase", k))
    # (under this target_kl every phase stops before its first step -- applied is 0 throughout -- so only the runs without it can differ)
    assert kl is not None or not torch.equal(s_a[-1]["theta"], s_t[-1]["theta"]), "other critic rows, another update"
    up_n.close()
    # ... two epochs with device_shuffle against the per-minibatch calls on the permutation the buffer holds
    c = fresh()
    up_c = c[2]
    obs, act, old_lp, adv, ret = a[3:]
    up_c.theta.copy_(up_a.theta); up_c.m.copy_(up_a.m); up_c.v.copy_(up_a.v); up_c.step = up_a.step; up_c.pack()
    pa = torch.empty(4 * B, dtype=torch.int32, device=obs.device)
    for ep in range(2):
        up_a.control(kl, clear=True); up_c.control(kl, clear=True)
        up_a.epoch(obs, act, old_lp, adv, ret, pa, B, lr, device_shuffle=True, critic_obs=Cr)
        torch.cuda.synchronize()
        pc = pa.clone()
        assert torch.equal(torch.sort(pc.long()).values, torch.arange(4 * B, device=pc.device))
        up_c.begin_epoch(adv, pc, B)
        for k in range(4):
            up_c.minibatch(obs, act, old_lp, adv, ret, pc[k * B:(k + 1) * B], lr, critic_obs=Cr)
        torch.cuda.synchronize()
        for name in ("theta", "m", "v"):
            assert torch.equal(_bits(getattr(up_a, name)), _bits(getattr(up_c, name))), ("epoch against minibatches", ep, name)
        assert up_a.step == up_c.step and up_a.status()[:3] == up_c.status()[:3]
    up_c.close()
    # ... minibatch_privileged = grad_privileged + qr_ppo_apply (see the module text on the clip)
    idx = torch.arange(B, dtype=torch.int32, device=obs.device)
    for norm in (1e30, 0.5):
        pairs = {}
        for name, rows in (("privileged", Cr), ("twin", None)):
            kw = {} if rows is None else dict(critic_obs=rows)
            x, y = fresh(), fresh()
            for s in (x, y):
                s[2].control(None, clear=True)
            x[2].minibatch(obs, act, old_lp, adv, ret, idx, lr, max_grad_norm=norm, **kw)
            g = y[2].grad(obs, act, old_lp, adv, ret, idx, **HP, **kw)
            y[2].apply(g, lr, B, max_grad_norm=norm)
            torch.cuda.synchronize()
            assert x[2].step == y[2].step == 1
            pairs[name] = tuple(float((getattr(x[2], q) - getattr(y[2], q)).abs().max()) for q in ("theta", "m", "v"))
            if rows is not None:
                equal = all(torch.equal(_bits(getattr(x[2], q)), _bits(getattr(y[2], q))) for q in ("theta", "m", "v"))
            x[2].close(); y[2].close()
        print("minibatch against grad + apply, max_grad_norm %g: largest |difference| (theta, m, v) privileged %s twin %s" % (norm, pairs["privileged"], pairs["twin"]))
        assert equal, ("minibatch_privileged = grad_privileged + qr_ppo_apply, bit for bit", norm, pairs["privileged"])
    up_a.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from optimal_quad_control_rl_amd import _lib
    from optimal_quad_control_rl_amd.ppo import MfmaPpoUpdater

    L, B = 24, 128
    pol, ref, up, obs, act, old_lp, adv, ret = _setup(L, rows=B, seed=2, max_minibatch=B)
    Cr = _other_rows(obs, 1)
    idx = torch.arange(B, dtype=torch.int32, device=obs.device)
    lib, p = up._L, up._p
    g = torch.full((up.theta.numel() + 4,), 7.0, device=obs.device)
    theta0 = up.theta.clone()

    def grad(critic=Cr, o=obs, b=B, out=g):
        return lib.qr_ppo_grad_privileged(up._h, p(up.theta), p(o), p(critic), p(act), p(old_lp), p(adv), p(ret), p(idx), b, 0.2, 0.5, 0.0, p(out), None,
                                          up._stream())

    def minibatch(critic=Cr, o=obs, b=B, m=up.m, lr=3e-4, step=0):
        return lib.qr_ppo_minibatch_privileged(up._h, p(up.theta), p(m), p(up.v), p(o), p(critic), p(act), p(old_lp), p(adv), p(ret), p(idx), b, 0.2, 0.5,
                                               0.0, 0.5, lr, 0.9, 0.999, 1e-5, step, None, up._stream())

    def epoch(critic=Cr, o=obs, b=B, mbs=1, epochs=1, shuffle=0, lr=3e-4):
        return lib.qr_ppo_epoch_privileged(up._h, p(up.theta), p(up.m), p(up.v), p(o), p(critic), p(act), p(old_lp), p(adv), p(ret), p(idx), b, mbs,
                                           epochs, shuffle, 0.2, 0.5, 0.0, 0.5, lr, 0.9, 0.999, 1e-5, None, up._stream())

    def refused(call, message, **kw):
        rc = call(**kw)
        err = lib.qr_last_error()
        assert rc == _lib.QR_E_INVALID and message in err, (kw, rc, err)
        torch.cuda.synchronize()
        assert bool((g == 7.0).all()) and torch.equal(up.theta, theta0) and not bool(up.m.any())

    for call, who in ((grad, b"qr_ppo_grad_privileged"), (minibatch, b"qr_ppo_minibatch_privileged"), (epoch, b"qr_ppo_epoch_privileged")):
        refused(call, who + b": null critic_obs_dev", critic=None)
        refused(call, who + b": null critic_obs_dev", critic=None, o=None, b=1)       # ... ahead of the twin's own checks
    # the twin's argument checks, in its order
    refused(grad, b"qr_ppo: null argument", o=None, b=1, out=None)
    refused(grad, b"minibatch size must be >= 64", b=63, out=None)
    refused(grad, b"minibatch size must be >= 64", b=B + 64)
    refused(grad, b"qr_ppo_grad: null grad_out", out=None)
    refused(minibatch, b"learning rate must be >= 0", lr=-1.0, o=None)
    refused(minibatch, b"qr_ppo: null argument", o=None, m=None)
    refused(minibatch, b"bad Adam state", m=None)
    refused(minibatch, b"bad Adam state", step=-1)
    refused(epoch, b"qr_ppo_epoch: null argument", o=None, mbs=0)
    refused(epoch, b"bad minibatch size / count / learning rate", mbs=0, epochs=2)
    refused(epoch, b"bad minibatch size / count / learning rate", lr=float("nan"))
    refused(epoch, b"num_epochs > 1 needs device_shuffle", epochs=2)
    assert lib.qr_ppo_grad_privileged(None, *([None] * 8), B, 0.2, 0.5, 0.0, None, None, None) == _lib.QR_E_INVALID
    # the f32-class path and the data-parallel path have no privileged form: the Python layer says so before the library is called
    args = (obs, act, old_lp, adv, ret, idx)
    with pytest.raises(ValueError, match="f32-class gradient kernels .* have no privileged-critic form"):
        up.grad(*args, precision="f32", critic_obs=Cr)
    up32 = MfmaPpoUpdater(pol, L, obs.device, max_minibatch=B, precision="f32")
    for call in (lambda: up32.grad(*args, critic_obs=Cr), lambda: up32.minibatch(*args, 3e-4, critic_obs=Cr), lambda: up32.epoch(*args, B, 3e-4, critic_obs=Cr)):
        with pytest.raises(ValueError, match="no privileged-critic form"):
            call()
    MfmaPpoUpdater.force_data_parallel = True
    try:
        if MfmaPpoUpdater.data_parallel():      # (needs an initialised process group; the constructor-level refusal is tested without a GPU)
            with pytest.raises(ValueError, match="no data-parallel form"):
                up.minibatch(*args, 3e-4, critic_obs=Cr)
    finally:
        MfmaPpoUpdater.force_data_parallel = False
    torch.cuda.synchronize()
    assert bool((g == 7.0).all()) and torch.equal(up.theta, theta0)
    assert grad() == _lib.QR_OK and minibatch() == _lib.QR_OK and epoch() == _lib.QR_OK      # ... and valid calls run
    torch.cuda.synchronize()
    assert not bool((g == 7.0).any()) and not torch.equal(up.theta, theta0) and up.step == 2
    up.close(); up32.close()


# ---- PPO(privileged_critic=True) -------------------------------------------------------------------------------------------------------------
BUFFERS = ("buf_obs", "buf_act", "buf_lp", "buf_val", "buf_rew", "buf_done", "buf_term_val", "last_val", "ep_ret", "ep_len", "ep_gates")


def test_ppo_under_the_ideal_sensor_is_the_ppo_of_the_ideal_sensor():
    """three rounds: theta, Adam moments, buffers and stats bit for bit; ep_rew_mean within the bound of
    test_gpu_rollout_sensing.test_ppo_under_the_ideal_sensor_is_the_plain_fused_ppo, for the reason given there (the GAE kernel sums it with
    one float atomic per wave, in whatever order the waves arrive)"""
    from optimal_quad_control_rl_amd.ppo import PPO
    from optimal_quad_control_rl_amd.sensing import SensingParams

    T, n = 16, 768
    kw = dict(n_steps=T, seed=4, fused_collect=True, native_update=True)
    ea, eb = _ppo_env(n), _ppo_env(n)
    plain = PPO(ea, sensing=[SensingParams.ideal()], **kw)
    priv = PPO(eb, privileged_critic=True, **kw)
    assert [s.name for s in priv.sensing] == ["ideal"] and priv.stats["critic_input"] == "clean" and plain.stats["critic_input"] == "policy"
    assert plain.buf_critic_obs is None and tuple(priv.buf_critic_obs.shape) == tuple(priv.buf_obs.shape)
    for e in (ea, eb):
        _force_rows(e, n // E)
    calls = []
    launch = eb.rollout_policy_privileged_device
    eb.rollout_policy_privileged_device = lambda *a, **k: (calls.append(a[7]), launch(*a, **k))[1]
    running = torch.zeros(n, dtype=torch.float64, device=ea.device)
    ended = 0
    for rnd in range(3):
        for m in (plain, priv):
            m.collect(); m.train()
        assert torch.equal(_bits(priv.buf_critic_obs), _bits(priv.buf_obs)), "an ideal sensor: the clean rows are the policy's rows"
        abs_sum = 0.0
        for k in range(T):
            running += plain.buf_rew[k].double()
            d = plain.buf_done[k].double()
            abs_sum += float((running.abs() * d).sum())
            running *= 1.0 - d
        ended += int(plain.buf_done.sum())
        for name in BUFFERS:
            assert torch.equal(_bits(getattr(plain, name)), _bits(getattr(priv, name))), (rnd, name)
        assert torch.equal(_bits(_theta(plain)), _bits(_theta(priv))), (rnd, "theta")
        assert torch.equal(_bits(plain._updater.m), _bits(priv._updater.m)) and torch.equal(_bits(plain._updater.v), _bits(priv._updater.v)), (rnd, "Adam")
        assert int(plain._updater.step) == int(priv._updater.step) > 0
        assert set(priv.stats) == set(plain.stats)
        exact = [k for k in plain.stats if k not in ("ep_rew_mean", "critic_input")]
        assert repr({k: priv.stats[k] for k in exact}) == repr({k: plain.stats[k] for k in exact})
        if "ep_rew_mean" in plain.stats and plain.stats.get("episodes"):
            bound = 1.01 * 2 * (n // 64 - 1) * 2.0 ** -24 * abs_sum / plain.stats["episodes"]
            diff = abs(priv.stats["ep_rew_mean"] - plain.stats["ep_rew_mean"])
            print("round", rnd, "ep_rew_mean %.9g against %.9g: |difference| %.3e, bound %.3e" % (priv.stats["ep_rew_mean"], plain.stats["ep_rew_mean"], diff, bound))
            assert diff <= bound
    assert calls == [0, 0, 0] and ended >= n, "the H = 0 form of the launch, and every env's episode ended (time limit 30 inside 48 steps)"
    assert set(priv.state_dict()) == set(plain.state_dict()) | {"privileged_critic"}
    ea.close(); eb.close()


def test_ppo_under_a_noisy_sensor_with_a_command_history():
    from optimal_quad_control_rl_amd.ppo import PPO
    from optimal_quad_control_rl_amd.sensing import SensingParams

    n, T, H = 1024, 16, 2
    sensors = [SensingParams.from_sigma(NOISY, 2, name="noisy d=2")]
    kw = dict(n_steps=T, seed=4, fused_collect=True, native_update=True, sensing=sensors, command_history=H, privileged_critic=True)
    ea, eb, ec, ed = (_ppo_env(n) for _ in range(4))
    whole, first = PPO(ea, **kw), PPO(eb, **kw)
    L = ea.state_len
    W = L + 4 * H
    for e in (ea, eb):
        _force_rows(e, n // E)
    # after one collect: the values are those of the clean rows, and the updater is handed the clean rows
    whole.collect()
    up = whole._updater
    flat = lambda t: t.view(T * n, -1)
    assert tuple(whole.buf_critic_obs.shape) == (T, n, W)
    assert torch.equal(_bits(whole.buf_val.view(-1)), _bits(up.forward(1, flat(whole.buf_critic_obs)).contiguous())), "buf_val = forward(1, buf_critic_obs)"
    assert not torch.equal(whole.buf_val.view(-1), up.forward(1, flat(whole.buf_obs)).contiguous())
    assert float((whole.buf_critic_obs[..., :L] != whole.buf_obs[..., :L]).float().mean()) > 0.99, "the clean rows differ from the policy's rows"
    assert torch.equal(_bits(whole.buf_critic_obs[..., L:]), _bits(whole.buf_obs[..., L:])), "... and carry the same history"
    seen = []
    epoch = up.epoch
    up.epoch = lambda *a, **k: (seen.append((a[0].data_ptr(), k["critic_obs"].data_ptr(), tuple(k["critic_obs"].shape))), epoch(*a, **k))[1]
    obs, act, old_lp, adv, ret, rows = whole._train_prepare()
    idx = torch.arange(whole.batch_size, dtype=torch.int32, device=ea.device)
    args = (act, old_lp.contiguous(), adv.contiguous(), ret.contiguous(), idx)
    clean = flat(whole.buf_critic_obs)
    g_priv, g_obs, g_clean = (up.grad(*a, *args, **HP, **k).clone() for a, k in (((obs,), dict(critic_obs=clean)), ((obs,), {}), ((clean,), {})))
    (pa, pc), (oa, oc), (ca, cc) = _split(g_priv, W), _split(g_obs, W), _split(g_clean, W)
    assert torch.equal(_bits(pa), _bits(oa)) and torch.equal(_bits(pc), _bits(cc)) and not torch.equal(pc, oc), "P1 on the model's own buffers"
    whole._train_native(obs, args[0], args[1], args[2], args[3], rows)
    assert seen and all(s == (whole.buf_obs.data_ptr(), whole.buf_critic_obs.data_ptr(), (T * n, W)) for s in seen), "the updater received the clean rows"
    up.epoch = epoch
    assert whole.stats["critic_input"] == "clean" and whole.stats["per_sensor"][0]["name"] == "noisy d=2"
    # save, load and continue equals the uninterrupted run
    for _ in range(2):
        whole.collect(); whole.train()
    for _ in range(2):
        first.collect(); first.train()
    sd, params = first.state_dict(), {k: v.clone() for k, v in first.policy.state_dict().items()}
    assert sd["privileged_critic"] is True and sd["command_history"] == H and sd["stats"]["critic_input"] == "clean"
    resumed = PPO(ec, **kw)
    resumed.policy.load_state_dict(params)
    resumed.load_state_dict(sd)
    resumed.collect(); resumed.train()
    assert torch.equal(_bits(_theta(whole)), _bits(_theta(resumed))), "theta"
    for name in BUFFERS + ("buf_critic_obs", "_pending"):
        assert torch.equal(_bits(getattr(whole, name)), _bits(getattr(resumed, name))), name
    assert torch.equal(_bits(whole._updater.m), _bits(resumed._updater.m)) and torch.equal(_bits(whole._updater.v), _bits(resumed._updater.v))
    assert int(whole._done_u8.sum()) + int(first._done_u8.sum()) >= 1
    # a checkpoint of the other kind is refused, in both directions, before anything is loaded
    other = PPO(ed, **{**kw, "privileged_critic": False})
    theta = _theta(other).clone()
    assert "privileged_critic" not in other.state_dict() and other.buf_critic_obs is None
    with pytest.raises(ValueError, match="privileged_critic=True.*privileged_critic=False"):
        other.load_state_dict(sd)
    with pytest.raises(ValueError, match="privileged_critic=False.*privileged_critic=True"):
        resumed.load_state_dict(other.state_dict())
    assert torch.equal(theta, _theta(other))
    for e in (ea, eb, ec, ed):
        e.close()


# ---- time, printed ---------------------------------------------------------------------------------------------------------------------------
def test_privileged_epoch_time_is_printed():
    """Median us per call of qr_ppo_epoch_privileged against qr_ppo_epoch (one epoch of four minibatches, device shuffle, L = 28, replayed
    graph) at 16 384 and 131 072 rows: order-swapped pairs, one warm-up pair, medians of 6, host clock around a stream synchronise, lr = 0
    so that every replay does the same work.  Each workgroup gathers one row array either way; NO bound is asserted (DESIGN.md section 8
    and profiles/privileged_critic_time.txt hold the numbers of one run)."""
    import statistics
    import time

    L = 28
    for rows in (16384, 131072):
        B = rows // 4
        a, b = (_setup(L, rows=rows, seed=9, max_minibatch=B) for _ in range(2))
        Cr = _other_rows(a[3], 2)
        perm = {name: torch.empty(rows, dtype=torch.int32, device=Cr.device) for name in ("privileged", "twin")}
        stream = torch.cuda.current_stream(Cr.device)

        def timed(name):
            s, kw = (a, dict(critic_obs=Cr)) if name == "privileged" else (b, {})
            stream.synchronize()
            t0 = time.perf_counter()
            s[2].epoch(*s[3:], perm[name], B, 0.0, device_shuffle=True, **kw)
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e6

        t_p, t_t = [], []
        for rep in range(7):
            if rep % 2 == 0:
                x = timed("privileged"); y = timed("twin")
            else:
                y = timed("twin"); x = timed("privileged")
            if rep:
                t_p.append(x); t_t.append(y)
        mp, mt = statistics.median(t_p), statistics.median(t_t)
        print("update, %d rows (4 minibatches of %d, L %d): qr_ppo_epoch_privileged median %.2f us %s; qr_ppo_epoch median %.2f us %s; ratio %.4f"
              % (rows, B, L, mp, ["%.1f" % t for t in t_p], mt, ["%.1f" % t for t in t_t], mp / mt))
        assert mp > 0.0 and mt > 0.0
        a[2].close(); b[2].close()
