"""GPU: the optimiser step of ppo_apply_kernel (qr_ppo_apply / qr_ppo_minibatch) against a float64 restatement of torch's
clip_grad_norm_ + Adam, fed the float32 theta, m, v, gradient and hyper-parameters the kernel receives, at every observation length.

    clip = min(1, max_norm / (|g| + 1e-6));  m' = b1 m + (1 - b1) clip g;  v' = b2 v + (1 - b2) (clip g)^2
    theta' = theta - lr / bc1 * m' / (sqrt(v') / sqrt(bc2) + eps),  bc_k = 1 - b_k^t

Bounds, from the float32 operation count (u = 2^-24, one rounding <= u / 2 relative):
  * clip: the squared norm is summed in double but rounded to float32 once per workgroup and once in total (2 u / 2), sqrt, + 1e-6 and
    the division add 3 u / 2: |clip - clip64| <= 2.5 u clip.  Asserted separately through m' from a zero m: <= 1e-6 relative (17 u).
  * m': clip g (+ u / 2), times (1 - b1) (+ u / 2), b1 m (u / 2), the sum (u / 2):  |dm| <= 4 u (b1 |m| + (1 - b1) |clip g|), asserted
    with 6 u.  The bound is on the sum of the terms' magnitudes, not on |m'|: b1 m and (1 - b1) clip g may cancel.
  * v': (clip g)^2 carries 2 x 3 u / 2 + u / 2, then as m':  |dv| <= 5 u (b2 v + (1 - b2) (clip g)^2), asserted with 8 u.
  * theta: sqrt(v') <= 2.5 u + u / 2, / bc2_sqrt u, + eps u / 2, the division u / 2, lr / bc1 u / 2, the product u / 2, m' 4 u:
    <= 9.5 u = 5.7e-7 relative to the step; asserted with 2e-6 relative, plus what the absolute m' bound contributes where its terms
    cancel (lr / bc1 * dm_bound / denominator), plus one ulp of theta' (the subtraction), plus the bias corrections: the kernel forms
    bc_k = 1 - powf(b_k, t) in float32 (torch: in double), and powf's 2-ulp error in b^t is amplified by b^t / (1 - b^t) in the
    difference (t >= 2; powf(b, 1) is exact) -- 2 u b1^t / bc1 + u / 2 for bc1, half of 2 u b2^t / bc2 + u / 2 plus the sqrt's u / 2 for bc2_sqrt.  With b2 = 0.999
    at t = 2 that term alone is 3e-5 relative (b2^2 / bc2 ~ 500): the f32 bias corrections, not the update arithmetic, set the bound at
    small t.
Each test prints the largest measured error / bound ratio."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import exact_net as E

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEV = torch.device("cuda", 0)


def _f(x):
    return float(np.float32(x))


def adam64(theta, m, v, g, t, lr, betas, eps, max_norm):
    """float64 restatement; inputs are the float32 tensors / values the kernel gets (g: the n parameter entries, no statistics)."""
    th, m, v, g = (x.detach().double().cpu() for x in (theta, m, v, g))
    b1, b2 = _f(betas[0]), _f(betas[1])
    clip = min(1.0, _f(max_norm) / (float(g.norm()) + 1e-6))
    gc = clip * g
    m1 = b1 * m + (1 - b1) * gc
    v1 = b2 * v + (1 - b2) * gc * gc
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    den = v1.sqrt() / math.sqrt(bc2) + _f(eps)
    th1 = th - _f(lr) / bc1 * m1 / den
    dm = 6 * U * (b1 * m.abs() + (1 - b1) * gc.abs())
    dv = 8 * U * (b2 * v.abs() + (1 - b2) * gc * gc)
    dth = _f(lr) / bc1 * dm / den
    pw = 0.0 if t == 1 else 2 * U   # powf(b, 1) = b exactly (and 1 - b is exact): at t = 1 only the roundings of the division and sqrt remain
    rel_bc = pw * b1 ** t / bc1 + U / 2 + 0.5 * (pw * b2 ** t / bc2 + U / 2) + U / 2
    return dict(theta=th1, m=m1, v=v1, clip=clip, dm=dm, dv=dv, dth=dth, th0=th, rel_bc=rel_bc)


def check_step(up, ref, label=""):
    """Asserts the kernel's (theta, m, v) against adam64's; returns the largest error / bound ratios."""
    th, m, v = (x.double().cpu() for x in (up.theta, up.m, up.v))
    em, ev = (m - ref["m"]).abs(), (v - ref["v"]).abs()
    d_ref, d = ref["theta"] - ref["th0"], th - ref["th0"]
    ulp = torch.from_numpy(np.spacing(np.abs(up.theta.cpu().numpy())).astype(np.float64))
    bth = (2e-6 + ref["rel_bc"]) * d_ref.abs() + ref["dth"] + ulp
    r = (float((em / ref["dm"].clamp_min(1e-45)).max()), float((ev / ref["dv"].clamp_min(1e-45)).max()),
         float(((d - d_ref).abs() / bth).max()))
    assert bool((em <= ref["dm"]).all()), (label, "m", r)
    assert bool((ev <= ref["dv"]).all()), (label, "v", r)
    assert bool(((d - d_ref).abs() <= bth).all()), (label, "theta", r)
    return r


def _updater(L, max_minibatch=4096, seed=1):
    from optimal_quad_control_rl_amd.ppo import MfmaPpoUpdater

    return MfmaPpoUpdater(E.to_actor_critic(L, seed).to(DEV), L, DEV, max_minibatch=max_minibatch)


def _heavy_tailed(n, gen, norm=None):
    """Magnitudes log-uniform in 1e-8 .. 1e2, random signs, 5 % exact zeros; optionally rescaled to a given global norm."""
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 10.0 - 8.0)
    sgn = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    g = mag * sgn * (torch.rand(n, generator=gen) >= 0.05).double()
    if norm is not None:
        g = g * (norm / float(g.norm()))
    return g.float()


HPARAMS = [((0.9, 0.999), 1e-5, 3e-4), ((0.8, 0.99), 1e-8, 1e-3), ((0.9, 0.999), 1e-5, 0.0)]
STEPS = (0, 1, 9, 999, 10 ** 6)


@pytest.mark.parametrize("L", E.OBS_LENS)
def test_apply_matches_float64_adam_and_clip(L):
    """qr_ppo_apply with an external gradient: fresh and random Adam state, device step counts 0, 1, 9, 999 and 10^6 (set through the step
    setter: bias corrections at t = 1 .. 10^6 + 1), the default and other betas / eps, lr = 0, a gradient norm below max_grad_norm (no clip)
    and far above it (clip ~ 1e-4).  m', v', theta' within the bounds of the module docstring; the clip coefficient implied by m' from a
    zero m within 1e-6 of float64; the caller-counted mode (adam_step = t through the ABI) gives the same bits as the device count."""
    up = _updater(L)
    n = up.theta.numel()
    gen = torch.Generator().manual_seed(L)
    theta0 = up.theta.clone()
    worst = [0.0, 0.0, 0.0, 0.0]
    for state in ("fresh", "random"):
        if state == "fresh":
            m0, v0 = torch.zeros(n), torch.zeros(n)
        else:
            m0 = (torch.randn(n, generator=gen) * 1e-3).float()
            v0 = (10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 8.0 - 12.0)).float()
        for clipped in (False, True):
            g = _heavy_tailed(n, gen, norm=None if clipped else 0.3)
            gfull = torch.cat([g, torch.zeros(4)]).to(DEV)
            for betas, eps, lr in HPARAMS:
                for t0 in STEPS:
                    up.theta.copy_(theta0); up.m.copy_(m0); up.v.copy_(v0)
                    up.betas, up.eps = betas, eps
                    up.control(None, clear=True)
                    up.step = t0
                    up.apply(gfull, lr=lr, B=1000, max_grad_norm=0.5)
                    assert up.status() == (False, 1, 0, 0) and up.step == t0 + 1
                    ref = adam64(theta0, m0, v0, g, t0 + 1, lr, betas, eps, 0.5)
                    assert (ref["clip"] < 1e-3) if clipped else ref["clip"] == 1.0
                    r = check_step(up, ref, (state, clipped, betas, lr, t0))
                    worst[:3] = [max(a, b) for a, b in zip(worst[:3], r)]
                    if lr == 0.0:
                        assert torch.equal(up.theta, theta0)
                    if state == "fresh":
                        big = g.abs() > 1e-3 * float(g.abs().max())
                        implied = up.m.double().cpu()[big] / ((1 - _f(betas[0])) * g.double()[big])
                        rel = float((implied.median() - ref["clip"]).abs() / ref["clip"])
                        worst[3] = max(worst[3], rel / 1e-6)
                        assert rel <= 1e-6, rel
                    # the ABI's caller-counted mode at the same t: the same bits
                    if state == "random" and lr != 0.0:
                        got = (up.theta.clone(), up.m.clone(), up.v.clone())
                        up.theta.copy_(theta0); up.m.copy_(m0); up.v.copy_(v0)
                        up._lib.check(up._L.qr_ppo_apply(up._h, *[C.c_void_p(x.data_ptr()) for x in (up.theta, up.m, up.v, gfull)],
                                                         1000, 0.5, lr, betas[0], betas[1], eps, t0 + 1, None, up._stream()))
                        assert all(torch.equal(a, b) for a, b in zip(got, (up.theta, up.m, up.v))), (t0, betas)
    print("L=%d: error / bound  m %.3f  v %.3f  theta %.3f  clip %.3f" % (L, *worst))
    up.close()


@pytest.mark.parametrize("L", E.OBS_LENS)
def test_minibatch_step_matches_float64_adam_on_its_own_gradient(L):
    """qr_ppo_minibatch (internal reduction, DenseMap thread -> parameter order, grid-barrier norm) from a snapshot (theta, m, v, t): the
    step equals the restatement fed g = qr_ppo_grad of the same rows (the same gradient and reduction kernels: deterministic, so the same
    g), within the same bounds."""
    from test_gpu_ppo_kernel import _setup

    pol, ref_net, up, obs, act, old_lp, adv, ret = _setup(L, 8192, seed=50 + L, max_minibatch=4096)
    n = up.theta.numel()
    gen = torch.Generator().manual_seed(L)
    up.m.copy_((torch.randn(n, generator=gen) * 1e-4).to(DEV))
    up.v.copy_((10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 6.0 - 12.0)).float().to(DEV))
    worst = [0.0, 0.0, 0.0]
    perm = torch.randperm(8192, device=DEV, generator=torch.Generator(device=DEV).manual_seed(L)).to(torch.int32)
    for k, (t0, B) in enumerate(((0, 2048), (7, 1000), (999, 4096))):
        idx = perm[k * 2048:k * 2048 + B].contiguous()
        up.control(None, clear=True)
        up.step = t0
        th0, m0, v0 = up.theta.clone(), up.m.clone(), up.v.clone()
        g = up.grad(obs, act, old_lp, adv, ret, idx, 0.2, 0.5, 0.01).clone()
        up.minibatch(obs, act, old_lp, adv, ret, idx, lr=3e-4, clip=0.2, vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5)
        assert up.status() == (False, 1, 0, 0) and up.step == t0 + 1
        ref = adam64(th0, m0, v0, g[:n], t0 + 1, 3e-4, up.betas, up.eps, 0.5)
        r = check_step(up, ref, (t0, B))
        worst = [max(a, b) for a, b in zip(worst, r)]
    print("L=%d minibatch: error / bound  m %.3f  v %.3f  theta %.3f" % (L, *worst))
    up.close()


@pytest.mark.parametrize("path", ["apply", "minibatch"])
def test_target_kl_boundary_and_nonfinite_gradients_are_device_decisions(path):
    """SB3's target-KL stop at its boundary: with S = the minibatch's KL sum, target_kl = S / (1.5 B) (1 + 1e-3) takes the step and
    (1 - 1e-3) takes none -- theta, m, v and the step count untouched, the stop flag set.  A +inf and a NaN gradient element are each
    skipped and counted without advancing t; the next finite step matches the restatement at bias correction t + 1."""
    from test_gpu_ppo_kernel import _setup

    L, B = 24, 2048
    pol, ref_net, up, obs, act, old_lp, adv, ret = _setup(L, 8192, seed=77, max_minibatch=4096)
    n = up.theta.numel()
    idx = torch.randperm(8192, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))[:B].to(torch.int32).contiguous()
    up.control(None, clear=True)
    up.minibatch(obs, act, old_lp, adv, ret, idx, lr=3e-4)     # a non-zero Adam state
    g = up.grad(obs, act, old_lp, adv, ret, idx, 0.2, 0.5, 0.0).clone()
    S = float(g[n + 2])
    assert S > 1e-3 * B

    def step():
        if path == "apply":
            up.apply(g, lr=3e-4, B=B)
        else:
            up.minibatch(obs, act, old_lp, adv, ret, idx, lr=3e-4)

    for side, stops in ((1.0 - 1e-3, True), (1.0 + 1e-3, False)):
        up.control(S / (1.5 * B) * side, clear=True)
        t0 = up.step
        before = (up.theta.clone(), up.m.clone(), up.v.clone())
        step()
        st = up.status()
        if stops:
            assert st == (True, 0, 0, 0) and up.step == t0
            assert all(torch.equal(a, b) for a, b in zip(before, (up.theta, up.m, up.v)))
        else:
            assert st == (False, 1, 0, 0) and up.step == t0 + 1
            check_step(up, adam64(*before, g[:n], t0 + 1, 3e-4, up.betas, up.eps, 0.5), ("kl", side))
    if path == "minibatch":
        return
    up.control(None, clear=True)
    t0 = up.step
    before = (up.theta.clone(), up.m.clone(), up.v.clone())
    for k, bad in enumerate((float("inf"), float("nan"))):
        gb = g.clone()
        gb[123] = bad
        up.apply(gb, lr=3e-4, B=B)
        assert up.status() == (False, 0, k + 1, 0) and up.step == t0
        assert all(torch.equal(a, b) for a, b in zip(before, (up.theta, up.m, up.v)))
    up.apply(g, lr=3e-4, B=B)
    assert up.status() == (False, 1, 2, 0) and up.step == t0 + 1
    r = check_step(up, adam64(*before, g[:n], t0 + 1, 3e-4, up.betas, up.eps, 0.5), "after non-finite")
    print("after the skipped steps: error / bound  m %.3f  v %.3f  theta %.3f" % r)
    up.close()
