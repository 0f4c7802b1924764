"""GPU: observation length 16 -- the raw-state observation of the predecessor envs (include/quad3d.h) -- in the policy and PPO kernels,
held to the checks the race envs' lengths are held to, with the same helpers: the f16-operand forward bit for bit against
tests/exact_net.py, the f32-class forward within tests/test_gpu_policy.py's bound, the f16 gradient bit for bit against
tests/exact_grad.py, the f32-class gradient within its propagated bound, and one minibatch step through Adam."""
import numpy as np
import pytest
import torch

import exact_grad as G
import exact_net as E
from test_gpu_exact_grad import _compare, _dev, _grad_with_kernel_log_std, _updater

pytestmark = pytest.mark.gpu

L = 16
NS = (1, 63, 64, 65, 100, 1000, 65536)


def test_policy_forward_is_bit_exact_at_16():
    """tests/test_gpu_exact_forward.py::test_policy_forward_is_bit_exact, at L = 16 (17 inputs with the bias: two layer-1 K-steps, the
    second one holding the bias column alone)."""
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    layers = E.make_net(L, 1)
    pol = MfmaPolicy(L).set_weights(layers)
    for n in NS:
        obs = E.make_obs(n, L, 11)
        out = pol.forward(torch.from_numpy(obs).cuda()).cpu()
        want = torch.from_numpy(E.forward64(layers, obs).astype(np.float32))
        assert torch.equal(out, want), (n, float((out - want).abs().max()))
    pol.close()


@pytest.mark.parametrize("n", [1, 63, 100, 1000, 65536])
def test_f32class_policy_matches_float64_torch_at_16(n):
    """tests/test_gpu_policy.py::test_f32class_policy_matches_float64_torch, at L = 16: error <= 4e-6 of the output scale against the
    float64 evaluation of the same float32 parameters."""
    from optimal_quad_control_rl_amd.policy import MfmaPolicy
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    torch.manual_seed(L * 1000 + n % 997)
    net = ActorCritic(L, 4).cuda()
    with torch.no_grad():
        for m in net.pi:
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
        net.pi[-1].weight.mul_(30.0)
    obs = (torch.randn(n, L, device="cuda") * 2.0).contiguous()
    obs[:, 9] *= 300.0                      # a body-rate column near the 1000 rad/s guard
    pol = MfmaPolicy(L).load_torch(net.pi)
    out = pol.forward(obs, precision="f32")
    out16 = pol.forward(obs)
    with torch.no_grad():
        ref64 = net.pi.double()(obs.double())
    scale = max(1.0, ref64.abs().max().item())
    err, err16 = (out.double() - ref64).abs().max().item(), (out16.double() - ref64).abs().max().item()
    print("n %d: f32-class error %.3e, f16-operand error %.3e, scale %.3g" % (n, err, err16, scale))
    assert out.shape == (n, 4)
    assert err <= 4e-6 * scale, (err, scale)


@pytest.mark.parametrize("B", [64, 100, 5000])
def test_grad_is_bit_exact_at_16(B):
    """tests/test_gpu_exact_grad.py::test_grad_is_bit_exact, at L = 16: both partial formats, both clips, both log-std settings."""
    ups = {}
    worst = 0.0
    for j, clip in enumerate(G.CLIPS):
        ls = G.LOG_STDS[j % 2]
        pi, vf = G.nets(L, 1)
        b = G.make_batch(L, B, 7 + j, pi, vf, ls)
        out = G.restate(b, pi, vf, clip, partial=("bf16", "f32"))
        args = _dev(b)
        for fmt in ("bf16", "f32"):
            up = ups[(fmt, ls)] = _updater(L, ls, fmt, max_b=5056)
            up.stats.zero_()
            g = up.grad(*args, clip=clip, vf_coef=G.VF_COEF, ent_coef=G.ENT_COEF, stats=True)
            worst = max(worst, _compare(g, *out[fmt], (L, B, clip, fmt)))
            assert torch.equal(up.stats.cpu(), g[-4:].cpu())
    print("L 16 B %d: largest error / bound of the log-std and statistics entries %.3g" % (B, worst))
    for up in ups.values():
        up.close()


def test_f32class_grad_on_the_fixture_at_16():
    """tests/test_gpu_exact_grad.py::test_f32class_grad_on_the_fixture, at L = 16."""
    ls = G.LOG_STDS[1]
    up = _updater(L, ls, "bf16", max_b=5000, precision="f32")
    worst = 0.0
    for j, B in enumerate((2, 3, 100, 5000)):
        clip = G.CLIPS[j % 2]
        pi, vf = G.nets(L, 1)
        b = G.make_batch(L, B, 9 + j, pi, vf, ls)
        want, bound = G.restate_f32class(b, pi, vf, clip)
        g = up.grad(*_dev(b), clip=clip, vf_coef=G.VF_COEF, ent_coef=G.ENT_COEF)
        worst = max(worst, _compare(g, want, bound, (L, B, clip)))
    print("L 16 f32class: largest error / bound %.3g" % worst)
    up.close()


def test_minibatch_step_matches_restated_gradient_through_adam_at_16():
    """tests/test_gpu_exact_grad.py::test_minibatch_step_matches_restated_gradient_through_adam, at L = 16 and the reference's
    batch_size 5000."""
    from test_gpu_adam_apply import adam64, check_step

    B, clip, lr = 5000, 0.2, 3e-4
    ls = G.LOG_STDS[1]
    pi, vf = G.nets(L, 1)
    b = G.make_batch(L, B, 5, pi, vf, ls)
    want, bound = G.restate(b, pi, vf, clip, partial="bf16")
    up = _updater(L, ls, "bf16", max_b=5056)
    args = _dev(b)
    g = up.grad(*args, clip=clip, vf_coef=G.VF_COEF, ent_coef=G.ENT_COEF)
    print("grad: largest error / bound %.3g" % _compare(g, want, bound, "grad"))
    gref = _grad_with_kernel_log_std(want, g)
    theta0, m0, v0 = up.theta.clone(), up.m.clone(), up.v.clone()
    up.control(None, clear=True)
    up.stats.zero_()
    up.minibatch(*args, lr=lr, clip=clip, vf_coef=G.VF_COEF, ent_coef=G.ENT_COEF, max_grad_norm=0.5)
    assert up.status()[:3] == (False, 1, 0)
    ref = adam64(theta0, m0, v0, gref, 1, lr, up.betas, up.eps, 0.5)
    assert ref["clip"] < 1.0                                     # the global-norm clip is active
    print("minibatch: error / bound (m, v, theta)", check_step(up, ref, "minibatch"))
    st = up.stats.cpu().numpy()
    assert st[1] == want[-3] and st[3] == want[-1]
    assert abs(st[0] - want[-4]) <= bound[-4] and abs(st[2] - want[-2]) <= bound[-2]
    up.close()


def test_ppo_forward_and_scatter_repack_are_bit_exact_at_16():
    """tests/test_gpu_exact_forward.py::test_ppo_forward_and_scatter_repack_are_bit_exact, at L = 16: qr_ppo_forward for both heads (the
    value head fills buf_val, last_val and buf_term_val of the predecessor envs' trainer in the f16-operand mode) and the scatter re-pack
    after qr_ppo_apply / qr_ppo_minibatch."""
    from test_gpu_exact_forward import test_ppo_forward_and_scatter_repack_are_bit_exact

    test_ppo_forward_and_scatter_repack_are_bit_exact(L)


def test_apply_matches_float64_adam_and_clip_at_16():
    """tests/test_gpu_adam_apply.py::test_apply_matches_float64_adam_and_clip, at L = 16 (the parameter count, and with it the tail of
    ppo_apply_kernel, depends on L)."""
    from test_gpu_adam_apply import test_apply_matches_float64_adam_and_clip

    test_apply_matches_float64_adam_and_clip(L)


def test_minibatch_step_matches_float64_adam_on_its_own_gradient_at_16():
    """tests/test_gpu_adam_apply.py::test_minibatch_step_matches_float64_adam_on_its_own_gradient, at L = 16."""
    from test_gpu_adam_apply import test_minibatch_step_matches_float64_adam_on_its_own_gradient

    test_minibatch_step_matches_float64_adam_on_its_own_gradient(L)
