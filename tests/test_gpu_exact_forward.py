"""GPU: the f16-operand forward kernels bit for bit against the float64 restatement of tests/exact_net.py, at every observation length the
templates instantiate.  On the fixture's dyadic networks every partial sum is exact in float32 whatever the summation order, so the
kernel's output is fully determined: torch.equal, no tolerance.  A misplaced weight, a lost bias column, another rounding mode or a
wrong K-step count changes the bits (tests/test_exact_net.py::test_teeth shows it does on these very networks)."""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_net as E

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 1000, 65536)


def _want(layers, obs):
    return torch.from_numpy(E.forward64(layers, obs).astype(np.float32))


@pytest.mark.parametrize("L", E.OBS_LENS)
def test_policy_forward_is_bit_exact(L):
    """qr_policy_forward (MfmaPolicy) on n = 1 .. 65 536 rows: one ragged wave, one row either side of a full wave, a ragged grid."""
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    layers = E.make_net(L, 1)
    pol = MfmaPolicy(L).set_weights(layers)
    for n in NS:
        obs = E.make_obs(n, L, 11)
        out = pol.forward(torch.from_numpy(obs).cuda()).cpu()
        want = _want(layers, obs)
        assert torch.equal(out, want), (n, float((out - want).abs().max()))
    pol.close()


def _ppo_forward4(up, net, obs):
    """qr_ppo_forward's whole [n, 4] output (MfmaPpoUpdater.forward returns column 0 for the value net)."""
    from optimal_quad_control_rl_amd import _lib

    out = torch.full((obs.shape[0], 4), float("nan"), device=obs.device)
    _lib.check(up._L.qr_ppo_forward(up._h, int(net), int(obs.shape[0]), C.c_void_p(obs.data_ptr()), C.c_void_p(out.data_ptr()),
                                    up._stream()))
    return out


@pytest.mark.parametrize("L", E.OBS_LENS)
def test_ppo_forward_and_scatter_repack_are_bit_exact(L):
    """qr_ppo_forward with the images of qr_ppo_pack: net 0 (action means) and net 1 (the value in column 0 of the padded 4-row head, whose
    other three columns are exactly 0) equal the restatement bit for bit.  Then one qr_ppo_apply step moves every parameter and re-packs
    the images by scatter (pack_scatter, DenseMap-free natural order): both networks must forward exactly as after a qr_ppo_pack of the
    same theta; and again after a qr_ppo_minibatch step, whose update threads own their parameters in DenseMap order."""
    from optimal_quad_control_rl_amd.ppo import MfmaPpoUpdater

    dev = torch.device("cuda", 0)
    ac = E.to_actor_critic(L, 1).to(dev)
    up = MfmaPpoUpdater(ac, L, dev, max_minibatch=4096)
    pi, vf = E.make_net(L, 1), E.make_net(L, 2, out=1)
    for n in NS:
        obs_np = E.make_obs(n, L, 12)
        obs = torch.from_numpy(obs_np).to(dev)
        assert torch.equal(_ppo_forward4(up, 0, obs).cpu(), _want(pi, obs_np)), n
        v4 = _ppo_forward4(up, 1, obs).cpu()
        assert torch.equal(v4[:, :1], _want(vf, obs_np)), n
        assert torch.equal(v4[:, 1:], torch.zeros(n, 3)), n
    obs = torch.from_numpy(E.make_obs(1000, L, 13)).to(dev)
    m0, v0 = up.forward(0, obs).clone(), up.forward(1, obs).clone()
    theta0 = up.theta.clone()
    g = torch.randn(up.theta.numel() + 4, device=dev, generator=torch.Generator(device=dev).manual_seed(L))
    g[-4:] = 0.0                                   # minibatch statistics: no KL (no early stop is armed anyway)
    up.control(None, clear=True)
    up.apply(g, lr=1e-2, B=1000)                   # Adam's first step: every parameter moves by ~1e-2, far beyond its f16 spacing
    assert up.status()[1] == 1 and bool((up.theta != theta0).all())
    m_scatter, v_scatter = up.forward(0, obs).clone(), up.forward(1, obs).clone()
    assert not torch.equal(m_scatter, m0) and not torch.equal(v_scatter, v0)
    up.pack()
    assert torch.equal(m_scatter, up.forward(0, obs)) and torch.equal(v_scatter, up.forward(1, obs))
    # the same after a qr_ppo_minibatch step: accumulator-order partials, DenseMap's thread -> parameter map, then pack_scatter
    gen = torch.Generator(device=dev).manual_seed(L + 1)
    act, adv, ret = (torch.randn(s, device=dev, generator=gen) for s in ((1000, 4), (1000,), (1000,)))
    old_lp = torch.randn(1000, device=dev, generator=gen) * 0.1 - 5.0
    up.minibatch(obs, act, old_lp, adv, ret, torch.arange(1000, device=dev, dtype=torch.int32), lr=1e-2)
    assert up.status()[1] == 2
    m_scatter, v_scatter = up.forward(0, obs).clone(), up.forward(1, obs).clone()
    up.pack()
    assert torch.equal(m_scatter, up.forward(0, obs)) and torch.equal(v_scatter, up.forward(1, obs))
    up.close()
