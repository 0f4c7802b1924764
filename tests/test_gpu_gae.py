"""GPU: qr_ppo_gae (MfmaPpoUpdater.gae, csrc/quadrace_ppo.hip ppo_gae_kernel) against the float64 restatement of
tests/gae_spec.py, element by element within the restatement's own float32 bound (C = 8 roundings per recursion step), at the
shapes where a one-lane-per-env kernel with (N + 255) / 256 blocks goes wrong: N below a wave, N one past a block, T = 1, an
episode ending on the first or the last row, gamma = 1, lam 0 and 1.  Outputs are views into a larger sentinel-filled
allocation, so a store outside [T][N] shows.  Every case makes two calls on the same episode state and `fin`, so state carried
across calls and `fin` accumulated (not overwritten) are covered; the `none` pattern is the call in which no episode finishes."""
import numpy as np
import pytest
import torch

import gae_spec as G

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
PAD = 300            # floats of sentinel on either side of the [T][N] views: more than one 256-lane block


@pytest.fixture(scope="module")
def updater():
    from optimal_quad_control_rl_amd.ppo import ActorCritic, MfmaPpoUpdater

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    return MfmaPpoUpdater(ActorCritic(17, 4).to(dev), 17, dev, max_minibatch=256)


def _cases(T, N):
    full = T * N <= 48 * 4096
    for pattern in G.DONE_PATTERNS:
        for with_term in (False, True):
            for gamma in G.GAMMAS:
                for lam in G.LAMS:
                    # the full training size visits every pattern at the training (gamma, lam) and every (gamma, lam) at the
                    # random pattern with the bootstrap; the smaller shapes take the whole product
                    if full or (gamma, lam) == (0.99, 0.95) or (pattern == "random" and with_term):
                        yield pattern, with_term, gamma, lam


@pytest.mark.parametrize("T,N", G.SHAPES)
def test_gae_within_the_float32_bound_of_the_float64_restatement(updater, T, N):
    dev = torch.device("cuda", 0)
    dv = lambda a: None if a is None else torch.as_tensor(a).to(dev).contiguous()
    worst = {"adv": 0.0, "ret": 0.0, "ep_ret": 0.0, "fin0": 0.0}
    inputs = {}
    for pattern, with_term, gamma, lam in _cases(T, N):
        key = (pattern, with_term)
        if key not in inputs:
            host = G.make_inputs(T, N, pattern, with_term, seed=0)
            inputs = {key: (host, tuple(dv(a) for a in host))}
        (rew, done, val, last_val, tv), (d_rew, d_done, d_val, d_last, d_tv) = inputs[key]
        adv_ref, ret_ref, bound = G.gae(rew, done, val, last_val, tv, gamma, lam)
        b_ret = G.bound_ret(bound, val)
        slab = torch.full((2, PAD + T * N + PAD), SENTINEL, device=dev)
        out = tuple(slab[j, PAD:PAD + T * N].view(T, N) for j in range(2))
        er, el, eg = (torch.zeros(N, device=dev) for _ in range(3))
        fin = torch.zeros(4, device=dev)
        state, aux = (np.zeros(N), np.zeros(N), np.zeros(N)), (None, None)
        fin_ref, fin_terms, fin_abs = np.zeros(4), 0.0, 0.0
        for call in range(2):
            fin_before = fin.clone()
            slab[:, PAD:PAD + T * N] = SENTINEL
            updater.gae(d_rew, d_done, d_val, d_last, gamma, lam, (er, el, eg), fin, term_val=d_tv, out=out)
            torch.cuda.synchronize()
            tag = (T, N, pattern, with_term, gamma, lam, call)
            # nothing outside [T][N] changed
            assert bool((slab[:, :PAD] == SENTINEL).all()) and bool((slab[:, PAD + T * N:] == SENTINEL).all()), tag
            adv, ret = out[0].cpu().numpy().astype(np.float64), out[1].cpu().numpy().astype(np.float64)
            e_adv, e_ret = np.abs(adv - adv_ref) / bound, np.abs(ret - ret_ref) / b_ret
            worst["adv"], worst["ret"] = max(worst["adv"], e_adv.max()), max(worst["ret"], e_ret.max())
            assert e_adv.max() <= 1.0, (tag, "adv", float(e_adv.max()), np.unravel_index(e_adv.argmax(), e_adv.shape))
            assert e_ret.max() <= 1.0, (tag, "ret", float(e_ret.max()), np.unravel_index(e_ret.argmax(), e_ret.shape))
            # episode statistics: raw rewards, state carried across the two calls, fin accumulated
            state, f, (b_er, _, n_f, a_f), aux = G.episode_stats(rew, done, *state, *aux)
            fin_ref += f; fin_terms += n_f; fin_abs += a_f
            assert fin_ref[1] < 2 ** 24                                       # integers stay exact in float32
            assert np.array_equal(el.cpu().numpy(), state[1]) and np.array_equal(eg.cpu().numpy(), state[2]), tag
            d_er = np.abs(er.cpu().numpy().astype(np.float64) - state[0])
            assert (d_er <= b_er).all(), (tag, "ep_ret", float((d_er - b_er).max()))
            got = fin.cpu().numpy().astype(np.float64)
            assert np.array_equal(got[1:], fin_ref[1:]), (tag, got, fin_ref)
            b_fin = G.U32 * fin_terms * fin_abs
            assert abs(got[0] - fin_ref[0]) <= b_fin, (tag, "fin0", got[0], fin_ref[0], b_fin)
            if b_er.max() > 0:
                worst["ep_ret"] = max(worst["ep_ret"], float((d_er[b_er > 0] / b_er[b_er > 0]).max()))
            if b_fin > 0:
                worst["fin0"] = max(worst["fin0"], abs(got[0] - fin_ref[0]) / b_fin)
            if not done.any():
                assert torch.equal(fin, fin_before), tag                      # no episode finished: fin untouched, bit for bit
    print(f"gae T={T} N={N}: worst error / bound  " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_gae_without_episode_state_leaves_fin_alone(updater):
    """ep_state absent: advantages as before, and a `fin` handed in alone receives nothing."""
    dev = torch.device("cuda", 0)
    T, N = 7, 63
    rew, done, val, last_val, tv = G.make_inputs(T, N, "random", True, seed=1)
    fin = torch.full((4,), 3.0, device=dev)
    adv, ret = updater.gae(*(torch.as_tensor(a).to(dev) for a in (rew, done, val, last_val)), 0.99, 0.95, None, fin,
                           term_val=torch.as_tensor(tv).to(dev))
    adv_ref, ret_ref, bound = G.gae(rew, done, val, last_val, tv, 0.99, 0.95)
    assert (np.abs(adv.cpu().numpy() - adv_ref) <= bound).all()
    assert (np.abs(ret.cpu().numpy() - ret_ref) <= G.bound_ret(bound, val)).all()
    assert fin.tolist() == [3.0] * 4
