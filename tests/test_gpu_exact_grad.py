"""GPU: the PPO gradient kernels element by element against the float64 restatement of tests/exact_grad.py.

qr_ppo_grad (ppo_grad_kernel + the apply kernel's reduction): on the fixture every delta and every per-workgroup weight-gradient sum is
exact in float32 in any order and every output delta is known after its f16 rounding, so the weight and bias entries are compared with
torch.equal -- every L, both partial formats, clip 0.2 and 50, B from 64 to 65 536.  The log-std entries and the surrogate / KL statistics
carry the kernel's float32 __expf and sums: they are compared within the per-element bound the restatement derives; the squared value
error and the clipped count are exact.  qr_ppo_minibatch and qr_ppo_epoch (device shuffle) feed that gradient through Adam
(tests/test_gpu_adam_apply.py: adam64 and its bounds).  qr_ppo_grad_f32class: value net bit for bit, policy net within its propagated
bound.  Each test prints the largest observed error / bound ratio of its bounded entries."""
import numpy as np
import pytest
import torch

import exact_grad as G
import exact_net as E

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SMALL_B = (64, 100, 4096, 5000)
LARGE_B = (16448, 32768, 65536)      # 129 pairs (two passes on workgroup 0); 256 pairs; 512 pairs and 2048 waves per net


def _updater(L, ls, partial, max_b=65536, precision="f16-operands"):
    from optimal_quad_control_rl_amd.ppo import MfmaPpoUpdater

    return MfmaPpoUpdater(G.actor_critic(L, 1, ls).to(DEV), L, DEV, max_minibatch=max_b, flags=1 if partial == "f32" else 0,
                          precision=precision)


def _dev(b):
    return [torch.from_numpy(np.ascontiguousarray(b[k])).to(DEV) for k in ("obs", "act", "old_logp", "adv", "ret", "idx")]


def _compare(got, want, bound, label):
    """torch.equal on the exact entries, |got - want| <= bound on the others; returns the largest error / bound ratio."""
    got = got.cpu().numpy()
    exact = bound == 0
    bad = np.nonzero(got[exact] != want[exact])[0]
    assert bad.size == 0, (label, "exact entries differ", bad.size, int(np.nonzero(exact)[0][bad[0]]),
                           float(got[exact][bad[0]]), float(want[exact][bad[0]]))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))[~exact]
    ratio = float((err / bound[~exact]).max())
    assert ratio <= 1.0, (label, "bounded entries", ratio, np.nonzero(~exact)[0][np.argmax(err / bound[~exact])])
    return ratio


@pytest.mark.parametrize("L", E.OBS_LENS)
def test_grad_is_bit_exact(L):
    """qr_ppo_grad at B = 64 .. 65 536, both partial formats (bf16 / f32), clip 0.2 and 50 (the large sizes at one clip per L,
    alternating over L), both log-std settings (alternating over B)."""
    k = E.OBS_LENS.index(L)
    ups = {}
    worst = 0.0
    cases = [(B, clip) for B in SMALL_B for clip in G.CLIPS] + [(B, G.CLIPS[(k + j) % 2]) for j, B in enumerate(LARGE_B)]
    for j, (B, clip) in enumerate(cases):
        ls = G.LOG_STDS[(j // 2 + k) % 2]
        pi, vf = G.nets(L, 1)
        b = G.make_batch(L, B, 7 + j, pi, vf, ls)
        out = G.restate(b, pi, vf, clip, partial=("bf16", "f32"))
        args = _dev(b)
        for fmt in ("bf16", "f32"):
            if (fmt, ls) not in ups:
                ups[(fmt, ls)] = _updater(L, ls, fmt)
            up = ups[(fmt, ls)]
            up.stats.zero_()
            g = up.grad(*args, clip=clip, vf_coef=G.VF_COEF, ent_coef=G.ENT_COEF, stats=True)
            worst = max(worst, _compare(g, *out[fmt], (L, B, clip, fmt)))
            assert torch.equal(up.stats.cpu(), g[-4:].cpu())
    print("L %d: largest error / bound of the log-std and statistics entries %.3g" % (L, worst))
    for up in ups.values():
        up.close()


def _grad_with_kernel_log_std(want, g):
    """The restated gradient with the kernel's own log-std entries (checked against their bound first): adam64's bounds assume an
    exact gradient."""
    n = want.size - 4
    out = torch.from_numpy(want[:n].copy())
    out[n - 4:] = g[n - 4:n].cpu()
    return out


def test_minibatch_step_matches_restated_gradient_through_adam():
    """qr_ppo_minibatch (grad kernel -> apply kernel with clip_grad_norm_ and Adam, one launch pair): (theta, m, v) equal adam64 of the
    restated gradient within tests/test_gpu_adam_apply.py's bounds; the minibatch statistics are those of the restatement."""
    from test_gpu_adam_apply import adam64, check_step

    L, B, clip, lr = 24, 5000, 0.2, 3e-4
    ls = G.LOG_STDS[1]
    pi, vf = G.nets(L, 1)
    b = G.make_batch(L, B, 5, pi, vf, ls)
    want, bound = G.restate(b, pi, vf, clip, partial="bf16")
    up = _updater(L, ls, "bf16", max_b=B)
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


def test_epoch_with_device_shuffle_uses_the_restated_permutation():
    """qr_ppo_epoch with device_shuffle, one minibatch of all rows: the permutation it draws is _shuffle_reference's, and its Adam step
    is adam64 of the gradient restated on exactly that row order (a 5000-row ragged minibatch: 40 workgroups, the last one partial)."""
    from test_gpu_adam_apply import adam64, check_step
    from test_gpu_round3 import _shuffle_reference

    L, B, clip, lr, seed, count = 20, 5000, 0.2, 1e-3, 0x5EED1234ABCD, 3
    ls = G.LOG_STDS[1]
    pi, vf = G.nets(L, 1)
    perm = _shuffle_reference(B, seed, count)
    b = G.make_batch(L, B, 6, pi, vf, ls, extra_rows=0, idx=perm)
    want, bound = G.restate(b, pi, vf, clip, partial="bf16")
    up = _updater(L, ls, "bf16", max_b=B)
    obs, act, old, adv, ret, idx = _dev(b)
    g = up.grad(obs, act, old, adv, ret, idx, clip=clip, vf_coef=G.VF_COEF, ent_coef=G.ENT_COEF)
    _compare(g, want, bound, "grad on perm")
    gref = _grad_with_kernel_log_std(want, g)
    theta0, m0, v0 = up.theta.clone(), up.m.clone(), up.v.clone()
    up.control(None, clear=True)
    up.set_shuffle(seed, count)
    pbuf = torch.zeros(B, dtype=torch.int32, device=DEV)
    up.epoch(obs, act, old, adv, ret, pbuf, B, lr, clip=clip, vf_coef=G.VF_COEF, ent_coef=G.ENT_COEF, max_grad_norm=0.5,
             device_shuffle=True)
    assert torch.equal(pbuf.cpu().long(), torch.from_numpy(perm))
    assert up.shuffle_state() == (seed, count + 1) and up.status()[:3] == (False, 1, 0)
    ref = adam64(theta0, m0, v0, gref, 1, lr, up.betas, up.eps, 0.5)
    print("epoch: error / bound (m, v, theta)", check_step(up, ref, "epoch"))
    up.close()


@pytest.mark.parametrize("L", E.OBS_LENS)
def test_f32class_grad_on_the_fixture(L):
    """qr_ppo_grad_f32class: value-net entries and the exact statistics bit for bit, policy entries, log-std and the other statistics
    within the restatement's propagated bound, at B = 2, 3, 100 and 5000 (clip alternating)."""
    k = E.OBS_LENS.index(L)
    ls = G.LOG_STDS[k % 2]
    up = _updater(L, ls, "bf16", max_b=5000, precision="f32")
    worst = 0.0
    for j, B in enumerate((2, 3, 100, 5000)):
        clip = G.CLIPS[(j + k) % 2]
        pi, vf = G.nets(L, 1)
        b = G.make_batch(L, B, 9 + j, pi, vf, ls)
        want, bound = G.restate_f32class(b, pi, vf, clip)
        g = up.grad(*_dev(b), clip=clip, vf_coef=G.VF_COEF, ent_coef=G.ENT_COEF)
        worst = max(worst, _compare(g, want, bound, (L, B, clip)))
    print("L %d f32class: largest error / bound %.3g" % (L, worst))
    up.close()
