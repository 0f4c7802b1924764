"""GPU: the network kernels at the edges of their f16 operands, against the restatements of tests/exact_net.py / tests/exact_grad.py.

Every float32 operand of the f16-operand kernels is converted on the way in: observations and loss-layer deltas by sat_pack, hidden
activations and deltas by relu_pack / relu_pack2 and the backward epilogues, weights by three packers (the host's __float2half in
pack_policy_images, the device cast of ppo_pack_kernel, the scatter re-pack of ppo_apply_kernel).  The edge fixtures put operands
where those conversions can go wrong -- +-65504, 65519.996 (rounds down), 65520 (rounds to inf: saturated), 7e4, 1e30, +-inf, NaN of
both signs with a payload, f16 subnormals and the ties around them, +-0, rounding ties, hidden pre-activations beyond 65504, exactly
0, in (0, 2^-25] (-> +0), in (-2^-25, 0) (-> -0) -- and keep every partial sum exact in float32 in any order
(tests/test_exact_edges.py), so the comparisons are torch.equal.

What the MI355X does, measured by these tests (every kernel agreed with the restatements; no kernel was changed):
  * f16 subnormal operands through v_cvt_pk_f16_f32 and v_mfma_f32_32x32x16_f16 are KEPT, on both sides: observations, weights, biases
    and hidden activations below 2^-14 count with their value, the ties at 2^-25 and 3 2^-25 round to even, 2^-14 - 2^-26 rounds up
    to the smallest normal.  Nothing is flushed, in the forward, the backward or the weight-gradient products.
  * But the matrix core adds the products of one instruction in a window aligned at the largest NOMINAL exponent, and an f16
    subnormal operand counts there with the exponent of the smallest normal: in 65504 x 3 2^-24 + 2^-24 x 1 (one K-step of the head)
    the second product was dropped -- 25 bits below the first one's nominal 2^1, only 18 below its value -- while each product
    alone, and 65504 x 2^-24 - 16376 x 2^-24, came out exact.  "Exact in float32 in any order" is therefore not enough for a
    bit-exact fixture with subnormal operands; exact_net.exactness_margin / dot_margin now also keep 2 x the largest nominal term
    within 2^24 grid steps.
  * v_pk_max_f16(-0, +0) gives +0: a pre-activation in (-2^-25, 0) converts to f16 -0, the published activation has the bits 0x0000
    and the gradient kernel's "bits non-zero" criterion counts the unit as inactive, as relu'(x) = 0 for x <= 0 wants.  A saturated
    unit (65504) and a subnormal activation count as active.
  * The three weight packers (host __float2half, the device cast of ppo_pack_kernel, the scatter re-pack of ppo_apply_kernel) agree
    bit for bit on subnormals, ties and 65519.996 -> 65504; Adam at lr = 0 leaves theta bit-identical.
  * The two-piece (f32-class) forward has an ABSOLUTE operand floor of 2^-25: 1.5 2^-24 is held as 2 2^-24, and 114633 as
    65504 + 49120.  A chain that amplifies such a residue by 2^15 or 65504 is outside its accuracy by construction (measured on the
    N3 probe: 1.95e-3 = 2^-25 x 65520); make_edge_net(f32class=True) keeps those chains away from the head.
  * Largest error / bound ratios of the bounded entries: f32-class forward 0.125 (of 4e-6 x the output scale 513); log-std and
    statistics entries of the gradient 0.109.
"""
import numpy as np
import pytest
import torch

import exact_net as E

pytestmark = pytest.mark.gpu

LENS = E.OBS_LENS + (16,)
DEV = torch.device("cuda", 0)
F32_BOUND = 4e-6          # of the output scale: tests/test_gpu_policy.py::test_f32class_policy_matches_float64_torch


def _want(layers, obs):
    return torch.from_numpy(E.forward64(layers, obs).astype(np.float32))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a.cpu()), _bits(b.cpu()))


@pytest.mark.parametrize("L", LENS)
def test_policy_forward_on_the_edge_rows(L):
    """qr_policy_forward with the host-packed images (pack_policy_images) of the edge net on the 65 edge rows."""
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    layers = E.make_edge_net(L)
    obs, _ = E.make_edge_obs(L)
    pol = MfmaPolicy(L).set_weights(layers)
    out = pol.forward(torch.from_numpy(obs).to(DEV)).cpu()
    want = _want(layers, obs)
    bad = np.nonzero((out != want).any(dim=1).numpy())[0]
    assert torch.equal(out, want), (bad.tolist(), out[bad[:4]].tolist(), want[bad[:4]].tolist())
    pol.close()


@pytest.mark.parametrize("L", LENS)
def test_ppo_forward_and_scatter_repack_on_the_edge_rows(L):
    """qr_ppo_forward on the images of qr_ppo_pack (the device cast of ppo_pack_kernel): net 0 and net 1 (columns 1..3 exactly 0) equal
    the restatement, hence the host-packed policy, bit for bit.  Then the images are overwritten with those of an all-zero theta
    (both nets forward 0) and ONE qr_ppo_apply with lr = 0 and a finite random gradient runs: Adam at lr = 0 leaves theta
    bit-identical, and its scatter re-pack rebuilds the images -- both nets forward exactly as before."""
    from optimal_quad_control_rl_amd import _lib
    from optimal_quad_control_rl_amd.ppo import MfmaPpoUpdater
    from test_gpu_exact_forward import _ppo_forward4

    pi, vf = E.make_edge_net(L), E.make_edge_net(L, out=1)
    obs_np, _ = E.make_edge_obs(L)
    obs = torch.from_numpy(obs_np).to(DEV)
    n = obs.shape[0]
    up = MfmaPpoUpdater(E.to_actor_critic(L, 0, nets=(pi, vf)).to(DEV), L, DEV, max_minibatch=256)

    def check(label):
        m = _ppo_forward4(up, 0, obs).cpu()
        want = _want(pi, obs_np)
        assert torch.equal(m, want), (label, "policy net", np.nonzero((m != want).any(dim=1).numpy())[0].tolist())
        v4 = _ppo_forward4(up, 1, obs).cpu()
        want = _want(vf, obs_np)
        assert torch.equal(v4[:, :1], want), (label, "value net", np.nonzero((v4[:, :1] != want).any(dim=1).numpy())[0].tolist())
        assert torch.equal(v4[:, 1:], torch.zeros(n, 3)), label

    check("qr_ppo_pack")
    theta0 = up.theta.clone()
    _lib.check(up._L.qr_ppo_pack(up._h, up._p(torch.zeros_like(up.theta)), up._stream()))
    assert not _ppo_forward4(up, 0, obs).any() and not _ppo_forward4(up, 1, obs).any()
    g = torch.randn(up.theta.numel() + 4, device=DEV, generator=torch.Generator(device=DEV).manual_seed(L))
    g[-4:] = 0.0
    up.control(None, clear=True)
    up.apply(g, lr=0.0, B=n)
    assert up.status()[1:3] == (1, 0)
    assert _same_bits(up.theta, theta0)
    check("scatter re-pack")
    up.close()


@pytest.mark.parametrize("L", LENS)
def test_f32class_forward_on_the_edge_rows(L):
    """qr_policy_forward_f32class (split_pack: x = X0 + X1, two f16 pieces).  (a) The 65 edge rows with NaN replaced by 0 and +-inf by
    +-131008 give bit-identical outputs to the unreplaced rows (both pieces 0 for NaN, both saturated for inf).  (b) On the finite
    edge rows, rows whose low piece X1 is an f16 subnormal (|x| in [2^-12, 2^-3] in the column with weights +-2^15: a lost X1 would
    miss the bound more than tenfold, tests/test_exact_edges.py) and a 1e5 row: within 4e-6 of the output scale of the float64
    evaluation of the same float32 parameters (observations beyond +-131008, split_pack's range, clipped to it)."""
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    layers = E.make_edge_net(L, f32class=True)
    pol = MfmaPolicy(L).set_weights(layers)
    obs, rows = E.make_edge_obs(L)
    rep = np.nan_to_num(obs, nan=0.0, posinf=E.SPLIT_MAX, neginf=-E.SPLIT_MAX)
    assert (rep != obs).any(axis=1).sum() == 4
    a = pol.forward(torch.from_numpy(obs).to(DEV), precision="f32").cpu()
    b = pol.forward(torch.from_numpy(rep).to(DEV), precision="f32").cpu()
    assert bool(torch.isfinite(a).all()) and _same_bits(a, b)
    x = E.split_obs_rows(L)
    out = pol.forward(torch.from_numpy(x).to(DEV), precision="f32").cpu().numpy().astype(np.float64)
    ref = E.forward_plain64(layers, x)
    scale = max(1.0, float(np.abs(ref).max()))
    err = np.abs(out - ref).max(axis=1)
    print("L %d f32-class: largest error / bound %.3g (scale %.4g)" % (L, err.max() / (F32_BOUND * scale), scale))
    assert err.max() <= F32_BOUND * scale, (int(err.argmax()), float(err.max()), scale)
    pol.close()


# ---- closed-loop kernels: the forward inlined into the rollouts, kernel against kernel ------------------------------------------------
N_ENVS = 256
INJECTED = (float("nan"), float("inf"), float("-inf"), 7e4, 1e-7)
PRECISIONS = ("f16-operands", "f32")


def _random_policy(L):
    from optimal_quad_control_rl_amd.policy import MfmaPolicy
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    torch.manual_seed(100 + L)
    net = ActorCritic(L, 4)
    with torch.no_grad():
        net.pi[-1].weight.mul_(30.0)
    return MfmaPolicy(L).load_torch(net.pi)


def _inject(state, cols, values=INJECTED):
    """state [N, S] (numpy, modified in place): value j in column cols[i] of env 3 + 10 (j len(cols) + i) -- a few envs each, in every
    wave.  Returns [(env, column, value)]."""
    where = []
    for j, v in enumerate(values):
        for i, c in enumerate(cols):
            e = 3 + 10 * (j * len(cols) + i)
            state[e, c] = v
            where.append((e, c, v))
    assert where[-1][0] < state.shape[0]
    return where


def _check_rollout(out, where, pol, precision, label):
    obs0, act0 = out[0][0].contiguous(), out[1][0]
    got = obs0.cpu().numpy()
    for e, c, v in where:
        want = np.float32(v)
        assert (np.isnan(got[e, c]) if np.isnan(want) else got[e, c] == want), (label, e, c, v, float(got[e, c]))
    mean = pol.forward(obs0, precision=precision)
    assert bool(torch.isfinite(mean).all()), label
    assert _same_bits(act0, mean), (label, np.nonzero((act0 != mean).any(dim=1).cpu().numpy())[0].tolist())
    # and a NaN acted as 0, an infinity as the largest finite operand (65504; two pieces: 131008), inside the rollout too
    top = E.F16_MAX if precision == "f16-operands" else E.SPLIT_MAX
    finite = torch.nan_to_num(obs0, nan=0.0, posinf=top, neginf=-top)
    assert not torch.equal(finite, obs0) and _same_bits(act0, pol.forward(finite, precision=precision)), label


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("variant", ("e2e", "indi"))
def test_race_rollouts_forward_injected_observations_like_the_policy_kernel(variant, precision):
    """E2E and INDI, N = 256, K = 1, deterministic: world states with NaN, +-inf, 7e4 and 1e-7 in vz and the three body rates (columns
    that reach the observation unchanged).  The stored observation holds those values, and the stored action equals the policy
    kernel on that stored row -- for qr_rollout_policy, and for qr_rollout_policy_conditions, which stages the images through its
    condition-bank path."""
    from optimal_quad_control_rl_amd.conditions import Condition, ConditionBank
    from test_gpu_action_noise import _env

    env = _env(variant, N_ENVS)
    pol = _random_policy(env.state_len)
    start = [None if t is None else t.clone() for t in env.get_state_tensors()]
    world = start[0].cpu().numpy().copy()
    where = _inject(world, (5, 9, 10, 11))
    bank = ConditionBank(env.VARIANT, 1)
    bank.set(0, Condition.from_env(env))
    for launch in ("rollout_policy", "rollout_policy_conditions"):
        env.set_state_tensors(world, *start[1:])
        if launch == "rollout_policy":
            out = env.rollout_policy_device(pol, 1, (0.0,) * 4, deterministic=True, precision=precision)
        else:
            out = env.rollout_policy_conditions_device(pol, bank, [0], N_ENVS, 1, (0.0,) * 4, deterministic=True, precision=precision)
        _check_rollout(out, where, pol, precision, (variant, launch, precision))
    bank.close()
    pol.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ("hover", "gates"))
def test_predecessor_rollouts_forward_injected_observations_like_the_policy_kernel(kind, precision):
    """Both predecessor envs (the state row is the observation), N = 256, K = 1, deterministic, through their state setters; the hover
    env's float64 state also carries 1e39, which the cast to the float32 observation turns into inf."""
    from test_gpu_q3_rollout_policy import _make

    env = _make(kind, N_ENVS)
    pol = _random_policy(16)
    st, tg, sc = env.get_state_tensors()
    state = st.cpu().numpy().copy()
    wide = state.dtype == np.float64
    where = _inject(state, (3, 5, 9, 11), INJECTED + ((1e39,) if wide else ()))
    env.set_state_tensors(state, tg, sc)
    out = env.rollout_policy_device(pol, 1, (0.0,) * 4, deterministic=True, precision=precision)
    with np.errstate(over="ignore"):
        _check_rollout(out, where, pol, precision, (kind, precision))
    if kind == "hover":
        assert wide and bool(torch.isinf(out[0][0][where[-1][0], where[-1][1]]))
    pol.close()


# ---- the gradient kernel on edge deltas and edge masks ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (64, 100))
@pytest.mark.parametrize("L", (13, 16, 36))
def test_grad_on_edge_deltas_and_edge_masks(L, B):
    """qr_ppo_grad, both partial formats, on tests/exact_grad.py's edge batches: value-net loss deltas of +-65504, beyond it (saturated),
    f16 subnormal, below 2^-25 (vanishing) and on the two ties; hidden units whose pre-activation is 65504, beyond 65520 (saturated,
    active), exactly 0, rounds to +0 or to -0 (inactive) or is an f16 subnormal (active), in two hidden layers of both nets (deltas reach them in the policy net).  Weight
    and bias entries bit for bit; log-std and statistics within the restatement's bounds.  (Policy-net loss deltas stay ordinary: they
    carry the kernel's float32 __expf, and loss_row_margins keeps them away from every f16 rounding boundary by construction -- a
    saturating or subnormal one cannot be placed exactly.  The squared value error, exact on the plain fixture, is a float32 sum of
    float32 squares here: bounded by (u + gamma_depth) sum e^2.)"""
    import exact_grad as G
    from optimal_quad_control_rl_amd.ppo import MfmaPpoUpdater
    from test_gpu_exact_grad import _compare, _dev

    pi, vf = G.edge_nets(L)
    ls = G.LOG_STDS[B == 100]
    ups = {fmt: MfmaPpoUpdater(G.actor_critic(L, 1, ls, nets=(pi, vf)).to(DEV), L, DEV, max_minibatch=128, flags=1 if fmt == "f32" else 0)
           for fmt in ("bf16", "f32")}
    worst = 0.0
    for j, kind in enumerate(G.EDGE_E):
        clip = G.CLIPS[j % 2]
        b = G.make_edge_batch(L, B, 3, pi, vf, ls, kind)
        out = G.restate(b, pi, vf, clip, partial=("bf16", "f32"))
        args = _dev(b)
        for fmt, up in ups.items():
            g = up.grad(*args, clip=clip, vf_coef=G.VF_COEF, ent_coef=G.ENT_COEF)
            worst = max(worst, _compare(g, *out[fmt], (L, B, kind, clip, fmt)))
    print("L %d B %d: largest error / bound of the log-std and statistics entries %.3g" % (L, B, worst))
    for up in ups.values():
        up.close()
