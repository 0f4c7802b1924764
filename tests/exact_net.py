"""Exact-arithmetic fixture for the f16-operand network kernels (qr_policy_forward, qr_ppo_forward, the closed-loop policy).

`make_net(L, seed)` builds the four layers of a policy / value network ([120, L] -> 120 -> 120 -> O) and `make_obs(n, L, seed)` an
observation batch, both on a dyadic grid chosen so that the kernel's result is fully determined:

  * every value the kernels round to an f16 operand (observations, weights, biases) is f16-exact and not an f16 subnormal;
  * every product and every partial sum of every layer is a multiple of that layer's grid 2^-GRID[k] with sum |terms| < 2^24 2^-GRID[k],
    so it is exactly representable in float32 WHATEVER the summation order (checked by `exactness_margin`);
  * hidden pre-activations are multiples of 2^-11 (layer 1: 2^-6, layer 3: 2^-14) -- never an f16 subnormal after rounding -- and
    layers 2 and 3 DO round: many of their pre-activations need more than the 11 significant bits of f16, so the rounding mode matters.

`forward64` restates in float64 what the f16-operand kernels compute (quadrace_policy.hpp): observations -> f16 round-to-nearest-even,
saturated to +-65504, NaN -> 0 (sat_pack); weights and biases -> f16 RNE; exact accumulation; hidden layers -> f16 RNE, ReLU, saturation
at 65504 (relu_pack / relu_pack2); the output layer stays in float32.  With the fixture its float64 result equals the kernel's float32
result bit for bit, so the GPU tests compare with torch.equal.  The `rounding`, `drop_bias` and `obs_len_shift` arguments model kernel
bugs for the fixture's own "teeth" tests (tests/test_exact_net.py).
"""
import numpy as np

H = 120
OBS_LENS = (13, 17, 20, 21, 24, 25, 28, 29, 32, 36)   # 13 + 4 g (INDI) and 20 + 4 g (E2E), gates_ahead g = 0..4
F16_MAX = 65504.0
F16_MIN_NORMAL = 2.0 ** -14

# per layer: largest |weight integer|, weight exponent, bias integer range, bias exponent (weight = int 2^-WEXP, bias = int 2^-BEXP;
# integers are drawn from +-[1, max]: every weight and bias position is non-zero in every network)
_SPEC = ((3, 4, 64, 6), (7, 5, 512, 10), (3, 3, 1024, 10), (3, 5, 1024, 11))
OBS_EXP = 2            # observations: integers in [-8, 8] times 2^-2
GRID = (6, 11, 14, 19)  # exponent of each layer's product grid: OBS_EXP + WEXP[0], then GRID[k-1] + WEXP[k]


def make_net(L, seed, out=4):
    """[(W1[120, L], b1), (W2[120, 120], b2), (W3, b3), (W4[out, 120], b4)] as float32 arrays (torch Linear layout)."""
    rng = np.random.default_rng([int(L), int(seed), int(out)])
    layers = []
    for k, (wmax, wexp, bmax, bexp) in enumerate(_SPEC):
        fan_in = L if k == 0 else H
        rows = out if k == 3 else H
        w = rng.integers(1, wmax + 1, size=(rows, fan_in)) * rng.choice([-1, 1], size=(rows, fan_in))
        b = rng.integers(1, bmax + 1, size=rows) * rng.choice([-1, 1], size=rows)
        layers.append((np.ldexp(w, -wexp).astype(np.float32), np.ldexp(b, -bexp).astype(np.float32)))
    return layers


def make_obs(n, L, seed):
    rng = np.random.default_rng([int(n), int(L), int(seed), 7])
    return np.ldexp(rng.integers(-8, 9, size=(n, L)), -OBS_EXP).astype(np.float32)


def to_f16(x, rounding="rne"):
    """float64 -> the float64 value of its f16 rounding (RNE like v_cvt_f16_f32 / numpy; 'rtz' = toward zero, a teeth model)."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        h = x.astype(np.float16)
        if rounding == "rtz":
            away = np.isfinite(x) & (np.abs(h.astype(np.float64)) > np.abs(x))
            h = np.where(away, np.nextafter(h, np.float16(0)), h)
        elif rounding != "rne":
            raise ValueError(rounding)
    return h.astype(np.float64)


def sat_pack(x, rounding="rne"):
    """sat_pack (quadrace_policy.hpp): f16 rounding, saturation to +-65504, NaN -> 0."""
    h = to_f16(x, rounding)
    h = np.where(np.isnan(h), 0.0, h)
    return np.clip(h, -F16_MAX, F16_MAX)


def relu_pack(x, rounding="rne"):
    """relu_pack / relu_pack2: f16 rounding, max with 0 (NaN -> 0), min with 65504."""
    h = to_f16(x, rounding)
    h = np.where(np.isnan(h), 0.0, h)
    return np.minimum(np.maximum(h, 0.0), F16_MAX)


def layer_terms(layers, obs, k, rounding="rne", drop_bias=False, obs_len_shift=0):
    """(operand x [n, K], f16 weight matrix W [rows, K] with the bias column last) of layer k -- what the matrix core multiplies."""
    x = sat_pack(np.asarray(obs, np.float64), rounding)
    for j in range(k + 1):
        w, b = layers[j]
        w16 = to_f16(np.asarray(w, np.float64), rounding)
        b16 = np.zeros(len(b)) if (drop_bias and j == 0) else to_f16(np.asarray(b, np.float64), rounding)
        if j == 0 and obs_len_shift:
            # a kernel instantiated for L - 1 on this image: input L - 1 is its constant-1 column, the real bias column is never read
            assert obs_len_shift == -1
            x = x.copy()
            x[:, -1] = 1.0
            b16 = np.zeros(len(b))
        xa = np.concatenate([x, np.ones((x.shape[0], 1))], axis=1)
        wa = np.concatenate([w16, b16[:, None]], axis=1)
        if j == k:
            return xa, wa
        x = relu_pack(xa @ wa.T, rounding)   # exact in float64 (and in float32) for the fixture


def forward64(layers, obs, rounding="rne", drop_bias=False, obs_len_shift=0):
    """float64 restatement of the f16-operand forward: [n, out]."""
    xa, wa = layer_terms(layers, obs, 3, rounding, drop_bias, obs_len_shift)
    return xa @ wa.T


def forward32_in_order(layers, obs, rng):
    """The same network with FLOAT32 accumulation of the terms of every dot product in a random order (one order per layer): what a
    kernel with some other summation order computes.  Equal to forward64 bit for bit iff every partial sum is exact."""
    x = sat_pack(np.asarray(obs, np.float64))
    for k, (w, b) in enumerate(layers):
        xa = np.concatenate([x, np.ones((x.shape[0], 1))], axis=1).astype(np.float32)
        wa = np.concatenate([to_f16(w), to_f16(b)[:, None]], axis=1).astype(np.float32)
        acc = np.zeros((xa.shape[0], wa.shape[0]), np.float32)
        for c in rng.permutation(xa.shape[1]):
            acc += xa[:, c:c + 1] * wa[None, :, c]      # f16 x f16 products are exact in float32
        x = relu_pack(acc.astype(np.float64)) if k < 3 else acc.astype(np.float64)
    return x


def exactness_margin(layers, obs):
    """Per layer: (max over outputs of sum |terms| / (2^24 grid), whether every term is a multiple of the layer's grid).  A margin below
    1 with all terms on the grid makes every partial sum in every order exactly representable in float32."""
    out = []
    for k in range(4):
        xa, wa = layer_terms(layers, obs, k)
        grid = 2.0 ** -GRID[k]
        prod_scale = np.abs(xa) @ np.abs(wa).T
        # every term is a multiple of the grid: inputs of 2^-(GRID[k] - WEXP[k]) times weights of 2^-WEXP[k]; biases times 1
        qx, qw, qb = xa[:, :-1] * 2.0 ** (GRID[k] - _SPEC[k][1]), wa[:, :-1] * 2.0 ** _SPEC[k][1], wa[:, -1] / grid
        on_grid = all(bool(np.all(q == np.round(q))) for q in (qx, qw, qb))
        out.append((float(prod_scale.max() / (2.0 ** 24 * grid)), on_grid))
    return out


def to_actor_critic(L, seed, log_std=(-0.3, 0.1, -0.5, 0.2)):
    """An ActorCritic(L, 4) holding make_net(L, seed) as the policy and make_net(L, seed + 1, out=1) as the value net."""
    import torch

    from optimal_quad_control_rl_amd.ppo import ActorCritic

    ac = ActorCritic(L, 4)
    with torch.no_grad():
        for net, layers in ((ac.pi, make_net(L, seed)), (ac.vf, make_net(L, seed + 1, out=1))):
            lins = [m for m in net if isinstance(m, torch.nn.Linear)]
            for lin, (w, b) in zip(lins, layers):
                lin.weight.copy_(torch.from_numpy(w))
                lin.bias.copy_(torch.from_numpy(b))
        ac.log_std.copy_(torch.tensor(log_std))
    return ac
