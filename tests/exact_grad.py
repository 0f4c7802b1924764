"""Exact-arithmetic fixture for the PPO GRADIENT kernels (ppo_grad_kernel + ppo_apply_kernel behind qr_ppo_grad, and the f32-class path).

`make_grad_net(L, seed, out)` builds sparse small-integer networks ([120, L] -> 120 -> 120 -> O): every weight is 0 or +-1 (one or two
non-zeros per row, every input column used (by a +1 in the hidden layers), every hidden unit feeding exactly one output), biases are multiples of 1/4.  With observations
on the 1/4 grid (tests/exact_net.py) every activation is a multiple of 1/4 below ~2^6, and `make_batch` builds loss rows whose output deltas
are coarse dyadic values: the deltas of every layer then span few significant bits too, so that

  * every forward activation, every delta and every partial sum of every weight gradient over the rows of ONE workgroup is exact in
    float32 in ANY summation order (`grad_exactness_margin` < 1: sum |terms| < 2^24 grid steps) -- the MFMA order does not matter;
  * the loss-layer deltas are known exactly after their f16 rounding (sat_pack of dout).  Value net: ret = v - e, so dout = vf_coef 2 e.
    Policy net: z = act - mean is dyadic and old_logp is chosen so that A ratio lands on a coarse dyadic c (ratio = c / A, A = the
    kernel's float32 normalised advantage, replicated bit for bit here): dout = -c z / std^2.  The kernel's float32 A, __expf and
    log-ratio move dout by ~1e-6 relative; `loss_row_margins` derives that error per row from the operation count and asserts it stays
    far inside the distance to the nearest f16 rounding boundary (>= 2^-12 relative), and equally far from the clip edges.

`restate` reproduces what qr_ppo_grad returns, in the kernel's order: advantage normalisation from float64 sums (unbiased, + 1e-8, cast
to float); the masked backward chain with f16 deltas; per-workgroup sums over the rows the kernel assigns to the workgroup (pair p =
positions [128 p, 128 p + 128) runs on workgroup p mod wgs, wgs = min(pairs, 128)); f32(S f32(1 / B)), then the f32 or bf16-RNE partial;
the apply kernel's fixed-shape float32 tree over the 128 chunk slots (two 64-slot trees, then lower + upper).  The weight and bias entries
are exact.  The log-std entries (float32 wave sums of gl (z^2 - 1) with the kernel's __expf) and the surrogate / KL statistics carry a
per-element bound (`bound`): per row the relative error of gl from the operation count (see _row_eps), then gamma_n sum |terms| for the
n-deep float32 summation (wave shuffle tree 6, per-thread rows, block shuffle tree 6, 4 wave parts, x 1/B, - ent_coef).  The squared
value error sum and the clipped count are exact.

`restate_f32class` does the same for qr_ppo_grad_f32class (no f16 anywhere, split-K partial tiles: k_per_slice rows per slice, four
interleaved float32 chains, then x 1/B).  The value net is exact; the policy net's deltas start from the float32 dout and carry a bound
propagated through |W|^T and the float32 accumulations.

The `bug` argument models kernel bugs for the teeth tests (tests/test_exact_grad.py).

`edge_nets` / `make_edge_batch` (further down) put loss-layer deltas and ReLU masks at the edges of f16; `forward` and `deltas` state
the kernel's rule there (EDGE_BUGS are its mis-models; tests/test_exact_edges.py, tests/test_gpu_operand_edges.py)."""
import numpy as np

import exact_net as E

H = 120
U = 2.0 ** -24
PAIR_ROWS = 128
MAX_WGS = 128                       # qr_ppo::kFusedChunks
LN2 = float(np.float32(np.log(2.0)))
LOG_STDS = ((0.0, 0.0, 0.0, 0.0), (-LN2, LN2, 0.0, -LN2))   # std^2 = 1 everywhere / 4, 1/4, 1, 4
C_NORM = float(np.float32(0.9189385332046727))
CLIPS = (0.2, 50.0)
VF_COEF, ENT_COEF = 0.5, 0.01
BUGS = ("drop_row", "ragged_tail", "swap_k", "wrong_mask", "drop_bias", "biased_var", "scale_bm1", "ent_flip", "rtz", "bf16_trunc")
EDGE_BUGS = ("neg_zero_active", "flush_delta", "no_sat_delta", "saturated_inactive")   # told apart on the edge batches only


def make_grad_net(L, seed, out=4):
    """[(W1[120, L], b1), (W2, b2), (W3, b3), (W4[out, 120], b4)] as float32 arrays (torch Linear layout)."""
    rng = np.random.default_rng([int(L), int(seed), int(out), 101])
    layers = []
    for k in range(4):
        fan_in = L if k == 0 else H
        rows = out if k == 3 else H
        w = np.zeros((rows, fan_in))
        if k < 3:
            r = np.arange(rows)
            # hidden layers: the covering weight is +1 (its input is >= 0: a -1 alone would leave the unit dead for every row)
            w[r, rng.permutation(np.resize(rng.permutation(fan_in), rows))] = rng.choice([-1.0, 1.0], rows) if k == 0 else 1.0
            c2 = rng.integers(0, fan_in, rows)
            extra = (rng.random(rows) < 0.5) & (w[r, c2] == 0)
            w[r[extra], c2[extra]] = rng.choice([-1.0, 1.0], int(extra.sum()))
            b = rng.integers(-4, 3, rows) / 4.0
        else:
            w[rng.integers(0, rows, fan_in), np.arange(fan_in)] = rng.choice([-1.0, 1.0], fan_in)
            b = rng.integers(-8, 9, rows) / 4.0
        layers.append((w.astype(np.float32), b.astype(np.float32)))
    return layers


def forward(layers, x, pre=None):
    """[x|1, h1|1, h2|1, h3|1] (float64: the f16 operands the kernel publishes -- sat_pack of the observations, relu_pack of the hidden
    pre-activations, both the identity on the plain fixture -- with f16-rounded weights) and the output [n, O].  `pre`: a list that
    receives the three hidden pre-activations."""
    acts = []
    x = E.sat_pack(x)
    for k, (w, b) in enumerate(layers):
        xa = np.concatenate([x, np.ones((x.shape[0], 1))], axis=1)
        acts.append(xa)
        x = xa @ E.weights_f16(w, b).T
        if k < 3:
            if pre is not None:
                pre.append(x)
            x = E.relu_pack(x)
    return acts, x


def normalised_advantage(adv_rows, biased=False):
    """The kernel's float32 A (quadrace_ppo.hip, loss section): float64 sums, unbiased variance, + 1e-8, cast to float."""
    a = np.asarray(adv_rows, np.float64)
    B = a.size
    s1, s2 = float(a.sum()), float((a * a).sum())        # exact: advantages on a 1/16 grid
    amean = s1 / B
    avar = max((s2 - B * amean * amean) / (B if biased else (B - 1 if B > 1 else 1)), 0.0)
    rstd = np.float32(1.0 / (np.sqrt(avar) + 1e-8))
    return (np.asarray(adv_rows, np.float32) - np.float32(amean)) * rstd, amean


def _logp(z, ls):
    return (-0.5 * z * z - np.asarray(ls, np.float64) - C_NORM).sum(axis=1)


def _grid(x, q):
    return np.round(np.asarray(x) / q) * q


def make_batch(L, B, seed, pi, vf, log_std, extra_rows=37, idx=None, obs_at=None, e_at=None):
    """Rows [B + extra_rows] and the minibatch idx [B] (a random subset in random order unless given).  Only the rows in idx are
    constructed for exactness; the others hold arbitrary data the kernel must not read."""
    rng = np.random.default_rng([int(L), int(B), int(seed), 202])
    rows = B + extra_rows if idx is None else len(idx) + extra_rows
    idx = rng.permutation(rows)[:B].astype(np.int32) if idx is None else np.asarray(idx, np.int32)
    obs = E.make_obs(rows, L, seed + 1000)
    if obs_at is not None:                      # the edge batches: the observation / value error of minibatch POSITION p
        obs[idx] = obs_at
    x = obs[idx].astype(np.float64)
    mean = forward(pi, x)[1]
    v = forward(vf, x)[1][:, 0]
    ls = np.asarray(log_std, np.float32)
    s = np.exp(-ls.astype(np.float64))
    delta = rng.choice([-1.0, -0.5, 0.5, 1.0], size=(B, 4))
    act = rng.normal(size=(rows, 4)).astype(np.float32)
    act[idx] = (mean + delta).astype(np.float32)
    assert np.array_equal(act[idx].astype(np.float64) - mean, delta)
    # advantages: +-[1, 2] on the 1/16 grid (|A| stays away from 0), plus a few exact zeros
    adv = (rng.integers(16, 33, size=rows) * rng.choice([-1, 1], size=rows) / 16.0).astype(np.float32)
    adv[rng.random(rows) < 0.03] = 0.0
    A, _ = normalised_advantage(adv[idx])
    A64 = A.astype(np.float64)
    # target ratio: 1 (flowing at clip 0.2) for 70 % of the rows, else the non-flowing side (1.5 for A > 0, 0.5 for A < 0); c = A ratio on
    # a 1/4 grid, non-zero, with the sign of A, and the ratio at least 1e-3 away from the clip edges 0.8 / 1.2
    want = np.where(rng.random(B) < 0.7, 1.0, np.where(A64 > 0, 1.5, 0.5))
    c = _grid(A64 * want, 0.25)
    c = np.where((c == 0) | (np.sign(c) != np.sign(A64)), np.sign(A64) * 0.25, c)
    for _ in range(4):
        r = np.where(A64 != 0, c / np.where(A64 != 0, A64, 1.0), 1.0)
        bad = (np.abs(r - 0.8) < 2e-3) | (np.abs(r - 1.2) < 2e-3)
        c = np.where(bad, c + np.sign(A64) * 0.25, c)
    ratio = np.where(A64 != 0, c / np.where(A64 != 0, A64, 1.0), 1.0)
    z = delta * s
    lp = _logp(z, ls)
    old = rng.normal(size=rows).astype(np.float32) - 5.0
    old[idx] = (lp - np.log(ratio)).astype(np.float32)
    e = rng.integers(-8, 9, size=B) / 8.0
    if e_at is not None:
        e = np.asarray(e_at, np.float64)
    ret = rng.normal(size=rows).astype(np.float32)
    ret[idx] = (v - e).astype(np.float32)
    assert np.array_equal(v - ret[idx].astype(np.float64), e)
    return dict(obs=obs, act=act, old_logp=old, adv=adv, ret=ret, idx=idx, B=B, log_std=ls, L=L)


def _row_eps(z, ls, log_ratio):
    """Relative error bound of the kernel's float32 gl = -A ratio (A itself is replicated exactly) and of dout = gl z / std, per row, from
    the operation count (u = 2^-24 per rounding): __expf(x) = exp2 of the rounded x log2(e): (|x| + 2) u; z = delta inv_std: eps_s + u;
    logp = sum_k (-0.5 z^2 - ls - C): each z^2 2 eps_z + u, twelve roundings of partial sums <= u M, M = sum_k (z^2 / 2 + |ls| + C);
    log_ratio - old_logp: u |log_ratio|; ratio: the log-ratio error + (|log_ratio| + 2) u; A ratio: u.  Doubled for safety."""
    ls = np.abs(np.asarray(ls, np.float64))
    eps_s = (ls + 2.0) * U
    eps_z = eps_s + U
    M = (0.5 * z * z + ls + C_NORM).sum(axis=1)
    d_logp = (0.5 * z * z * (2 * eps_z + U)).sum(axis=1) + 12 * U * M + U * np.abs(log_ratio)
    eps_ratio = d_logp + (np.abs(log_ratio) + 2.0) * U
    eps_gl = 2.0 * (eps_ratio + U)
    eps_dout = eps_gl[:, None] + 2.0 * (eps_z + eps_s + 2 * U)
    return eps_gl, eps_ratio, eps_dout, eps_z


def _f16_boundary_distance(v):
    """Relative distance of float64 v to the nearest f16 rounding boundary (inf for 0)."""
    v = np.asarray(v, np.float64)
    h = v.astype(np.float16)
    up = np.nextafter(h, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(h, np.float16(-np.inf)).astype(np.float64)
    h = h.astype(np.float64)
    d = np.minimum(np.abs(v - (h + up) / 2), np.abs(v - (h + dn) / 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(v == 0, np.inf, d / np.abs(v))


def loss_rows(batch, pi, vf, clip, bug=None):
    """Per-row loss quantities of the minibatch (positions 0 .. B-1), float64: the forward activations, dout before f16 rounding,
    gl, z, ratio, A and the error bounds."""
    idx, B, ls = batch["idx"], batch["B"], batch["log_std"]
    x = batch["obs"][idx].astype(np.float64)
    acts_pi, mean = forward(pi, x)
    acts_vf, v = forward(vf, x)
    s = np.exp(-ls.astype(np.float64))
    z = (batch["act"][idx].astype(np.float64) - mean) * s
    lp = _logp(z, ls)
    log_ratio = lp - batch["old_logp"][idx].astype(np.float64)
    ratio = np.exp(log_ratio)
    A = normalised_advantage(batch["adv"][idx], biased=bug == "biased_var")[0].astype(np.float64)
    hi, lo = float(np.float32(1.0) + np.float32(clip)), float(np.float32(1.0) - np.float32(clip))
    flows = np.where(A >= 0, ratio <= hi, ratio >= lo)
    gl = np.where(flows, -A * ratio, 0.0)
    dout_pi = gl[:, None] * z * s
    err = v[:, 0] - batch["ret"][idx].astype(np.float64)
    dout_vf = np.zeros((B, 4))
    dout_vf[:, 0] = np.float32(VF_COEF) * 2.0 * err
    eps_gl, eps_ratio, eps_dout, eps_z = _row_eps(z, ls, log_ratio)
    return dict(acts=(acts_pi, acts_vf), mean=mean, v=v, z=z, s=s, ratio=ratio, log_ratio=log_ratio, A=A, flows=flows, gl=gl,
                dout=(dout_pi, dout_vf), err=err, eps_gl=eps_gl, eps_ratio=eps_ratio, eps_dout=eps_dout, eps_z=eps_z, hi=hi, lo=lo)


def loss_row_margins(batch, pi, vf, clip):
    """(largest eps_dout / f16-boundary distance over the policy deltas, largest ratio error / distance to a clip edge or to the
    clipped-count edge).  Both below 1: the kernel's float32 dout rounds to the same f16 as the float64 value, and every branch (flows,
    clipped) is taken as in float64."""
    q = loss_rows(batch, pi, vf, clip)
    dist = _f16_boundary_distance(q["dout"][0])
    m_dout = float(np.max(np.where(q["dout"][0] != 0, q["eps_dout"] / dist, 0.0)))
    r, er = q["ratio"], q["eps_ratio"] * q["ratio"] + 1e-7
    edges = [np.abs(r - q["hi"]), np.abs(r - q["lo"])]
    m_ratio = float(np.max(er / np.minimum(*edges)))
    return m_dout, m_ratio


def _relu_mask(h):
    return (h[:, :-1] > 0).astype(np.float64)


def _f16(x, bug):
    model = {"flush_delta": "flush_obs", "no_sat_delta": "no_sat"}.get(bug)
    return E.sat_pack(x, "rtz" if bug == "rtz" else "rne", model)


def deltas(acts, layers, dout, bug=None):
    """[d1, d2, d3, d4] (float64) of one net: d4 = sat_pack(dout), d_l = relu'(h_l) * sat_pack(W_(l+1)^T d_(l+1)) -- the kernel's masks
    come from the published f16 activations: a unit is active iff its f16 activation is non-zero and positive.  A saturated unit
    (h = 65504) is active; a pre-activation that is exactly 0, rounds to +0 (in (0, 2^-25]) or to -0 (in [-2^-25, 0)) is inactive."""
    O = layers[3][0].shape[0]
    d = [None, None, None, _f16(dout[:, :O], bug)]
    pre = []
    if bug == "neg_zero_active":
        forward(layers, acts[0][:, :-1], pre)
    for l in (2, 1, 0):
        m = _relu_mask(acts[l + 1 if bug != "wrong_mask" or l != 2 else l])
        if bug == "neg_zero_active":     # v_pk_max_f16(-0, +0) handing back -0: bits 0x8000, non-zero, the unit counts as active
            m = np.maximum(m, ((pre[l] < 0) & (E.to_f16(pre[l]) == 0)).astype(np.float64))
        if bug == "saturated_inactive":
            m = m * (acts[l + 1][:, :-1] < E.F16_MAX)
        with np.errstate(invalid="ignore", over="ignore"):
            d[l] = m * _f16(d[l + 1] @ E.weights_f16(*layers[l + 1])[:, :-1], bug)
    return d


def position_workgroup(B):
    """(workgroup of every minibatch position 0 .. B-1, number of workgroups)."""
    G = (B + 63) // 64
    pairs = (G + 1) // 2
    wgs = min(pairs, MAX_WGS)
    return (np.arange(B) // PAIR_ROWS) % wgs, wgs


def workgroup_sums(d, a, wg, wgs, rows=None, dtype=np.float32):
    """S[w] = sum over the rows of workgroup w of d^T a: [wgs, out, in + 1].  With the fixture every partial sum is exact in float32, so
    float32 BLAS (any order) gives the exact value (checked against float64 by the CPU tests)."""
    order = np.argsort(wg, kind="stable")
    cnt = np.bincount(wg, minlength=wgs)
    n = int(cnt.max())
    slot = np.arange(len(wg)) - np.repeat(np.cumsum(cnt) - cnt, cnt)     # position inside the sorted workgroup run
    dd = np.zeros((wgs, n, d.shape[1]), dtype)
    aa = np.zeros((wgs, n, a.shape[1]), dtype)
    dd[wg[order], slot] = d[order]
    aa[wg[order], slot] = a[order]
    return np.matmul(dd.transpose(0, 2, 1), aa)


def bf16_rne(x):
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32)


def bf16_trunc(x):
    return (np.asarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def chunk_tree(p):
    """ppo_apply_kernel's sum over the 128 chunk slots of [chunks, ...] float32 partials (slots past the count hold 0): two 64-slot
    trees (w = 32 .. 1: s[q] += s[q + w]), then lower + upper."""
    s = np.zeros((MAX_WGS,) + p.shape[1:], np.float32)
    s[:p.shape[0]] = p
    lo, hi = s[:64].copy(), s[64:].copy()
    w = 32
    while w >= 1:
        lo[:w] += lo[w:2 * w]
        hi[:w] += hi[w:2 * w]
        w //= 2
    return lo[0] + hi[0]


def _flat(grads):
    return np.concatenate([g.reshape(-1) for g in grads])


def _gamma(n):
    return n * U / (1 - n * U)


def restate(batch, pi, vf, clip, partial="bf16", bug=None, return_sums=False):
    """(expected [n + 4] float32 vector of qr_ppo_grad, elementwise bound [n + 4]: 0 where the entry is exact).  `partial` = "bf16",
    "f32", or a tuple of both: then {format: (expected, bound)} from one pass."""
    fmts = (partial,) if isinstance(partial, str) else tuple(partial)
    B, L = batch["B"], batch["L"]
    q = loss_rows(batch, pi, vf, clip, bug)
    wg, wgs = position_workgroup(B)
    scale = np.float32(1.0) / np.float32(B - 1 if bug == "scale_bm1" else B)
    grads, sums = {f: [] for f in fmts}, []
    for net, layers in enumerate((pi, vf)):
        acts = [a.copy() for a in q["acts"][net]]
        dout = q["dout"][net].copy()
        keep = np.ones(B, bool)
        if bug == "drop_row":
            keep[B // 3] = False
        dout[~keep] = 0.0
        if bug == "drop_bias":
            for a in acts:
                a[:, -1] = 0.0
        d = deltas(acts, layers, dout, bug)
        wgp, ds, aas = wg, list(d), list(acts)
        if bug == "ragged_tail" and B % 64:
            # positions B .. 64 G - 1 read row B - 1 and (the bug) keep its loss gradients
            G = (B + 63) // 64
            extra = np.arange(B, 64 * G)
            wgp = np.concatenate([wg, (extra // PAIR_ROWS) % wgs])
            ds = [np.concatenate([x, np.repeat(x[-1:], len(extra), 0)]) for x in d]
            aas = [np.concatenate([x, np.repeat(x[-1:], len(extra), 0)]) for x in acts]
        for l in range(4):
            a_l = aas[l]
            if bug == "swap_k" and l == 1:
                # the h operand of samples 0 and 1 swapped in ONE 32 x 32 dW tile (output rows 0..31, input columns 0..31)
                S = workgroup_sums(ds[l], a_l, wgp, wgs)
                a_sw = a_l.copy()
                a_sw[[0, 1], :32] = a_l[[1, 0], :32]
                S_sw = workgroup_sums(ds[l][:, :32], a_sw[:, :32], wgp, wgs)
                S[:, :32, :32] = S_sw
            else:
                S = workgroup_sums(ds[l], a_l, wgp, wgs)
            sums.append(S.astype(np.float64).sum(axis=0) / B)
            O = layers[l][0].shape[0]
            for f in fmts:
                P = S * scale
                if f == "bf16":
                    P = bf16_trunc(P) if bug == "bf16_trunc" else bf16_rne(P)
                g = chunk_tree(P)
                grads[f] += [g[:O, :-1], g[:O, -1]]
    n_rows = (B + 63) // 64 * 2          # chain waves per net
    depth = 6 + -(-n_rows // 256) + 6 + 4
    g_ls, b_ls, stats, b_st = _stat_terms(q, clip, depth, bug)
    b_surr, b_kl = b_st[0], b_st[2]
    out = {}
    for f in fmts:
        want = np.concatenate([_flat(grads[f]), g_ls.astype(np.float32), stats.astype(np.float32)]).astype(np.float32)
        bound = np.zeros(want.size)
        bound[-8:-4] = b_ls
        bound[-4] = b_surr
        bound[-3] = b_st[1]
        bound[-2] = b_kl
        out[f] = (want, bound)
    res = out[partial] if isinstance(partial, str) else out
    return (res, q, sums) if return_sums else res


def _stat_terms(q, clip, depth, bug=None):
    """(log_std gradient [4], its bound, statistics [4], their bound) -- shared by both restatements."""
    B = q["A"].size
    zz = q["z"] ** 2 - 1.0
    terms = q["gl"][:, None] * zz
    ent = -ENT_COEF if bug == "ent_flip" else ENT_COEF
    g_ls = terms.sum(axis=0) / B - np.float32(ent)
    row = np.abs(q["gl"])[:, None] * ((q["eps_gl"][:, None] + 2 * U) * np.abs(zz) + q["z"] ** 2 * (2 * q["eps_z"] + 2 * U))
    mag = (np.abs(terms) + row).sum(axis=0) / B
    b_ls = row.sum(axis=0) / B + _gamma(depth + 2) * mag + U * (np.abs(g_ls) + ENT_COEF)
    A, r = q["A"], q["ratio"]
    cr = np.clip(r, q["lo"], q["hi"])
    surr = -np.minimum(A * r, A * cr)
    b_surr = (np.abs(A) * np.maximum(r, cr) * (q["eps_ratio"] + 2 * U)).sum() + _gamma(depth) * np.abs(surr).sum() * (1 + 1e-3)
    kl = (r - 1.0) - q["log_ratio"]
    d_lr = q["eps_ratio"] - (np.abs(q["log_ratio"]) + 2.0) * U
    b_kl_row = r * q["eps_ratio"] + d_lr + 2 * U * (np.abs(r - 1.0) + np.abs(q["log_ratio"])) + U * np.abs(kl)
    b_kl = 2 * b_kl_row.sum() + _gamma(depth) * (np.abs(kl) + b_kl_row).sum()
    clipped = float((np.abs(r - 1.0) > float(np.float32(clip))).sum())
    sq = q["err"] ** 2
    # exact in float32 on the plain fixture (|e| <= 1 on the 1/8 grid: every square a multiple of 2^-6, the sum far below 2^24 of them);
    # with the edge errors (1e5 down to 2^-26) the squares and their partial sums round: u per square, gamma_depth over the sum
    g = 2.0 ** float(E._low_exp(sq).min())
    b_sq = 0.0 if float(sq.sum()) < 2.0 ** 24 * g else (U + _gamma(depth)) * float(sq.sum()) * (1 + 1e-3)
    stats = np.array([surr.sum(), float(sq.sum()), kl.sum(), clipped])
    return g_ls, b_ls, stats, np.array([b_surr, b_sq, b_kl, 0.0])


def f32class_slices(B, k_slices=64):
    """(k_per_slice, slices) of quadrace_ppo_f32.hip's weight-gradient GEMMs."""
    kps = ((-(-B // k_slices)) + 63) // 64 * 64
    kps = max(kps, 256)
    return kps, -(-B // kps)


def _chains(S):
    """f32_dw_reduce_kernel: four interleaved float32 chains over the slices, the remainder into the first, ((s0 + s1) + (s2 + s3))."""
    s = [np.zeros(S.shape[1:], np.float32) for _ in range(4)]
    z = 0
    while z + 4 <= S.shape[0]:
        for k in range(4):
            s[k] = s[k] + S[z + k]
        z += 4
    while z < S.shape[0]:
        s[0] = s[0] + S[z]
        z += 1
    return (s[0] + s[1]) + (s[2] + s[3])


def restate_f32class(batch, pi, vf, clip):
    """(expected [n + 4] float32 vector of qr_ppo_grad_f32class, elementwise bound).  No f16 rounding anywhere; the value net (deltas
    vf_coef 2 e, exact) is restated bit for bit; the policy net starts from dout = gl z / std with the per-row bound eps_dout |dout| and
    carries it through the backward GEMMs (3-piece bf16 deltas x one-piece weights: every product exact, float32 accumulation of K terms
    <= gamma_K sum |terms|) and the split-K weight-gradient sums (gamma_kps per slice, gamma_(slices/4 + 2) over the chains, u for x 1/B)."""
    B = batch["B"]
    q = loss_rows(batch, pi, vf, clip)
    kps, slices = f32class_slices(B)
    sl = np.arange(B) // kps
    scale = np.float32(1.0) / np.float32(B)
    grads, bounds = [], []
    for net, layers in enumerate((pi, vf)):
        acts = q["acts"][net]
        O = layers[3][0].shape[0]
        d = [None, None, None, q["dout"][net][:, :O]]
        e = [None, None, None, q["eps_dout"][:, :O] * np.abs(d[3]) if net == 0 else np.zeros_like(d[3])]
        for l in (2, 1, 0):
            w = layers[l + 1][0].astype(np.float64)
            m = _relu_mask(acts[l + 1])
            d[l] = m * (d[l + 1] @ w)
            e[l] = m * (e[l + 1] @ np.abs(w) + _gamma(w.shape[0]) * ((np.abs(d[l + 1]) + e[l + 1]) @ np.abs(w))) if net == 0 else None
        for l in range(4):
            if net == 1:
                S = workgroup_sums(d[l], acts[l], sl, slices)            # exact per slice (fixture margin)
                g = _chains(S) * scale
                b = np.zeros(g.shape)
            else:
                g = (d[l].T @ acts[l]) / B
                Sa = workgroup_sums(np.abs(d[l]) + e[l], np.abs(acts[l]), sl, slices, dtype=np.float64)
                b = ((e[l].T @ np.abs(acts[l])) + _gamma(kps) * Sa.sum(axis=0) + _gamma(slices // 4 + 2) * Sa.sum(axis=0)) / B
                b = b + 2 * U * (np.abs(g) + b)
            Ol = layers[l][0].shape[0]
            grads += [g[:Ol, :-1], g[:Ol, -1]]
            bounds += [b[:Ol, :-1], b[:Ol, -1]]
    g_ls, b_ls, stats, b_st = _stat_terms(q, clip, 8 + 2)
    want = np.concatenate([_flat(grads), g_ls, stats]).astype(np.float32)
    bound = np.concatenate([_flat(bounds), b_ls, b_st])
    # float64 values of the policy entries are compared within their bound; the exact (value-net) entries bit for bit
    return want, bound


def grad_exactness_margin(batch, pi, vf, clip):
    """Largest sum |terms| / (2^24 grid) over every delta product (d_l = W^T d_(l+1)), every forward product and every per-workgroup
    weight-gradient sum, with every term on its grid.  Below 1: float32 is exact in any order."""
    B = batch["B"]
    q = loss_rows(batch, pi, vf, clip)
    wg, wgs = position_workgroup(B)
    worst = 0.0

    def grid_of(x):
        """The largest power of two dividing every value of x (1 for all-zero x)."""
        nz = np.abs(x[x != 0])
        if nz.size == 0:
            return 1.0
        m, e = np.frexp(nz)
        mi = (m * 2.0 ** 53).astype(np.int64)
        low = np.log2((mi & -mi).astype(np.float64))
        return 2.0 ** float((e - 53 + low).min())

    for net, layers in enumerate((pi, vf)):
        acts = q["acts"][net]
        d = deltas(acts, layers, q["dout"][net])
        for l in range(4):
            w = np.concatenate([layers[l][0], layers[l][1][:, None]], axis=1).astype(np.float64)
            # forward products of layer l
            gf = grid_of(acts[l]) * grid_of(w)
            worst = max(worst, float((np.abs(acts[l]) @ np.abs(w).T).max() / (2.0 ** 24 * gf)))
            # backward product W_(l+1)^T d_(l+1) (the grid of the sum before f16 rounding)
            if l < 3:
                w1 = layers[l + 1][0].astype(np.float64)
                gb = grid_of(d[l + 1]) * grid_of(w1)
                worst = max(worst, float((np.abs(d[l + 1]) @ np.abs(w1)).max() / (2.0 ** 24 * gb)))
            # per-workgroup weight-gradient sums
            gw = grid_of(d[l]) * grid_of(acts[l])
            S = workgroup_sums(np.abs(d[l]), np.abs(acts[l]), wg, wgs, dtype=np.float64)
            worst = max(worst, float(S.max() / (2.0 ** 24 * gw)))
    return worst


# ---- edge fixtures: loss-layer deltas and ReLU masks at the edges of f16 -------------------------------------------------------------------
#
# edge_nets(L): make_grad_net networks whose first hidden units are probes in the manner of tests/exact_net.py's edge net, driven by
# q = obs[:, L-1] (cycling through EDGE_QS) and q2 = obs[:, L-2] (0 but for four rows: 1, 5/4, 3/2, 2):
#   layer 1   0: Q = q + 4    1: R = relu(q2)    2: N1 = 2^-24 (1 - q)    3: S1 = 65519.996 q2    4: Z1 = q - 1/2
#   layer 2   0, 1: Q, R carried    2: N2 = 2^-24 (5 - Q)    3: S2 = 65519.996 R    4: Z2 = Q - 9/2    5: 2^15 N1 + 1/4    6: 2^-14 S1    7: Z1
#   layer 3   0, 1: carried    5 .. 7: carried    2: 2^15 N2 + 1/4    3: 2^-14 S2    4: Z2
# N: pre-activation exactly 0 (q = 1), in (0, 2^-25] -> +0 (q = 3/4, 1/2), in (-2^-25, 0) -> -0 (q = 5/4), an f16 subnormal (q <= 0); it
# is read with 2^15, so an inactive unit wrongly counted as active passes a delta of 2^15 d.  S: 65504 (q2 = 1) and beyond 65520
# (q2 > 1: f16 inf, saturated): ACTIVE; it is read with 2^-14, so its delta is an f16 subnormal.  (Only four rows saturate: 65504 times
# a generic delta over many rows would leave the 2^24 grid steps of an exact weight-gradient sum.  A pre-activation strictly between
# 65504 and 65520 is left to the forward fixture.)  Z: exactly 0 at q = 1/2.  The probes are the only readers of columns L-2, L-1 and
# of each other, and every probe of layer 3 feeds one output with +-1 (the value head reads Q, R, Z only, so that the all-zero
# observation has an exactly known value: b4 is chosen to make it 0).
# value errors e (dout = vf_coef 2 e = e) on the first minibatch positions, by kind; the other positions hold multiples of the kind's
# step, so that deltas 40 bits apart never meet in one weight-gradient sum:
EDGE_E = {"sat": ((65504.0, -65504.0, 7e4, -1e5), 8.0),                                   # +-65504 and beyond it (saturated)
          "sub": ((2.0 ** -15, -3 * 2.0 ** -22, 2.0 ** -26, -2.0 ** -26, 2.0 ** -25, 3 * 2.0 ** -25), 2.0 ** -17),   # subnormal, vanishing, ties at 0
          "tie": ((E.TIE_DN, E.TIE_UP, -E.TIE_UP, 0.0), 0.125)}
N_PROBES = 8
EDGE_Q2 = (1.0, 1.25, 1.5, 2.0)


def edge_nets(L, seed=1):
    T24, big = E.T24, E.W_BIG
    nets_ = []
    for out, sd in ((4, seed), (1, seed + 1)):
        layers = [(w.copy(), b.copy()) for w, b in make_grad_net(L, sd, out)]
        P = N_PROBES
        (w1, b1), (w2, b2), (w3, b3), (w4, b4) = layers
        w1[:, L - 2:] = 0.0
        w1[:P], b1[:P] = 0.0, 0.0
        for u, (col, w, b) in enumerate(((1, 1.0, 4.0), (2, 1.0, 0.0), (1, -T24, T24), (2, big, 0.0), (1, 1.0, -0.5))):
            w1[u, L - col], b1[u] = w, b
        for wk, bk in ((w2, b2), (w3, b3)):
            wk[:, :P] = 0.0
            wk[:P], bk[:P] = 0.0, 0.0
        for u, (src, w, b) in enumerate(((0, 1.0, 0.0), (1, 1.0, 0.0), (0, -T24, 5 * T24), (1, big, 0.0), (0, 1.0, -4.5), (2, 2.0 ** 15, 0.25),
                                         (3, 2.0 ** -14, 0.0), (4, 1.0, 0.0))):
            w2[u, src], b2[u] = w, b
        for u, (src, w) in enumerate(((0, 1.0), (1, 1.0), (2, 2.0 ** 15), (3, 2.0 ** -14), (4, 1.0), (5, 1.0), (6, 1.0), (7, 1.0))):
            w3[u, src] = w
        b3[2] = 0.25                                  # the readers of N stay active where N is 0
        w4[:, :P] = 0.0
        for u in range(P):
            if out == 4 or u in (0, 1, 4, 7):
                w4[u % out, u] = -1.0 if u & 1 else 1.0
        if out == 1:
            b4[0] = 0.0
            b4[0] = -forward(layers, np.zeros((1, L)))[1][0, 0]
            assert E.to_f16(b4[0]) == b4[0]
        nets_.append(layers)
    return nets_


def make_edge_batch(L, B, seed, pi, vf, log_std, kind):
    """make_batch with q = obs[:, L-1] cycling through tests/exact_net.py's EDGE_QS over the minibatch positions and the value errors
    EDGE_E[kind] on the first positions, whose observation is all zero (value exactly 0: ret = -e is exact in float32 down to 2^-26;
    kind "sat": q = 1 instead, any value on the 1/4 grid does), and q2 on the four positions after them."""
    obs_at = E.make_obs(B, L, seed + 2000)
    obs_at[:, L - 1] = [E.EDGE_QS[p % len(E.EDGE_QS)] for p in range(B)]
    obs_at[:, L - 2] = 0.0
    special, step = EDGE_E[kind]
    n = len(special)
    if kind == "sat":
        obs_at[:n, L - 1] = 1.0     # N = 0 on these rows: a delta of 65504 never multiplies a subnormal activation (the matrix core's window)
    else:
        obs_at[:n] = 0.0
    obs_at[n:n + 4, L - 2] = EDGE_Q2
    e_at = np.random.default_rng([L, B, seed, 505]).integers(-8, 9, size=B) * step
    e_at[:n] = special
    return make_batch(L, B, seed, pi, vf, log_std, obs_at=obs_at, e_at=e_at)


def edge_grad_exactness_margin(batch, pi, vf, clip):
    """grad_exactness_margin with the grid found per output (tests/exact_net.py: dot_margin, which also keeps every term with an f16
    subnormal operand inside the matrix core's window): forward products, delta products and per-workgroup weight-gradient sums."""
    B = batch["B"]
    q = loss_rows(batch, pi, vf, clip)
    wg, wgs = position_workgroup(B)
    worst = 0.0
    for net, layers in enumerate((pi, vf)):
        acts = q["acts"][net]
        d = deltas(acts, layers, q["dout"][net])
        for l in range(4):
            wa = E.weights_f16(*layers[l])
            worst = max(worst, E.dot_margin(acts[l], wa))
            if l < 3:
                worst = max(worst, E.dot_margin(d[l + 1], E.weights_f16(*layers[l + 1])[:, :-1].T))
            for w in range(wgs):
                worst = max(worst, E.dot_margin(d[l][wg == w].T, acts[l][wg == w].T))
    return worst


def actor_critic(L, seed, log_std, nets=None):
    """An ActorCritic(L, 4) holding make_grad_net(L, seed) / make_grad_net(L, seed + 1, out=1) (or `nets`) and the given log_std."""
    import torch

    from optimal_quad_control_rl_amd.ppo import ActorCritic

    ac = ActorCritic(L, 4)
    with torch.no_grad():
        for net, layers in zip((ac.pi, ac.vf), nets or (make_grad_net(L, seed), make_grad_net(L, seed + 1, out=1))):
            lins = [m for m in net if isinstance(m, torch.nn.Linear)]
            for lin, (w, b) in zip(lins, layers):
                lin.weight.copy_(torch.from_numpy(w))
                lin.bias.copy_(torch.from_numpy(b))
        ac.log_std.copy_(torch.tensor(log_std, dtype=torch.float32))
    return ac


def nets(L, seed):
    return make_grad_net(L, seed), make_grad_net(L, seed + 1, out=1)
