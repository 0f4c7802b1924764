"""GPU: the black box and flight recorder of the sensing-grid evaluator -- qr_blackbox_policy_grid (blackbox_policy_grid_kernel<V, GA, H,
kF32>, csrc/quadrace_blackbox_grid.hip: eval_policy_body with a recording class).  Model: include/quadrace.h; the ring / freeze bookkeeping
is tests/blackbox_spec.py, the command queue tests/command_history_spec.py.

1. Evaluator half: rec, recf, pending and the state equal the evaluator twin's (qr_evaluate_policy_history_grid; H = 0:
   qr_evaluate_policy_sensing_grid) in all 15 (GA, H) forms x 2 variants, triggers 0 and 3.
2. Rows: trigger 0, window = K: column g M + j equals the per-step loop on an E-env twin (state from qr_get_state before each step, the
   command FLOWN, reward, end code, target and steps before the step).
3. Freezing: triggers 1, 2, 3 at window 8 against blackbox_spec applied to the rows of 2.   4. Continuation: 64 = 64 x 1 = 40 + 24.
5. Guards stay SENTINEL; permuting the groups permutes the column blocks.   6. Refusals.   7. blackbox_grid / record_grid.   8. Time, printed.
Every comparison is bit for bit.  Shapes: four groups of E = 256 envs that share one start, K = 64, env_id_base = 2^32 - 300, first_step =
2^32 - 20 (first_step mod 8 = 4), the short condition (max_steps 30) with forced rows (crashes and time limits), group sensors ideal /
(NOISY, d) / noise alone / delay alone, rec_per_group = 100: wave 0 a block, wave 1 lane-masked with 36 lanes, waves 2 and 3 record nothing."""
import ctypes as C
import functools
import statistics
import time

import numpy as np
import pytest
import torch

import blackbox_spec as B
import command_history_spec as CH
import eval_spec as S
from eval_helpers import SENTINEL, _closed_loop_layers, _policy_bank, _ptr, _records
from test_gpu_blackbox import _check_against_spec
from test_gpu_command_history import DELAY
from test_gpu_dynamics_grid import _dynamics_bank
from test_gpu_rollout_conditions import _bank, _force_rows
from test_gpu_rollout_sensing import SEED, _short
from test_gpu_sensing_grid import BASE, NOISY, _based_twin, _bits, _pending, _sensing_bank, _sensor

pytestmark = pytest.mark.gpu

SC = S.SCENARIO
E, G, K, FIRST, W8, M = 256, 4, 64, 2 ** 32 - 20, 8, 100
PAIRS = [(ga, h) for ga in range(5) for h in range(0, 5 - ga)]                       # the 15 (GA, H) with H >= 0, GA + H <= 4
assert len(PAIRS) == 15 and FIRST % W8 == 4
DELAYS = {**DELAY, (0, 0): 2, (1, 0): 4, (2, 0): 1, (3, 0): 3, (4, 0): 2}              # H = 0: some delay; H > 0: the command-history test's table
STD = {"e2e": ("e2e", 1, 2, 3), "indi": ("indi", 2, 0, 2)}                            # the forms of tests 2 - 5: (variant, GA, H, d)


def _sensors(d):
    """group sensors: ideal, (NOISY, d), noise alone, delay alone; and each group's delay"""
    return [None, _sensor(NOISY, d), _sensor(NOISY, 0), _sensor(delay=d or 1)], (0, d, 0, d or 1)


class _Rig:
    """a 4 E-env handle whose groups all start from the state of group 1 (forced rows included), and the banks of one form"""

    def __init__(self, variant, ga, H, d, layers=None):
        self.variant, self.ga, self.H, self.d = variant, ga, H, d
        self.cond = _short(variant)
        self.env = _based_twin(variant, G * E, ga, self.cond.replace(max_steps=97), BASE)     # the condition's max_steps must win
        self.W = self.env.state_len + 4 * H
        self.layers = layers or _closed_loop_layers(self.W, np.asarray(SC[variant + "_action"], np.float32), seed=3)
        self.pbank, self.cbank, self.dbank = _policy_bank(self.W, [self.layers]), _bank(variant, [self.cond]), _dynamics_bank(variant, [None])
        sensors, self.delays = _sensors(d)
        self.sbank = _sensing_bank(sensors)
        _force_rows(self.env, G)
        one = [None if t is None else t[E:2 * E] for t in self.env.get_state_tensors()]
        self.group_start = [None if t is None else t.clone() for t in one]
        self.start = [None if t is None else torch.cat([t] * G).contiguous() for t in one]
        self.S, self.R = self.env.STATE_LEN, self.env.STATE_LEN + 8

    def restart(self, env=None, rows=None):
        env = env or self.env
        env.set_state_tensors(*[None if t is None else (t if rows is None else t[rows].contiguous()) for t in self.start])
        return _pending(env), _records(env)

    def twin_env(self):
        """an E-env handle configured with the condition, keyed as the evaluator keys a group (the env's own base), at the groups' start"""
        twin = _based_twin(self.variant, E, self.ga, self.cond, BASE)
        twin.set_state_tensors(*self.group_start)
        twin.update_states()
        return twin

    def evaluate(self, env, pend, rec, recf, steps=K, first=FIRST, precision="f16-operands", sog=(0, 1, 2, 3)):
        maps = ([0] * G, [0] * G, [0] * G, list(sog))
        if self.H:
            return env.evaluate_history_grid_device(self.pbank, self.cbank, self.dbank, self.sbank, *maps, self.H, E, steps, pend, rec, recf,
                                                    precision=precision, noise_seed=SEED, first_step=first)
        return env.evaluate_sensing_grid_device(self.pbank, self.cbank, self.dbank, self.sbank, *maps, E, steps, pend, rec, recf, precision=precision,
                                                noise_seed=SEED, first_step=first)

    def blackbox(self, env, pend, rec, recf, bufs, m, trigger, window, steps=K, first=FIRST, precision="f16-operands", sog=(0, 1, 2, 3)):
        """bufs: guarded flat buffers (_guarded); returns the three views"""
        ring, st, term = bufs.views(window, G * m, self.R, self.S)
        out = env.blackbox_grid_device(self.pbank, self.cbank, self.dbank, self.sbank, [0] * G, [0] * G, [0] * G, list(sog), self.H, E, steps, pend, rec,
                                       recf, precision=precision, noise_seed=SEED, first_step=first, window=window, trigger=trigger, rec_per_group=m,
                                       ring=ring, status=st, terminal=term)
        assert out[2].data_ptr() == ring.data_ptr() and out[3].data_ptr() == st.data_ptr() and out[4].data_ptr() == term.data_ptr()
        return ring, st, term

    def close(self):
        for x in (self.env, self.pbank, self.cbank, self.dbank, self.sbank):
            x.close()


class _guarded:
    """ring / status / terminal buffers between SENTINEL-filled guards of `guard` elements on both sides (a multiple of 4: 16-byte aligned)"""

    def __init__(self, dev, window, cols, r, s, guard=256):
        self.guard, self.sizes = guard, (window * cols * r, cols * 4, cols * s)
        self.ring = torch.full((self.sizes[0] + 2 * guard,), SENTINEL, dtype=torch.float32, device=dev)
        self.st = torch.full((self.sizes[1] + 2 * guard,), 12345, dtype=torch.int32, device=dev)
        self.st[guard:guard + self.sizes[1]] = 0
        self.term = torch.full((self.sizes[2] + 2 * guard,), SENTINEL, dtype=torch.float32, device=dev)

    def views(self, window, cols, r, s):
        g, (a, b, c) = self.guard, self.sizes
        assert (a, b, c) == (window * cols * r, cols * 4, cols * s)
        return self.ring[g:g + a].view(window, cols, r), self.st[g:g + b].view(cols, 4), self.term[g:g + c].view(cols, s)

    def guards_intact(self):
        g = self.guard
        for name, t, fill in (("ring", self.ring, SENTINEL), ("st", self.st, 12345), ("term", self.term, SENTINEL)):
            assert bool((t[:g] == fill).all()) and bool((t[-g:] == fill).all()), "memory outside %s was written" % name


def _row_loop(twin, pol, noise, d, H, steps, precision):
    """test_gpu_command_history._loop with the recorder's row taken at every step: steps x [qr_get_state -> row(obs + noise[k], queue, H) ->
    forward -> clamp -> push -> step(the command flown) -> clear].  Returns (rows [steps][E][S + 8], the computed commands [steps][E][4])."""
    n, dev, s = twin.num_envs, twin.device, twin.STATE_LEN
    rows = torch.empty((steps, n, s + 8), device=dev)
    computed = torch.empty((steps, n, 4), device=dev)
    queue = torch.zeros((n, 16), dtype=torch.float32, device=dev)
    obs = twin.states_tensor
    for k in range(steps):
        world, _, target, count, _ = twin.get_state_tensors()
        seen = CH.row(obs if noise is None else obs + noise[k], queue, H).contiguous()
        cmd = pol.forward(seen, precision=precision).clamp(-1, 1)
        computed[k].copy_(cmd)
        fly, queue = CH.push(queue, cmd, d, H)
        obs, rew, dd, t = twin.step_device(fly.contiguous())
        queue = CH.clear(queue, dd)
        rows[k, :, :s] = world
        rows[k, :, s:s + 4] = fly
        rows[k, :, s + 4] = rew
        rows[k, :, s + 5] = dd.float() * (1.0 + t.float())
        rows[k, :, s + 6] = target.float()
        rows[k, :, s + 7] = count.float()
    return rows, computed


@functools.lru_cache(maxsize=None)
def _reference(variant, precision="f16-operands"):
    """the four groups of the standard form through the per-step loop, once: rows [K][4 E][R] (host), computed commands [K][4 E][4]"""
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    rig = _Rig(*STD[variant])
    pol = MfmaPolicy(rig.W).set_weights(rig.layers)
    rows, computed = [], []
    for g, dg in enumerate(rig.delays):
        twin = rig.twin_env()
        noise = rig.env.sensing_noise_device(rig.sbank, g, E, K, noise_seed=SEED, first_step=FIRST) if g in (1, 2) else None
        r, c = _row_loop(twin, pol, noise, dg, rig.H, K, precision)
        rows.append(r.cpu().numpy()); computed.append(c.cpu().numpy())
        twin.close()
    pol.close(); rig.close()
    rows, computed = np.concatenate(rows, axis=1), np.concatenate(computed, axis=1)
    # non-vacuity, on the loop's own outputs
    s = rig.S
    code = rows[..., s + 5]
    assert ((code != 0).sum(axis=0) >= 1).all(), "every env ended an episode"
    assert (code == 1).sum() >= 1 and (code == 2).sum() >= 1, "crashes and time limits"
    delayed = slice(E, 2 * E)
    assert (rows[:, delayed, s:s + 4] != computed[:, delayed]).any(), "under a delay some flown command differs from the computed one"
    assert not rows[:rig.delays[1], delayed, s:s + 4].any(), "an episode's first d steps fly zeros"
    return rows, computed


def _columns(m):
    return np.concatenate([np.arange(g * E, g * E + m) for g in range(G)])


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), \
        (what, int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum()))


# ---- 1. the evaluator half ----------------------------------------------------------------------------------------------------------------------
_HALF = [(v, ga, h, "f16-operands") for v in ("e2e", "indi") for ga, h in PAIRS] + \
        [(v, ga, h, "f32") for v in ("e2e", "indi") for ga, h in ((0, 4), (2, 0), (1, 2))]


@pytest.mark.parametrize("variant,ga,H,precision", _HALF, ids=["%s-ga%d-h%d-%s" % c for c in _HALF])
def test_evaluator_half_equals_the_evaluator_twin(variant, ga, H, precision):
    rig = _Rig(variant, ga, H, DELAYS[(ga, H)])
    other = _based_twin(variant, G * E, ga, rig.cond.replace(max_steps=97), BASE)
    pend, (rec, recf) = rig.restart()
    rig.evaluate(rig.env, pend, rec, recf, precision=precision)
    want_state = rig.env.get_state_tensors()
    assert int((rec[:, 1] + rec[:, 2]).sum()) >= G * E and bool((rec[:, 5] == K).all()), "every env ended an episode"
    assert bool(pend.any())
    for trigger, m, window in ((0, M, W8), (3, M, W8), (1, E, 5)):
        p2, (r2, f2) = rig.restart(other)
        bufs = _guarded(other.device, window, G * m, rig.R, rig.S)
        _, st, _ = rig.blackbox(other, p2, r2, f2, bufs, m, trigger, window, precision=precision)
        torch.cuda.synchronize()
        assert torch.equal(r2, rec) and torch.equal(_bits(f2), _bits(recf)) and torch.equal(_bits(p2), _bits(pend)), (trigger, "rec / recf / pending")
        for name, x, y in zip(("world", "disturbances", "target", "steps", "episode"), want_state, other.get_state_tensors()):
            assert x is None or torch.equal(x, y), (trigger, name)
        bufs.guards_intact()
        assert bool((st[:, 1] >= 1).all()) and (trigger == 0) == (not bool(st[:, 0].any()))
    other.close(); rig.close()


# ---- 2. rows ------------------------------------------------------------------------------------------------------------------------------------
_ROWS = [("e2e", "f16-operands", M), ("indi", "f16-operands", M), ("e2e", "f32", M), ("e2e", "f16-operands", E), ("indi", "f16-operands", 98)]


@pytest.mark.parametrize("variant,precision,m", _ROWS, ids=["%s-%s-M%d" % c for c in _ROWS])
def test_rows_equal_the_per_step_loop(variant, precision, m):
    """trigger 0, window = K: the ring is the flight record; M = 100: block + masked lanes; 256: all blocks; INDI 98: M % 4 != 0, R = 21, no block"""
    rows, _ = _reference(variant, precision)
    rig = _Rig(*STD[variant])
    pend, (rec, recf) = rig.restart()
    bufs = _guarded(rig.env.device, K, G * m, rig.R, rig.S)
    ring, st, term = rig.blackbox(rig.env, pend, rec, recf, bufs, m, 0, K, precision=precision)
    cols = rows[:, _columns(m)]
    source, want_st, _ = B.run_arrays(cols, FIRST, K, 0)
    assert (source >= 0).all() and FIRST % K != 0
    got = ring.cpu().numpy()
    s = rig.S
    for name, lo, hi in (("state", 0, s), ("flown command", s, s + 4), ("reward", s + 4, s + 5), ("end code", s + 5, s + 6), ("target", s + 6, s + 7),
                         ("steps", s + 7, s + 8)):
        _same(got[..., lo:hi], B.ring_from_source(cols, source, SENTINEL)[..., lo:hi], name)
    assert np.array_equal(st.cpu().numpy(), want_st) and bool((term == SENTINEL).all()), "never frozen: status counts K rows, no terminal row"
    bufs.guards_intact()
    rig.close()


# ---- 3. freezing --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_freezing_equals_the_spec(variant):
    rows, _ = _reference(variant, "f16-operands")
    cols = rows[:, _columns(M)]
    rig = _Rig(*STD[variant])
    for trigger in (1, 2, 3):
        pend, (rec, recf) = rig.restart()
        bufs = _guarded(rig.env.device, W8, G * M, rig.R, rig.S)
        ring, st, term = (t.cpu().numpy() for t in rig.blackbox(rig.env, pend, rec, recf, bufs, M, trigger, W8))
        _check_against_spec(cols, FIRST, W8, trigger, ring, st, term, "%s trigger %d" % (variant, trigger))
        bufs.guards_intact()
        frozen = st[:, 0] != 0
        print(variant, "trigger", trigger, "frozen", int(frozen.sum()), "armed", int((~frozen).sum()), "causes", np.bincount(st[frozen, 3], minlength=9).tolist())
        assert frozen.sum() >= 1 and (trigger != 1 or (~frozen).sum() >= 1)
        # the trigger row is the row of the step that ended the episode, and under a delay it carries the command flown then
        trig_rows = ring[st[frozen, 2], np.nonzero(frozen)[0]]
        assert ((trig_rows[:, rig.S + 5].astype(np.int64) & trigger) != 0).all()
    rig.close()


# ---- 4. continuation ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_one_call_equals_many(variant):
    rig = _Rig(*STD[variant])
    others = [_based_twin(variant, G * E, rig.ga, rig.cond.replace(max_steps=97), BASE) for _ in range(2)]
    outs = []
    for env, parts in ((rig.env, [K]), (others[0], [1] * K), (others[1], [40, 24])):
        pend, (rec, recf) = rig.restart(env)
        bufs = _guarded(env.device, W8, G * M, rig.R, rig.S)
        done = 0
        for steps in parts:
            ring, st, term = rig.blackbox(env, pend, rec, recf, bufs, M, 1, W8, steps=steps, first=FIRST + done)
            done += steps
        bufs.guards_intact()
        outs.append((ring, st, term, rec, recf, pend, env.get_state_tensors()))
    assert bool(outs[0][1][:, 0].any()) and not bool(outs[0][1][:, 0].all()), "frozen and armed columns"
    for other, what in ((outs[1], "64 x 1"), (outs[2], "40 + 24")):
        for name, x, y in zip(("ring", "status", "terminal", "rec", "recf", "pending"), outs[0][:6], other[:6]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, name)
        for x, y in zip(outs[0][6], other[6]):
            assert x is None or torch.equal(x, y), (what, "state")
    for e in others:
        e.close()
    rig.close()


# ---- 5. bounds ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_permuting_the_groups_permutes_the_column_blocks(variant):
    """the groups share their start, so the sensors alone tell them apart: launch B flies A's sensors in another order"""
    order = [2, 0, 3, 1]
    rig = _Rig(*STD[variant])
    outs = []
    for sog in ((0, 1, 2, 3), tuple(order)):
        pend, (rec, recf) = rig.restart()
        bufs = _guarded(rig.env.device, W8, G * M, rig.R, rig.S)
        ring, st, term = rig.blackbox(rig.env, pend, rec, recf, bufs, M, 3, W8, sog=sog)
        bufs.guards_intact()
        outs.append((ring.clone(), st.clone(), term.clone()))
    cols = torch.cat([torch.arange(order[j] * M, (order[j] + 1) * M) for j in range(G)]).to(rig.env.device)
    (ra, sa, ta), (rb, sb, tb) = outs
    assert torch.equal(_bits(ra[:, cols]), _bits(rb)) and torch.equal(sa[cols], sb) and torch.equal(_bits(ta[cols]), _bits(tb))
    assert not torch.equal(_bits(ra[:, :M]), _bits(ra[:, M:2 * M])), "the sensors matter"
    never = ra == SENTINEL                                                             # slots no armed step reached stay SENTINEL, whole rows
    assert bool((never.all(dim=2) == never.any(dim=2)).all())
    rig.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from optimal_quad_control_rl_amd import _lib

    variant, ga, H, Kr, m = "indi", 1, 2, 8, 10
    rig = _Rig(variant, ga, H, 1)
    env, L = rig.env, rig.env._L
    own = _policy_bank(env.state_len, [_closed_loop_layers(env.state_len, np.asarray(SC["indi_action"], np.float32))])
    n, dev = env.num_envs, env.device
    bufs = dict(pend=torch.full((n, 16), SENTINEL, device=dev), rec=torch.full((n, S.REC_INTS), 7, dtype=torch.int32, device=dev),
                recf=torch.full((n, S.REC_FLOATS), SENTINEL, device=dev), ring=torch.full((W8, G * m, rig.R), SENTINEL, device=dev),
                st=torch.full((G * m, 4), 7, dtype=torch.int32, device=dev), term=torch.full((G * m, rig.S), SENTINEL, device=dev))
    before = env.get_state_tensors()
    i32p = C.POINTER(C.c_int32)
    ip = lambda x: None if x is None else np.asarray(x, np.int32).ctypes.data_as(i32p)
    h = lambda x: x._h if x is not None else None
    off = lambda t, nbytes: C.c_void_p(t.data_ptr() + nbytes)

    def call(pb=rig.pbank, sb=rig.sbank, sog=(0, 1, 2, 3), hist=H, k=Kr, flags=0, pend=True, trigger=1, window=W8, mm=m, ring=_ptr(bufs["ring"]),
             st=_ptr(bufs["st"]), term=_ptr(bufs["term"])):
        return L.qr_blackbox_policy_grid(env._h, h(pb), rig.cbank._h, rig.dbank._h, h(sb), G, E, ip([0] * G), ip([0] * G), ip([0] * G), ip(sog), hist, k, flags,
                                         3, 0, _ptr(bufs["pend"]) if pend else None, _ptr(bufs["rec"]), _ptr(bufs["recf"]), trigger, window, mm, ring, st,
                                         term, env._stream())

    def refused(code, message, **kw):
        rc = call(**kw)
        err = L.qr_last_error()
        assert rc == code and b"qr_blackbox_policy_grid" in err and message in err, (kw, rc, err)
        torch.cuda.synchronize()
        for name, t in bufs.items():
            assert bool((t == (SENTINEL if t.dtype == torch.float32 else 7)).all()), name
        for x, y in zip(before, env.get_state_tensors()):
            assert x is None or torch.equal(x, y)

    bad_bb = dict(ring=None, trigger=4, window=0, mm=0)                               # every evaluator refusal comes before the black box's
    refused(_lib.QR_E_INVALID, b"num_steps", k=0, hist=-1, **bad_bb)
    for bad in (-1, 5 - ga, 5):
        refused(_lib.QR_E_INVALID, b"history must be in [0, 4 - gates_ahead]", hist=bad, sb=None, **bad_bb)
    refused(_lib.QR_E_INVALID, b"bank obs_len != env obs_len + 4 * history", hist=1, **bad_bb)
    refused(_lib.QR_E_INVALID, b"obs_len", hist=0, **bad_bb)                         # history 0 wants the env's own length ...
    refused(_lib.QR_E_INVALID, b"bank obs_len != env obs_len + 4 * history", pb=own, **bad_bb)
    refused(_lib.QR_E_INVALID, b"null sensing bank", sb=None, **bad_bb)
    refused(_lib.QR_E_INVALID, b"sensing_of_group[2] is outside the sensing bank", sog=(0, 1, 4, 3), **bad_bb)
    refused(_lib.QR_E_INVALID, b"pending_dev is required", pend=False, **bad_bb)
    # the black box's own, in qr_blackbox_policy's order: each call carries every later fault too
    refused(_lib.QR_E_INVALID, b"ring_dev and st_dev are required", ring=None, term=off(bufs["term"], 2), trigger=4, window=0, mm=0)
    refused(_lib.QR_E_INVALID, b"ring_dev and st_dev are required", st=None, trigger=4, window=0, mm=0)
    refused(_lib.QR_E_INVALID, b"ring_dev and st_dev must be 16-byte aligned", ring=off(bufs["ring"], 4), term=off(bufs["term"], 2), trigger=4, window=0, mm=0)
    refused(_lib.QR_E_INVALID, b"ring_dev and st_dev must be 16-byte aligned", st=off(bufs["st"], 8), trigger=4, window=0, mm=0)
    refused(_lib.QR_E_INVALID, b"term_dev must be 4-byte aligned", term=off(bufs["term"], 2), trigger=4, window=0, mm=0)
    for bad in (0, -1, E + 1):
        refused(_lib.QR_E_INVALID, b"rec_per_group must be in 1..envs_per_group", mm=bad, trigger=4, window=0)
    for bad in (-1, 4):
        refused(_lib.QR_E_INVALID, b"`trigger` takes QR_BLACKBOX_ON_CRASH | QR_BLACKBOX_ON_TIME_LIMIT", trigger=bad, window=0)
    refused(_lib.QR_E_INVALID, b"window must be >= 1", window=0)
    # ... and valid calls run: with the terminal buffer, without it, and with history 0 on a bank of the env's own length
    bufs["pend"].zero_(); bufs["rec"].zero_(); bufs["recf"].zero_(); bufs["st"].zero_()
    assert call() == _lib.QR_OK and call(term=None) == _lib.QR_OK
    torch.cuda.synchronize()
    assert bool((bufs["rec"][:, 5] == 2 * Kr).all()) and bool((bufs["st"][:, 1] >= 1).all()) and env.last_rollout_ms() > 0.0
    bufs["st"].zero_()
    assert call(pb=own, hist=0) == _lib.QR_OK
    own.close(); rig.close()


# ---- 7. the tool path ---------------------------------------------------------------------------------------------------------------------------
def test_blackbox_grid_and_record_grid_fly_the_evaluators_cells():
    from optimal_quad_control_rl_amd import SensingParams, blackbox_grid, evaluate_sensing_grid, record_grid
    from optimal_quad_control_rl_amd.ppo import ActorCritic
    from test_gpu_eval_grid import _twin
    from test_gpu_rollout_conditions import _conditions

    H, n, seed, m = 2, 120, 99, 40
    nets = []
    for s_ in (5, 6):
        torch.manual_seed(s_)
        net = ActorCritic(24 + 4 * H, 4)
        with torch.no_grad():
            net.pi[-1].bias.copy_(torch.tensor([0.4, 0.4, 0.4, 0.4]))
        nets.append(net.pi)
    conds = [_conditions("e2e")[2]]                                                   # max_steps 40: time limits inside the flight
    ev = _twin("e2e", 2 * E, 1, conds[0], seed=1)                                     # two cells per launch: the four cells take two batches
    sensors = [SensingParams("noisy", *NOISY).with_delay(2), SensingParams.ideal()]
    kw = dict(envs_per_cell=E, seed=seed, noise_seed=7, command_history=H)
    want = evaluate_sensing_grid(nets, conds, sensors, ev, n_eval_steps=n, window_steps=n, **kw)
    logs = blackbox_grid(nets, conds, sensors, ev, n_steps=n, window=16, trigger="any", rec_per_cell=m, **kw)
    recs = record_grid(nets, conds, sensors, ev, n_steps=n, rec_per_cell=m, **kw)
    assert len(logs) == 2 and len(logs[0]) == 1 and len(logs[0][0]) == 2
    for p in range(2):
        for s_ in range(2):
            log, rec, total = logs[p][0][s_], recs[p][0][s_], want[p][0][s_]["total"]
            assert log.evaluation == total and rec.evaluation == total, (p, s_)
            assert log.num_envs == m and log.window == 16 and log.frozen.all() and log.last_step == n - 1
            assert rec.rows.shape == (n, m, 24) and not np.isnan(rec.rows).any()
            code = rec.rows[..., 21]
            first_end = (code != 0).argmax(axis=0)                                     # every env ends by step 40
            for j in (0, m - 1):                                                       # the log's flight is the record's rows up to the first end
                f = log.flight(j)
                assert np.array_equal(f, rec.rows[first_end[j] - len(f) + 1:first_end[j] + 1, j]), (p, s_, j)
            if s_ == 0:
                assert not rec.rows[:2, :, 16:20].any() and rec.rows[2:6, :, 16:20].any(), "two steps of delay: zeros first"
    assert logs[0][0][0].evaluation != logs[0][0][1].evaluation and not np.array_equal(recs[0][0][0].rows, recs[1][0][0].rows)
    ev.close()


# ---- 8. time, printed ---------------------------------------------------------------------------------------------------------------------------
def test_blackbox_grid_time_is_printed():
    """Median us per step at N = 65 536 = 256 groups x 256 envs, K = 200, E2E + residual MLPs + training disturbances, square track, gates_ahead 1,
    command history 2, the NOISY sensor with d = 2 in every group, both precisions: (a) trigger = crash, window 64, every env recorded, against
    the evaluator twin (qr_evaluate_policy_history_grid, whose code this change does not touch); (b) trigger 0, window = K against
    qr_record_policy with a policy of the same row length.  Launches alternate from the same seeded reset in ORDER-SWAPPED pairs, one warm-up
    pair, medians of 6, host clock around a stream synchronise.  NO bound is asserted: nobody had measured this launch when the test was
    written (DESIGN.md section 8 and profiles/blackbox_grid_time.txt hold the numbers of one run)."""
    from optimal_quad_control_rl_amd import Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, square_track
    from optimal_quad_control_rl_amd.conditions import Condition
    from optimal_quad_control_rl_amd.policy import MfmaPolicy, MfmaPolicyBank
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    n, Kc, H = 65536, 200, 2
    groups = n // E
    env = Quadcopter3DGates(n, *square_track(), gates_ahead=1, infos_mode="none", seed=99)
    env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    wide = Quadcopter3DGates(n, *square_track(), gates_ahead=3, infos_mode="none", seed=99)     # the recorder at the same row length (32)
    wide.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    Wd = env.state_len + 4 * H
    assert Wd == wide.state_len == 32
    cbank, dbank, sbank = _bank("e2e", [Condition.from_env(env)]), _dynamics_bank("e2e", [None]), _sensing_bank([_sensor(NOISY, 2)])
    torch.manual_seed(0)
    actor = ActorCritic(Wd, 4).pi
    pol = MfmaPolicy(Wd).load_torch(actor)
    pbank = MfmaPolicyBank(Wd, 1)
    pbank.load_torch(0, actor)
    dev, zero = env.device, [0] * groups
    pend, (rec, recf) = _pending(env), _records(env)
    r = env.STATE_LEN + 8
    big = torch.empty((Kc, n, r), device=dev)                                         # ring [K][N][R] of (b) and the recorder's rows; (a) uses its head
    st, term = torch.zeros((n, 4), dtype=torch.int32, device=dev), torch.empty((n, env.STATE_LEN), device=dev)
    stream = torch.cuda.current_stream(dev)

    def timed(e, launch):
        e.seed(99); e.reset_device()
        pend.zero_(); rec.zero_(); recf.zero_(); st.zero_()
        stream.synchronize()
        t0 = time.perf_counter()
        launch()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e6 / Kc

    for precision in ("f16-operands", "f32"):
        box = lambda trigger, window: env.blackbox_grid_device(pbank, cbank, dbank, sbank, zero, zero, zero, zero, H, E, Kc, pend, rec, recf,
                                                               precision=precision, noise_seed=1, window=window, trigger=trigger, rec_per_group=E,
                                                               ring=big[:window], status=st, terminal=term)
        pairs = {
            "(a) black box, trigger crash, window 64 / evaluator twin":
                (env, lambda: box(1, 64), env, lambda: env.evaluate_history_grid_device(pbank, cbank, dbank, sbank, zero, zero, zero, zero, H, E, Kc, pend, rec,
                                                                                        recf, precision=precision, noise_seed=1)),
            "(b) recorder form, trigger 0, window K / qr_record_policy":
                (env, lambda: box(0, Kc), wide, lambda: wide.record_policy_device(pol, Kc, torch.zeros(4), deterministic=True, out=big, precision=precision)),
        }
        for what, (ea, fa, eb, fb) in pairs.items():
            ta, tb = [], []
            for rep in range(7):
                if rep % 2 == 0:
                    a = timed(ea, fa); b = timed(eb, fb)
                else:
                    b = timed(eb, fb); a = timed(ea, fa)
                if rep:
                    ta.append(a); tb.append(b)
            ma, mb = statistics.median(ta), statistics.median(tb)
            print("%s, %s: median %.4f us/step %s against %.4f us/step %s; ratio %.4f"
                  % (what, precision, ma, ["%.3f" % t for t in ta], mb, ["%.3f" % t for t in tb], ma / mb))
            assert ma > 0.0 and mb > 0.0
    for x in (env, wide, cbank, dbank, sbank, pol, pbank):
        x.close()
