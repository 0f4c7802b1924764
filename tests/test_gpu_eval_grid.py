"""GPU: the grid evaluator (qr_evaluate_policy_grid, eval_policy_grid_kernel<V, GA, kF32>) against the single-policy evaluator
(qr_evaluate_policy), which tests/test_gpu_evaluate.py already pins to tests/eval_spec.py.  Group g of a grid launch must equal an
E-env twin handle that was configured with the group's condition through the ordinary Python setters (constructor track,
disturbance_ranges, disturbance_scale, max_steps), seeded alike and flown by evaluate_device with the group's weights in an
MfmaPolicy: start state equal, integer records equal, float records bit-equal, the five state tensors and the observation buffer
bit-equal.  No tolerance anywhere.

The conditions below were picked on the CPU oracle before anything ran on a GPU: the constant-action policy was flown with
oracle.OracleEnv + eval_spec.step under each of them (1 024 envs and their first 256, seed 5, 600 steps) until each satisfied
eval_spec.nonvacuous_e2e / nonvacuous_indi (gate passes, laps, crashes, for INDI time-limit ends and all eight lap slots) and the
three gave pairwise different records; the closed-loop policy was flown there with a float32 forward and showed passes and ends
under the E2E conditions too.  Non-vacuity is asserted here on
the twins' own data, so a comparison of nothing with nothing fails instead of passing."""
import ctypes as C
import statistics
import types

import numpy as np
import pytest
import torch

import eval_spec as S
from eval_helpers import SENTINEL, _closed_loop_layers, _constant_layers, _group_equals, _policy_bank, _ptr, _records

pytestmark = pytest.mark.gpu

SC = S.SCENARIO


def _other_track():
    """12 gates 0.5 m apart, a little higher and off the axis, with another start"""
    g = 12
    pos = np.stack([0.5 * np.arange(g), np.full(g, 0.05), np.full(g, -1.4)], axis=1).astype(np.float32)
    return pos, np.zeros(g, np.float32), np.asarray((-0.8, 0.1, -1.4), np.float32)


# other ranges than the training ones: rows 0 and 5 have lo == hi, the case in which the observation scaling widens the range to
# (lo - 1, hi + 1) (R:419-441; update_obs_scale / the condition header), and the forces of rows 3, 4 are switched on
OTHER_RANGES = np.array([[0.01, 0.01], [-0.02, 0.04], [-0.015, 0.005], [-0.1, 0.1], [-0.05, 0.15], [-0.2, -0.2]], dtype=np.float32)


def condition_specs(variant):
    """The three conditions of a variant as plain dicts (also read by the CPU pick of the conditions)."""
    from optimal_quad_control_rl_amd import TRAIN_DISTURBANCE_RANGES

    a_track, b_track = S.scenario_track(), _other_track()
    gpl = SC[variant + "_gates_per_lap"]
    if variant == "e2e":
        return [dict(name="train x1", track=a_track, ranges=TRAIN_DISTURBANCE_RANGES, scale=1.0, max_steps=SC["max_steps"], gpl=gpl),
                dict(name="train x3", track=a_track, ranges=TRAIN_DISTURBANCE_RANGES, scale=3.0, max_steps=SC["max_steps"], gpl=gpl),
                dict(name="other", track=b_track, ranges=OTHER_RANGES, scale=1.5, max_steps=180, gpl=1)]
    return [dict(name="A 250", track=a_track, ranges=None, scale=1.0, max_steps=SC["max_steps"], gpl=gpl),
            dict(name="A 300", track=a_track, ranges=None, scale=1.0, max_steps=300, gpl=gpl),
            dict(name="B 220", track=b_track, ranges=None, scale=1.0, max_steps=220, gpl=1)]


def _conditions(variant):
    from optimal_quad_control_rl_amd.conditions import Condition

    return [Condition(s["name"], *s["track"], s["ranges"], s["scale"], s["max_steps"], s["gpl"]) for s in condition_specs(variant)]


def _twin(variant, n, gates_ahead, cond, seed=SC["seed"]):
    """an n-env handle configured with `cond` through the ordinary setters, seeded and reset"""
    from optimal_quad_control_rl_amd import Quadcopter3DGates, Quadcopter3DGatesINDI

    trk = (cond.gate_pos, cond.gate_yaw, cond.start_pos)
    if variant == "e2e":
        env = Quadcopter3DGates(n, *trk, gates_ahead=gates_ahead, seed=seed, infos_mode="none")   # residual MLPs: the default
        env.disturbance_ranges = cond.disturbance_ranges
        env.disturbance_scale = cond.disturbance_scale
    else:
        env = Quadcopter3DGatesINDI(n, *trk, gates_ahead=gates_ahead, seed=seed, infos_mode="none")
    env.max_steps = cond.max_steps
    env.reset_device()
    return env


def _two_policies(variant, obs_len):
    """slot 0: the scenario's constant action; slot 1: seeded closed loop around it"""
    act = np.asarray(SC[variant + "_action"], np.float32)
    return [_constant_layers(obs_len, act), _closed_loop_layers(obs_len, act, seed=3)]


def _condition_bank(variant, conds, capacity=None):
    from optimal_quad_control_rl_amd.conditions import ConditionBank

    bank = ConditionBank(0 if variant == "e2e" else 1, capacity or len(conds))
    for slot, c in enumerate(conds):
        bank.set(slot, c)
    return bank


def _grid_against_twins(variant, gates_ahead, E, precision, pol, cog, K=SC["steps"]):
    """One grid launch with the maps (pol, cog) against one twin per distinct (policy, condition) pair.  Returns the twins' integer
    records by pair."""
    from optimal_quad_control_rl_amd.policy import MfmaPolicy

    G = len(pol)
    conds = _conditions(variant)
    # the handle's own configuration is none of the conditions': the call must not use it
    env = _twin(variant, G * E, gates_ahead, conds[0].replace(max_steps=97, start_pos=(0.3, -0.2, -1.0)))
    sets = _two_policies(variant, env.state_len)
    pbank, cbank = _policy_bank(env.state_len, sets), _condition_bank(variant, conds)
    own = (env.gate_pos.copy(), env.start_pos.copy(), env.max_steps, np.array(env.disturbance_ranges), env.disturbance_scale)
    env.condition_starts(conds, cog, E)
    assert np.array_equal(own[0], env.gate_pos) and np.array_equal(own[1], env.start_pos) and own[2] == env.max_steps
    assert np.array_equal(own[3], env.disturbance_ranges) and own[4] == env.disturbance_scale      # the handle's own configuration is back
    start = env.get_state_tensors()
    rec, recf = _records(env)
    env.evaluate_grid_device(pbank, cbank, pol, cog, E, K, rec, recf, precision=precision)
    assert bool((rec[:, 22:] == 0).all()) and bool((recf[:, 3] == 0).all()) and bool((rec[:, 5] == K).all())
    after = env.get_state_tensors()
    obs_after = env.states_tensor.clone()
    twin_recs = {}
    for g in range(G):
        p, c = pol[g], cog[g]
        lo, hi = g * E, (g + 1) * E
        twin = _twin(variant, E, gates_ahead, conds[c])
        _group_equals(start, twin, lo, hi, "condition_starts, group %d" % g)        # every group starts as its E-env handle does
        mp = MfmaPolicy(twin.state_len).set_weights(sets[p])
        trec, trecf = _records(twin)
        twin.evaluate_device(mp, K, conds[c].gates_per_lap, trec, trecf, precision=precision)
        srec = trec.cpu().numpy()
        if (p, c) not in twin_recs:
            nv = S.nonvacuous_e2e(srec) if variant == "e2e" else S.nonvacuous_indi(srec)
            ends = int(srec[:, 1].sum() + srec[:, 2].sum())
            print(variant, gates_ahead, E, precision, "policy", p, "condition", conds[c].name, "passes", int(srec[:, 0].sum()), "ends", ends, nv)
            assert int(srec[:, 0].sum()) > 0 and ends > 0, (p, c)                     # every twin: gate passes, and crashes or time-limit ends
            if p == 0:
                assert nv["ok"], (c, nv)                                              # the constant policy: the scenario's full non-vacuity
            twin_recs[(p, c)] = srec
        assert torch.equal(rec[lo:hi], trec), ("integer records", g, p, c, int((rec[lo:hi] != trec).any(dim=1).sum()))
        assert torch.equal(recf[lo:hi].view(torch.int32), trecf.view(torch.int32)), ("float records", g, p, c)
        _group_equals(after, twin, lo, hi, "group %d" % g)
        assert torch.equal(obs_after[lo:hi], twin.states_tensor), ("observation buffer", g)   # the wrapper refreshed its buffer
        twin.close(); mp.close()
    env.close(); pbank.close(); cbank.close()
    return twin_recs


_CASES = [(v, g, e, p) for v in ("e2e", "indi") for g in (0, 1) for e in (256, 1024) for p in ("f16-operands", "f32")]
# every other instantiation of eval_policy_grid_kernel<variant, gates_ahead, f32class>, one workgroup per cell
_CASES += [(v, g, 256, p) for v in ("e2e", "indi") for g in (2, 3, 4) for p in ("f16-operands", "f32")]


@pytest.mark.parametrize("variant,gates_ahead,E,precision", _CASES, ids=["%s-ga%d-E%d-%s" % c for c in _CASES])
def test_every_cell_equals_a_standalone_handle(variant, gates_ahead, E, precision):
    """2 policies x 3 conditions, 6 groups, policy-major."""
    recs = _grid_against_twins(variant, gates_ahead, E, precision, [0, 0, 0, 1, 1, 1], [0, 1, 2, 0, 1, 2])
    for p in (0, 1):        # the three conditions give pairwise different records for the same policy
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert not np.array_equal(recs[(p, a)], recs[(p, b)]), (p, a, b)
    assert not np.array_equal(recs[(0, 0)], recs[(1, 0)])      # and the policies do fly differently


@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_an_arbitrary_group_map_matches_the_twins(variant):
    """policy and condition indices permuted and repeated: nothing depends on the map being sorted or a product"""
    _grid_against_twins(variant, 1, 256, "f16-operands", [1, 0, 1, 1, 0, 1, 0], [2, 0, 2, 1, 1, 0, 2])


@pytest.mark.parametrize("variant", ["e2e", "indi"])
@pytest.mark.parametrize("precision", ["f16-operands", "f32"])
def test_one_condition_equal_to_the_handle_is_the_bank_call(variant, precision):
    """Every group on the one condition that equals the handle's own configuration: records and state bit-equal to
    qr_evaluate_policy_bank on a handle configured alike."""
    from optimal_quad_control_rl_amd.conditions import Condition

    K, P, E = SC["steps"], 4, 256
    conds = _conditions(variant)
    a, b = _twin(variant, P * E, 1, conds[0]), _twin(variant, P * E, 1, conds[0])
    a.share_starts(E); b.share_starts(E)
    two = _two_policies(variant, a.state_len)
    pbank = _policy_bank(a.state_len, [two[0], two[1], two[1], two[0]])
    own = Condition.from_env(a, gates_per_lap=conds[0].gates_per_lap)
    cbank = _condition_bank(variant, [conds[2], own], capacity=3)
    ra, rfa = _records(a)
    rb, rfb = _records(b)
    a.evaluate_grid_device(pbank, cbank, [0, 1, 2, 3], [1, 1, 1, 1], E, K, ra, rfa, precision=precision)
    b.evaluate_bank_device(pbank, P, E, K, conds[0].gates_per_lap, rb, rfb, precision=precision)
    assert int(rb[:, 0].sum()) > 0 and int(rb[:, 1].sum() + rb[:, 2].sum()) > 0
    assert torch.equal(ra, rb) and torch.equal(rfa.view(torch.int32), rfb.view(torch.int32))
    for x, y in zip(a.get_state_tensors(), b.get_state_tensors()):
        assert x is None or torch.equal(x, y)
    assert torch.equal(a.states_tensor, b.states_tensor)
    a.close(); b.close(); pbank.close(); cbank.close()


@pytest.mark.parametrize("precision", ["f16-operands", "f32"])
def test_common_random_numbers_across_disturbance_scales(precision):
    """Same policy, two conditions that differ in disturbance_scale only (s = 1 and 2 s), shared starts, every env one step short of
    its time limit (the forcing pattern of tests/test_gpu_terminal_rows.py: the episode clock is set, nobody waits for a crash).  After
    ONE step every env of both groups has restarted with the same episode number from the same group-local stream: world, target,
    steps and episode are bit-equal between the groups, and `disturbances` is exactly 2 x (the reset table multiplies by the scale,
    a power of two here)."""
    from optimal_quad_control_rl_amd import disturbance_sweep

    E = 512
    base = _conditions("e2e")[0]
    env = _twin("e2e", 2 * E, 1, base)
    conds = disturbance_sweep(env, [1.0, 2.0])
    assert all(np.array_equal(c.gate_pos, base.gate_pos) and c.max_steps == base.max_steps for c in conds)
    env.share_starts(E)
    w, d, t, s, ep = env.get_state_tensors()
    env.set_state_tensors(steps=torch.full_like(s, base.max_steps - 1))
    sets = _two_policies("e2e", env.state_len)
    pbank, cbank = _policy_bank(env.state_len, sets), _condition_bank("e2e", conds)
    rec, recf = _records(env)
    env.evaluate_grid_device(pbank, cbank, [1, 1], [0, 1], E, 1, rec, recf, precision=precision)
    w2, d2, t2, s2, ep2 = env.get_state_tensors()
    assert bool((rec[:, 2] == 1).all()) and bool((s2 == 0).all()) and bool((ep2 == ep + 1).all())     # every env ended by the time limit and restarted
    assert not torch.equal(w2, w)
    for name, x in (("world", w2), ("target", t2), ("steps", s2), ("episode", ep2)):
        assert torch.equal(x[:E], x[E:]), name
    assert torch.equal(rec[:E], rec[E:]) and torch.equal(recf[:E].view(torch.int32), recf[E:].view(torch.int32))
    assert int((d2[:E] != 0).any(dim=1).sum()) == E                                                   # disturbances were drawn
    assert torch.equal((d2[:E] * 2.0).view(torch.int32), d2[E:].view(torch.int32))                    # ... and scale only: exactly 2 x
    assert not torch.equal(d2[:E], d[:E])
    env.close(); pbank.close(); cbank.close()


@pytest.mark.parametrize("variant", ["e2e", "indi"])
def test_one_grid_call_equals_two_with_the_records_carried_over(variant):
    E, pol, cog = 256, [0, 0, 0, 1, 1, 1], [0, 1, 2, 0, 1, 2]
    conds = _conditions(variant)
    a, b = _twin(variant, 6 * E, 1, conds[0]), _twin(variant, 6 * E, 1, conds[0])
    a.condition_starts(conds, cog, E); b.condition_starts(conds, cog, E)
    pbank, cbank = _policy_bank(a.state_len, _two_policies(variant, a.state_len)), _condition_bank(variant, conds)
    ra, rfa = _records(a)
    rb, rfb = _records(b)
    a.evaluate_grid_device(pbank, cbank, pol, cog, E, 600, ra, rfa)
    b.evaluate_grid_device(pbank, cbank, pol, cog, E, 250, rb, rfb)
    first = rb.clone()
    b.evaluate_grid_device(pbank, cbank, pol, cog, E, 350, rb, rfb)
    assert bool((first[:, 5] == 250).all()) and int(ra[:, 14:22].sum()) > int(first[:, 14:22].sum()) > 0
    assert torch.equal(ra, rb) and torch.equal(rfa.view(torch.int32), rfb.view(torch.int32))
    for x, y in zip(a.get_state_tensors(), b.get_state_tensors()):
        assert x is None or torch.equal(x, y)
    a.close(); b.close(); pbank.close(); cbank.close()


def test_grid_refusals_launch_nothing():
    """Host-side argument checks only: nothing invalid is ever launched."""
    from optimal_quad_control_rl_amd import _lib
    from optimal_quad_control_rl_amd.conditions import ConditionBank
    from optimal_quad_control_rl_amd.policy import MfmaPolicyBank

    G, E, K = 2, 256, 8
    n = G * E
    conds = _conditions("indi")
    env = _twin("indi", n, 1, conds[0])
    L = env._L
    sets = _two_policies("indi", env.state_len)
    pbank = _policy_bank(env.state_len, sets, capacity=3)            # slots 0, 1 set, slot 2 never set
    cbank = _condition_bank("indi", conds[:2], capacity=3)           # slots 0, 1 set, slot 2 never set
    assert L.qr_condition_bank_capacity(cbank._h) == 3
    rec = torch.full((n, S.REC_INTS), 7, dtype=torch.int32, device=env.device)
    recf = torch.full((n, S.REC_FLOATS), SENTINEL, dtype=torch.float32, device=env.device)
    before = env.get_state_tensors()
    i32p = C.POINTER(C.c_int32)

    def call(e=env, pb=pbank, cb=cbank, g=G, epg=E, pol=(0, 1), cog=(1, 0), k=K, flags=0, r=rec, rf=recf):
        pa = None if pol is None else np.asarray(pol, np.int32)
        ca = None if cog is None else np.asarray(cog, np.int32)
        return L.qr_evaluate_policy_grid(e._h, pb._h if pb is not None else None, cb._h if cb is not None else None, g, epg,
                                         None if pa is None else pa.ctypes.data_as(i32p), None if ca is None else ca.ctypes.data_as(i32p),
                                         k, flags, _ptr(r), _ptr(rf), e._stream())

    def refused(code, **kw):
        rc = call(**kw)
        assert rc == code, (list(kw.keys()), rc, L.qr_last_error())
        assert len(L.qr_last_error()) > 0 and L.qr_policy_last_error() == L.qr_last_error()
        torch.cuda.synchronize()
        assert bool((rec == 7).all()) and bool((recf == SENTINEL).all())
        for x, y in zip(before, env.get_state_tensors()):
            assert x is None or torch.equal(x, y)

    # everything qr_evaluate_policy_bank refuses, envs_per_group in the role of envs_per_policy
    refused(_lib.QR_E_INVALID, r=None)
    refused(_lib.QR_E_INVALID, k=0)
    refused(_lib.QR_E_INVALID, k=-3)
    refused(_lib.QR_E_INVALID, flags=1)
    refused(_lib.QR_E_INVALID, flags=4)
    refused(_lib.QR_E_INVALID, flags=2 | 8)
    refused(_lib.QR_E_INVALID, pb=None)
    big = torch.full((n * S.REC_INTS + 4,), 7, dtype=torch.int32, device=env.device)
    bigf = torch.full((n * S.REC_FLOATS + 4,), SENTINEL, dtype=torch.float32, device=env.device)
    refused(_lib.QR_E_INVALID, r=big[1:])
    refused(_lib.QR_E_INVALID, rf=bigf[2:])
    assert bool((big == 7).all()) and bool((bigf == SENTINEL).all())
    env.pause = True
    refused(_lib.QR_E_STATE)
    env.pause = False
    env.pause_if_collision = True
    refused(_lib.QR_E_STATE)
    env.pause_if_collision = False
    refused(_lib.QR_E_INVALID, g=0, pol=(), cog=())
    refused(_lib.QR_E_INVALID, g=-1)
    refused(_lib.QR_E_INVALID, epg=0)
    refused(_lib.QR_E_INVALID, epg=128, g=4, pol=(0, 1, 0, 1), cog=(0, 1, 0, 1))      # < 256 (4 x 128 == n)
    refused(_lib.QR_E_INVALID, epg=384)                                              # not a multiple of 256
    refused(_lib.QR_E_INVALID, g=1, pol=(0,), cog=(0,))                              # G E != n
    refused(_lib.QR_E_INVALID, g=3, pol=(0, 1, 0), cog=(0, 1, 0))
    refused(_lib.QR_E_INVALID, g=1, epg=1024, pol=(0,), cog=(0,))
    other_len = MfmaPolicyBank(env.state_len + 4, 2)
    refused(_lib.QR_E_INVALID, pb=other_len)
    other_len.close()
    # the grid's own refusals
    refused(_lib.QR_E_INVALID, cb=None)
    refused(_lib.QR_E_INVALID, pol=None)
    refused(_lib.QR_E_INVALID, cog=None)
    refused(_lib.QR_E_INVALID, pol=(0, 3))                                           # outside the policy bank's capacity
    refused(_lib.QR_E_INVALID, pol=(-1, 0))
    refused(_lib.QR_E_INVALID, cog=(3, 0))                                           # outside the condition bank's capacity
    refused(_lib.QR_E_INVALID, cog=(0, -1))
    refused(_lib.QR_E_INVALID, pol=(0, 2 ** 31 - 1))
    refused(_lib.QR_E_STATE, pol=(0, 2))                                             # a referenced policy slot that was never set
    assert b"policy bank" in L.qr_last_error()
    refused(_lib.QR_E_STATE, cog=(2, 0))                                             # a referenced condition slot that was never set
    assert b"condition bank" in L.qr_last_error()
    e2e_bank = ConditionBank(0, 2)
    e2e_bank.set(0, _conditions("e2e")[0]); e2e_bank.set(1, _conditions("e2e")[1])
    refused(_lib.QR_E_INVALID, cb=e2e_bank)                                          # a condition bank of another variant
    assert b"variant" in L.qr_last_error()
    e2e_bank.close()
    if torch.cuda.device_count() > 1:
        far = ConditionBank(1, 2, device=1)
        far.set(0, conds[0]); far.set(1, conds[1])
        torch.cuda.set_device(0)
        refused(_lib.QR_E_INVALID, cb=far)                                           # ... or of another device
        far.close()
    # an unset slot that no group references does not matter; qr_condition_bank_set's own refusals
    c0 = conds[0]
    with pytest.raises(_lib.QuadraceError):
        cbank.set(3, c0)
    with pytest.raises(_lib.QuadraceError):
        cbank.set(-1, c0)
    with pytest.raises(_lib.QuadraceError):
        cbank.set(2, c0.replace(gate_pos=c0.gate_pos[:1], gate_yaw=c0.gate_yaw[:1]))      # one gate
    with pytest.raises(_lib.QuadraceError):
        cbank.set(2, c0.replace(gate_pos=np.zeros((33, 3), np.float32), gate_yaw=np.zeros(33, np.float32)))   # > QR_MAX_GATES
    with pytest.raises(_lib.QuadraceError):
        cbank.set(2, c0.replace(gates_per_lap=0))
    with pytest.raises(_lib.QuadraceError):
        cbank.set(2, c0.replace(disturbance_ranges=OTHER_RANGES))                          # INDI has no disturbances
    f32p = C.POINTER(C.c_float)
    gp, gy, sp = (np.ascontiguousarray(x) for x in (c0.gate_pos, c0.gate_yaw, c0.start_pos))
    p = lambda x: x.ctypes.data_as(f32p)
    assert L.qr_condition_bank_set(cbank._h, 2, None, p(gy), c0.num_gates, p(sp), None, 1.0, 100, 2) == _lib.QR_E_INVALID
    assert L.qr_condition_bank_set(cbank._h, 2, p(gp), None, c0.num_gates, p(sp), None, 1.0, 100, 2) == _lib.QR_E_INVALID
    assert L.qr_condition_bank_set(cbank._h, 2, p(gp), p(gy), c0.num_gates, None, None, 1.0, 100, 2) == _lib.QR_E_INVALID
    assert L.qr_condition_bank_set(None, 0, p(gp), p(gy), c0.num_gates, p(sp), None, 1.0, 100, 2) == _lib.QR_E_INVALID
    refused(_lib.QR_E_STATE, cog=(2, 0))                                             # none of the refused sets filled slot 2
    # a handle whose own track has one gate is refused like the other evaluators refuse it
    one = _twin("indi", n, 1, c0.replace(gate_pos=c0.gate_pos[:1], gate_yaw=c0.gate_yaw[:1]))
    rc = call(e=one)
    assert rc == _lib.QR_E_INVALID and b"one gate" in L.qr_last_error()
    torch.cuda.synchronize()
    assert bool((rec == 7).all()) and bool((recf == SENTINEL).all())
    one.close()
    # ... and a valid call runs, reports its time, and leaves a registered terminal-observation buffer alone
    tb = torch.full((K, n, env.state_len), SENTINEL, device=env.device)
    env.set_terminal_obs_buffer(tb)
    cbank.set(2, c0.replace(max_steps=5))
    rec.zero_(); recf.zero_()
    assert call(flags=2, cog=(2, 2)) == _lib.QR_OK and call(rf=None, cog=(2, 2)) == _lib.QR_OK
    torch.cuda.synchronize()
    assert bool((tb == SENTINEL).all())
    assert bool((rec[:, 5] == 2 * K).all()) and int(rec[:, 2].sum()) >= n
    assert env.last_rollout_ms() > 0.0           # qr_last_step_many_ms reports the launch
    env.close(); pbank.close(); cbank.close()


def test_python_evaluate_grid_equals_per_cell_evaluation():
    """2 policies x 3 conditions on a 4-group env: two launches, the second padded.  Every cell equals evaluate_policy on an E-env twin
    configured with the cell's condition, dict for dict; robustness_table reads the same numbers."""
    from optimal_quad_control_rl_amd import evaluate_grid, evaluate_policy
    from optimal_quad_control_rl_amd.evaluation import robustness_table
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    def actor(seed, bias):
        torch.manual_seed(seed)
        net = ActorCritic(20 + 4, 4)
        with torch.no_grad():
            net.pi[-1].bias.copy_(torch.tensor(bias))
        return net.pi

    E, K, W, seed = 256, 600, 250, 99
    conds = _conditions("e2e")
    ev = _twin("e2e", 4 * E, 1, conds[0], seed=1)
    assert ev.state_len == 24
    entries = [actor(5, [0.4, 0.4, 0.4, 0.4]), actor(6, [0.35, 0.4, 0.35, 0.4])]
    res = evaluate_grid(entries, conds, ev, envs_per_cell=E, n_eval_steps=K, window_steps=W, seed=seed)
    assert len(res) == 2 and all(len(r) == 3 for r in res)
    assert ev.max_steps == conds[0].max_steps and np.array_equal(ev.gate_pos, conds[0].gate_pos)      # the env keeps its configuration
    for p, entry in enumerate(entries):
        m = types.SimpleNamespace(_net=types.SimpleNamespace(pi=entry))
        for c, cond in enumerate(conds):
            twin = _twin("e2e", E, 1, cond, seed=1)
            want = evaluate_policy(m, twin, n_eval_steps=K, window_steps=W, gates_per_lap=cond.gates_per_lap, seed=seed, precision="f16-operands")
            print(p, cond.name, res[p][c]["window"]["crashes_per_window"], res[p][c]["total"]["flying_lap_seconds"])
            assert want["total"]["steps"] == K and want["window"]["steps"] == W and want["total"]["envs"] == E
            assert res[p][c] == want, (p, c)
            twin.close()
    assert res[0][0] != res[0][1] and res[0][0] != res[1][0]
    assert sum(r["total"]["episodes"] for row in res for r in row) > 0
    table = robustness_table(res, [c.name for c in conds])
    assert [row[0] for row in table[1]] == [c.name for c in conds]
    assert table[1][2][1] == res[1][2]["window"]["crashes_per_window"] and table[0][1][3] == res[0][1]["window"]["gates_per_window"]
    ev.close()


def test_grid_not_slower_than_the_bank():
    """The per-step work of a grid workgroup is the bank's; only the once-per-launch staging and a dozen scalar loads differ.  Protocol
    of test_bank_not_slower_than_the_single_evaluator: N = 65 536 = 256 groups x 256 envs, one seeded network in every slot, K = 2 000,
    E2E + residual MLPs + training disturbances, square track, every group on the ONE condition that equals the handle's configuration;
    against qr_evaluate_policy_bank on the same handle: alternating launches, one warm-up pair, medians of 5, times from
    qr_last_step_many_ms.  f16 operands: grid <= 1.03 x bank (the margin of the three sibling tests: identical per-step work, and the
    GPUs of a pool differ by about 3 %).  The f32 ratio is printed WITHOUT a bound, and so is a second f16 run with 256 DISTINCT
    condition images (scales and both tracks cycling).
    Measured (one run of this test, us per step, grid vs bank): f16 4.925 vs 5.115, ratio 0.963; f32 21.809 vs 21.780, ratio 1.001; 256 distinct
    conditions 5.199 vs 5.692 (there the bank launch flies the handle's own condition in every group: not the same work)."""
    from optimal_quad_control_rl_amd import Quadcopter3DGates, TRAIN_DISTURBANCE_RANGES, square_track, zigzag_track
    from optimal_quad_control_rl_amd.conditions import Condition
    from optimal_quad_control_rl_amd.ppo import ActorCritic

    n, K, E = 65536, 2000, 256
    P = n // E
    env = Quadcopter3DGates(n, *square_track(), gates_ahead=1, infos_mode="none", seed=99)
    env.disturbance_ranges = TRAIN_DISTURBANCE_RANGES
    env.max_steps = 10 ** 6
    torch.manual_seed(0)
    pi = ActorCritic(env.state_len, 4).pi
    layers = [(m.weight, m.bias) for m in pi if isinstance(m, torch.nn.Linear)]
    pbank = _policy_bank(env.state_len, [layers] * P)
    own = Condition.from_env(env)
    assert own.gates_per_lap == 4
    zz = zigzag_track()
    distinct = [Condition.from_env(env, name="c%d" % i, disturbance_scale=(0, 0.5, 1, 2, 3)[(i // 2) % 5]) if i % 2 == 0 else
                Condition.from_env(env, name="c%d" % i, gate_pos=zz[0], gate_yaw=zz[1], start_pos=zz[2], disturbance_scale=(0, 0.5, 1, 2, 3)[(i // 2) % 5])
                for i in range(P)]
    cbank = _condition_bank("e2e", [own] + distinct)
    rec, recf = _records(env)
    pol, same, cyc = list(range(P)), [0] * P, list(range(1, P + 1))
    medians = {}
    for label, precision, cog in (("f16-operands", "f16-operands", same), ("f32", "f32", same), ("f16-operands, 256 distinct conditions", "f16-operands", cyc)):
        t_grid, t_bank = [], []
        for rep in range(6):
            env.seed(99); env.reset_device(); rec.zero_(); recf.zero_()
            env.evaluate_grid_device(pbank, cbank, pol, cog, E, K, rec, recf, precision=precision)
            ms_g = env.last_rollout_ms()
            env.seed(99); env.reset_device(); rec.zero_(); recf.zero_()
            env.evaluate_bank_device(pbank, P, E, K, 4, rec, recf, precision=precision)
            ms_b = env.last_rollout_ms()
            if rep:
                t_grid.append(ms_g * 1e3 / K); t_bank.append(ms_b * 1e3 / K)
        mg, mb = statistics.median(t_grid), statistics.median(t_bank)
        medians[label] = (mg, mb)
        print("%s: qr_evaluate_policy_grid %s -> median %.4f us/step; qr_evaluate_policy_bank %s -> median %.4f us/step; ratio %.4f"
              % (label, ["%.4f" % t for t in t_grid], mg, ["%.4f" % t for t in t_bank], mb, mg / mb))
    env.close(); pbank.close(); cbank.close()
    mg, mb = medians["f16-operands"]
    assert mg <= 1.03 * mb, (mg, mb, mg / mb)
