"""CPU-side checks of the sensing-grid feature (no GPU needed): the qr_sensing_* / qr_evaluate_policy_sensing_grid entry points against
include/quadrace.h and optimal_quad_control_rl_amd/_lib.py in the manner of tests/abi_table.py and what they refuse without a device;
sensing.py (slot packing, validation, the two sweeps) against the restatement tests/sensing_spec.py; and the restatement itself: the group
map of every (variant, gates_ahead), the domain separation of the noise stream's counter and key, and the command queue on a hand-written
`done` pattern."""
import ctypes as C

import numpy as np
import pytest

import abi_decl
import action_noise as N
import sensing_spec as S
import test_abi_host
from abi_table import f32p, i32, i32p, row, u64, vp, vpp
from optimal_quad_control_rl_amd import _lib
from optimal_quad_control_rl_amd import sensing as M

SRC = "quadrace_eval_sensing.hip"
CONTRACT = ("typedef struct qr_sensing_bank qr_sensing_bank",
            ["CONTRACT", "bit for bit", "Refused before anything is launched", "scalar registers", "NOT modelled", "bias or drift", "correlated noise",
             "quantisation", "0x6A09E667", "0x3C6EF372", "(q << 24)", "2^56", "128 bytes", "add_rn(o[j], mul_rn(sigma[group(j)], eps[j]))",
             "cleared to zeros", "j + 1 steps ago", "+0.0f"])
_SIG, _DELAY = (C.c_float * 8)(), C.c_int32(0)
ROWS = [
    row("qr_sensing_bank_create", ["device", "capacity", "out"], types=["int32_t", "int32_t", "qr_sensing_bank * *"], bound=[i32, i32, vpp], optional=True,
        in_version_comment="qr_sensing_*", source=SRC, default_flags=True, vgpr_form=True, defines={"QR_ABI_VERSION": 3}, contract=CONTRACT,
        patterns=[r"typedef\s+struct\s+qr_sensing_bank\s+qr_sensing_bank\s*;"], same_as=[((0, None), "qr_dynamics_bank_create", (1, None))],
        null_call=((0, 1, None), _lib.QR_E_INVALID, b"qr_sensing_bank_create")),
    row("qr_sensing_bank_destroy", ["bank"], types=["qr_sensing_bank *"], bound=[vp], optional=True),
    row("qr_sensing_bank_capacity", ["bank"], types=["const qr_sensing_bank *"], bound=[vp], optional=True,
        null_call=((None,), _lib.QR_E_INVALID, b"qr_sensing_bank_capacity")),
    row("qr_sensing_bank_set", ["bank", "slot", "sigma8", "delay"], types=["qr_sensing_bank *", "int32_t", "const float *", "int32_t"],
        bound=[vp, i32, f32p, i32], optional=True, null_call=((None, 0, None, 0), _lib.QR_E_INVALID, b"qr_sensing_bank_set")),
    row("qr_sensing_bank_read", ["bank", "slot", "sigma8", "delay"], types=["const qr_sensing_bank *", "int32_t", "float *", "int32_t *"],
        bound=[vp, i32, f32p, i32p], optional=True, null_call=((None, 0, _SIG, C.byref(_DELAY)), _lib.QR_E_INVALID, b"qr_sensing_bank_read")),
    row("qr_evaluate_policy_sensing_grid",
        ["env", "policies", "conditions", "dynamics", "sensing", "num_groups", "envs_per_group", "policy_of_group", "condition_of_group",
         "dynamics_of_group", "sensing_of_group", "num_steps", "flags", "noise_seed", "first_step", "pending_dev", "rec_dev", "recf_dev", "stream"],
        types={3: "qr_dynamics_bank *", 4: "qr_sensing_bank *", 10: "const int32_t *", 13: "uint64_t", 14: "uint64_t", 15: "float *"},
        bound={4: vp, 7: i32p, 8: i32p, 9: i32p, 10: i32p, 11: i32, 12: i32, 13: u64, 14: u64}, optional=True,
        in_version_comment="qr_evaluate_policy_sensing_grid", in_exports="qr_*",
        same_as=[((0, 4), "qr_evaluate_policy_dynamics_grid", (0, 4)), ((5, 10), "qr_evaluate_policy_dynamics_grid", (4, 9)),
                 ((11, 13), "qr_evaluate_policy_dynamics_grid", (9, 11)), ((16, None), "qr_evaluate_policy_dynamics_grid", (11, None))],
        null_call=((None,) * 5 + (1, 256) + (None,) * 4 + (1, 0, 0, 0) + (None,) * 4, _lib.QR_E_INVALID, None)),
    row("qr_sensing_noise", ["env", "sensing", "slot", "envs_per_group", "num_steps", "noise_seed", "first_step", "out_dev", "stream"],
        types={1: "qr_sensing_bank *", 5: "uint64_t", 6: "uint64_t", 7: "float *"}, bound={2: i32, 3: i32, 4: i32, 5: u64, 6: u64}, optional=True,
        null_call=((None, None, 0, 256, 1, 0, 0, None, None), _lib.QR_E_INVALID, None)),
]


# ---- header <-> _lib <-> the built library --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", ROWS, ids=lambda r: r["name"])
def test_sensing_entry_points_are_pinned(r):
    test_abi_host.test_pinned_entry_points(r)
    assert r["name"] in _lib.SIGNATURES and r["name"] in _lib.OPTIONAL_SYMBOLS


def test_every_declared_sensing_function_has_a_row_and_is_exported():
    from optimal_quad_control_rl_amd import build

    code = abi_decl.header()[1]
    declared = sorted([f[0] for f in abi_decl.functions(code, "qr_sensing_")] + ["qr_evaluate_policy_sensing_grid"])
    assert abi_decl.declaration(code, "qr_evaluate_policy_sensing_grid")
    assert declared == sorted(r["name"] for r in ROWS) and len(declared) == 7
    build.build_native()
    L = C.CDLL(build.LIB)
    for name in declared:
        assert hasattr(L, name), name


@pytest.mark.parametrize("r", [r for r in ROWS if "null_call" in r], ids=lambda r: r["name"])
def test_null_calls_are_refused(r):
    test_abi_host.test_null_handles_are_refused_without_a_device(r)


def test_the_dynamics_grid_comment_points_to_the_sensing_grid():
    text = abi_decl.header()[0]
    comment = text.split("typedef struct qr_dynamics_bank qr_dynamics_bank")[0].rsplit("/*", 1)[1]
    assert "qr_evaluate_policy_sensing_grid" in comment and "no actuator delay and no observation noise" not in text


def test_python_exports():
    import optimal_quad_control_rl_amd as pkg

    for name in ("evaluate_sensing_grid", "SensingParams", "SensingBank", "noise_sweep", "delay_sweep"):
        assert name in pkg.__all__
    assert pkg.SensingParams is M.SensingParams and pkg.noise_sweep is M.noise_sweep and pkg.delay_sweep is M.delay_sweep


# ---- the group map ------------------------------------------------------------------------------------------------------------------------------
def test_group_map_of_every_variant_and_gates_ahead():
    assert S.GROUPS[(S.INDI, 0)].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4]
    assert S.GROUPS[(S.E2E, 1)].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 6, 7, 7, 7, 7]
    for v in (S.E2E, S.INDI):
        for ga in range(5):
            g = S.GROUPS[(v, ga)]
            L = (20 if v == S.E2E else 13) + 4 * ga
            assert len(g) == L == S.obs_len(v, ga) and S.num_blocks(L) <= S.MAX_BLOCKS
            counts = np.bincount(g, minlength=8).tolist()
            assert counts == [3, 3, 3, 3, 4 if v == S.E2E else 1, 3 * ga, ga, 4 if v == S.E2E else 0], (v, ga, counts)
            assert (np.diff(g[:S.STATE_LEN[v]]) >= 0).all()
    assert S.obs_len(S.E2E, 4) == 36 and S.num_blocks(36) == 9 and S.num_blocks(13) == 4


# ---- slots, validation, sweeps --------------------------------------------------------------------------------------------------------------------
def test_slot_packing_round_trips():
    p = M.SensingParams("imu", 0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, delay_steps=3)
    slot = p.pack()
    assert slot.dtype == np.float32 and slot.shape == (S.SLOT_FLOATS,) and slot.nbytes == 128
    want = S.pack_slot([0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08], 3)
    assert np.array_equal(slot.view(np.int32), want.view(np.int32))
    assert slot.view(np.int32)[8] == 3 and not slot.view(np.int32)[9:].any()
    back = M.SensingParams.unpack(slot)
    assert back == p and back.delay_steps == 3 and np.array_equal(back.sigma, p.sigma)
    ideal = M.SensingParams.ideal()
    assert ideal.is_ideal and not ideal.pack().view(np.int32).any() and not p.is_ideal
    assert not M.SensingParams.ideal().with_delay(1).is_ideal
    bad = slot.copy()
    bad[20] = 1.0
    with pytest.raises(ValueError):
        M.SensingParams.unpack(bad)
    assert M.SLOT_FLOATS == S.SLOT_FLOATS and M.MAX_DELAY == S.MAX_DELAY and M.QUEUE_FLOATS == S.QUEUE_FLOATS
    assert len(M.SIGMA_FIELDS) == S.SIGMAS


@pytest.mark.parametrize("field", M.SIGMA_FIELDS)
@pytest.mark.parametrize("bad", [-1e-3, float("nan"), float("inf"), -float("inf"), 1e39])
def test_a_sigma_must_be_finite_and_not_negative(field, bad):
    with pytest.raises(ValueError):
        M.SensingParams("x", **{field: bad})


@pytest.mark.parametrize("bad", [-1, 5, 1.5, 2 ** 31])
def test_delay_must_be_an_integer_in_range(bad):
    with pytest.raises(ValueError):
        M.SensingParams("x", delay_steps=bad)
    with pytest.raises(ValueError):
        M.SensingParams.ideal().with_delay(bad)
    if bad == int(bad):
        with pytest.raises(ValueError):
            S.DelayQueue(1, int(bad))


def test_negative_zero_is_stored_as_zero():
    p = M.SensingParams("x", sigma_pos=-0.0)
    assert not p.sigma.view(np.int32).any() and p.is_ideal


def test_sweeps():
    base = M.SensingParams("base", 0.02, 0.04, 0.01, 0.08, 0.0, 0.02, 0.01, 0.0, delay_steps=1)
    sweep = M.noise_sweep(base, [0, 0.5, 1, 2])
    assert [s.delay_steps for s in sweep] == [1] * 4 and len({s.name for s in sweep}) == 4
    assert not sweep[0].sigma.any() and sweep[2] == base
    for s, f in zip(sweep, (0, 0.5, 1, 2)):
        assert np.array_equal(s.sigma, (base.sigma.astype(np.float64) * f).astype(np.float32))
    delays = M.delay_sweep(base, [0, 1, 2, 3, 4])
    assert [s.delay_steps for s in delays] == [0, 1, 2, 3, 4] and all(np.array_equal(s.sigma, base.sigma) for s in delays)
    assert delays[1] == base and delays[0] != base
    with pytest.raises(ValueError):
        base.scaled(-1.0)
    with pytest.raises(ValueError):
        base.scaled(float("nan"))
    with pytest.raises(ValueError):
        M.delay_sweep(base, [0, 5])


# ---- the noise stream: counter and key ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 0xC0FFEE, 0x5EED << 32, 2 ** 64 - 1, 0x9E3779B9 ^ 0x6A09E667, (0x85EBCA6B ^ 0x3C6EF372) << 32])
def test_the_key_differs_from_every_other_stream_of_the_seed(seed):
    """Equal counters are possible (gid, step lo, step hi with q = 0 is an action-noise counter), so the KEYS must differ: reset stream
    (the seed itself), action noise, ES noise (quadrace_es.hip: 0x2545F491, 0x4F6CDD1D)."""
    s = seed & (2 ** 64 - 1)
    lo, hi = s & 0xFFFFFFFF, s >> 32
    mine = S.noise_key(seed)
    assert mine == (lo ^ 0x6A09E667, hi ^ 0x3C6EF372)
    others = [(lo, hi), N.noise_key(seed), (lo ^ 0x2545F491, hi ^ 0x4F6CDD1D)]
    assert N.noise_key(seed) == (lo ^ N.NOISE_KEY_TWEAK[0], hi ^ N.NOISE_KEY_TWEAK[1])
    for other in others:
        assert mine[0] != other[0] and mine[1] != other[1]          # both words differ for every seed: the tweaks differ word by word
    # the same counter under the two keys gives unrelated blocks
    ctr = [np.uint32(7), np.uint32(0), np.uint32(11), np.uint32(0)]
    a = N.philox4x32_10(*ctr, *mine)
    b = N.philox4x32_10(*ctr, *N.noise_key(seed))
    assert all(int(x) != int(y) for x, y in zip(a, b))


def test_counter_words_and_blocks_never_collide():
    """word 3 = (step hi & 0xFFFFFF) | (q << 24): with step < 2^56 the high word is below 2^24, so (step hi, q) -> word 3 is injective"""
    E, K, Q = 3, 4, 9
    for first in (0, 2 ** 32 - 2, 2 ** 56 - K, (0xABCDEF << 32) + 5):
        c = S.noise_counter(E, K, Q, env_id_base=2 ** 32 - 1, first_step=first)
        step = first + np.arange(K, dtype=np.uint64)
        assert np.array_equal(c[2][:, 0, 0], (step & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        assert np.array_equal(c[3][:, 0, :] & np.uint32(0xFFFFFF), np.broadcast_to((step >> np.uint64(32)).astype(np.uint32)[:, None], (K, Q)))
        assert np.array_equal(c[3][0, 0, :] >> np.uint32(24), np.arange(Q, dtype=np.uint32))
        gid = 2 ** 32 - 1 + np.arange(E)
        assert c[0][0, :, 0].tolist() == (gid & 0xFFFFFFFF).tolist() and c[1][0, :, 0].tolist() == (gid >> 32).tolist()
        quads = {tuple(int(w[k, e, q]) for w in c) for k in range(K) for e in range(E) for q in range(Q)}
        assert len(quads) == K * E * Q
    with pytest.raises(ValueError):
        S.noise_counter(1, 2, 1, first_step=2 ** 56 - 1)
    S.noise_counter(1, 1, 1, first_step=2 ** 56 - 1)
    # exhaustive over the high words' edges: distinct (hi, q) -> distinct word 3
    his = np.array([0, 1, 2 ** 24 - 1], np.uint32)
    word = (his[:, None] & np.uint32(0xFFFFFF)) | (np.arange(9, dtype=np.uint32) << np.uint32(24))[None, :]
    assert len(set(word.reshape(-1).tolist())) == 27


def test_noise_is_the_action_noise_arithmetic_on_the_new_counter():
    L, E, K, seed = 13, 5, 3, 0xC0FFEE + (0x5EED << 32)
    eps, u = S.noise(L, E, K, seed, env_id_base=9, first_step=2 ** 32 - 1)
    assert eps.shape == (K, E, 16) and u[0].shape == (K, E, 4)
    # block 0 of env e at step k: the action-noise restatement with this stream's key tweak, counter words (gid, step)
    for k in range(K):
        for e in range(E):
            step = 2 ** 32 - 1 + k
            x = N.philox4x32_10(np.uint32(9 + e), np.uint32(0), np.uint32(step & 0xFFFFFFFF), np.uint32((step >> 32) | (2 << 24)), *S.noise_key(seed))
            want, _, _ = N.box_muller(*N.uniforms(x))
            assert np.array_equal(eps[k, e, 8:12], np.asarray(want).reshape(4))
    swapped, _ = S.noise(L, E, K, seed, env_id_base=9, first_step=2 ** 32 - 1, swap_pairs=True)
    assert np.array_equal(swapped.reshape(K, E, 4, 4)[..., :2], eps.reshape(K, E, 4, 4)[..., 2:])
    assert abs(eps.mean()) < 0.3 and 0.7 < eps.std() < 1.3


def test_perturb_is_two_roundings():
    rng = np.random.default_rng(0)
    g = S.GROUPS[(S.E2E, 1)]
    o = rng.standard_normal((7, 24)).astype(np.float32)
    e = rng.standard_normal((7, 24)).astype(np.float32)
    sigma = np.asarray([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.0], np.float32)
    got = S.perturb(o, sigma, e, g)
    prod = (sigma[g].astype(np.float64) * e.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got, (o.astype(np.float64) + prod.astype(np.float64)).astype(np.float32))
    assert np.array_equal(got[:, 20:], o[:, 20:]) and not np.array_equal(got[:, :20], o[:, :20])


# ---- the command queue ----------------------------------------------------------------------------------------------------------------------------
def _cmd(t, n=2):
    return np.stack([np.full(4, 10.0 * (i + 1) + t, np.float32) for i in range(n)])


def test_queue_on_a_hand_written_done_pattern():
    """two envs, d = 2; env 1's episode ends at step 3.  flown[t] is the command of step t - 2, zeros for the first two steps of an
    episode; the step that ends the episode clears everything, its own command included."""
    q = S.DelayQueue(2, 2)
    done = [[0, 0], [0, 0], [0, 0], [0, 1], [0, 0], [0, 0], [0, 0]]
    flown = []
    for t, dn in enumerate(done):
        flown.append(q.exchange(_cmd(t)))
        q.clear(dn)
    flown = np.stack(flown)                    # [T, 2, 4]
    assert flown[:, 0, 0].tolist() == [0.0, 0.0, 10.0, 11.0, 12.0, 13.0, 14.0]
    assert flown[:, 1, 0].tolist() == [0.0, 0.0, 20.0, 21.0, 0.0, 0.0, 24.0]
    assert (flown == flown[..., :1]).all()
    c = q.canonical()
    assert c.shape == (2, 16) and c[0, :4].tolist() == [16.0] * 4 and c[0, 4:8].tolist() == [15.0] * 4 and not c[:, 8:].any()
    assert c[1, :4].tolist() == [26.0] * 4 and c[1, 4:8].tolist() == [25.0] * 4


@pytest.mark.parametrize("d", [0, 1, 2, 3, 4])
def test_queue_delays_by_d_and_continues_from_its_canonical_form(d):
    T = 9
    q = S.DelayQueue(1, d)
    flown = np.stack([q.exchange(_cmd(t, 1)) for t in range(T)])[:, 0, 0]
    assert flown.tolist() == [0.0] * min(d, T) + [10.0 + t for t in range(T - d)]
    c = q.canonical()
    assert c[0, :4 * d:4].tolist() == [10.0 + T - 1 - j for j in range(d)] and not c[0, 4 * d:].any()
    # a queue rebuilt from the canonical form goes on as the original does; entries behind d are dropped
    dirty = c.copy()
    dirty[0, 4 * d:] = 99.0
    r = S.DelayQueue(1, d, pending=dirty)
    assert np.array_equal(r.canonical(), c)
    assert np.array_equal(r.exchange(_cmd(T, 1)), q.exchange(_cmd(T, 1))) and np.array_equal(r.canonical(), q.canonical())
    q.clear([1])
    assert not q.canonical().any() and (d == 0 or q.exchange(_cmd(T + 1, 1))[0, 0] == 0.0)


# ---- the sweep tool's host side ---------------------------------------------------------------------------------------------------------------------
def test_sweep_tool_arguments_and_tables():
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import sensing_sweep as T

    assert T.parse_scales("0,0.5,1,2") == [0.0, 0.5, 1.0, 2.0] and T.parse_delays("0,1,2,3,4") == [0, 1, 2, 3, 4]
    assert T.parse_sigma("0.1") == [0.1] * 8 and len(T.parse_sigma(T.DEFAULT_SIGMA)) == 8
    for fn, bad in ((T.parse_scales, "-1"), (T.parse_scales, "1,1"), (T.parse_scales, "x"), (T.parse_scales, ""), (T.parse_delays, "5"),
                    (T.parse_delays, "1.5"), (T.parse_delays, "0,0"), (T.parse_sigma, "1,2"), (T.parse_sigma, "-1"), (T.parse_sigma, "nan")):
        with pytest.raises(SystemExit):
            fn(bad)
    cell = lambda c, lap: dict(window=dict(crashes_per_window=c), total=dict(flying_lap_seconds=lap))
    text = T.format_tables("ckpt.zip", [0.0, 1.0], [0, 2], [[cell(0.0, 2.5), cell(0.25, 2.75)], [cell(1.5, None), cell(3.0, 3.25)]])
    lines = text.split("\n")
    assert len(lines) == 8 and lines[0] == "ckpt.zip  crashes per window" and lines[4] == "ckpt.zip  flying-lap seconds"
    assert "d = 0" in lines[1] and "d = 2" in lines[1] and lines[2].split() == ["x0", "0.0000*", "0.2500"] and lines[3].split()[0] == "x1"
    assert lines[6].split()[1].endswith("*") and "*" not in lines[7]
