"""CPU-side checks of the evolution-strategies feature (no GPU needed): the qr_es_* entry points against include/quadrace.h and
optimal_quad_control_rl_amd/_lib.py in the manner of tests/abi_table.py, what they refuse without a device, properties of the NumPy
restatement tests/es_spec.py (which tests/test_gpu_es.py holds the kernels against), EvolutionStrategy's argument checks, and a
spec-only run of the synthetic ascent problem that fixes the sign convention: ASCENT, towards higher scores."""
import ctypes as C

import numpy as np
import pytest

import abi_decl
import es_spec as S
import test_abi_host
from abi_table import f32p, i32, row, u64, vp, vpp  # noqa: F401
from optimal_quad_control_rl_amd import _lib

ES = "quadrace_es.hip"
f32 = C.c_float
CONTRACT = ("typedef struct qr_es qr_es", ["CONTRACT", "bit for bit", "Refused before anything is launched", "no atomic", "qr_policy_bank_set",
                                           "DELIBERATE limit", "0x2545F491", "0x4F6CDD1D", "halving tree", "ascending", "Philox4x32-10",
                                           "QR_E_NO_DEVICE", "Adam ASCENT"])
_W = _lib.QrEsFitnessWeights(0, 0, 0, 0, -1, 1200)
ROWS = [
    row("qr_es_create", ["obs_len", "device", "num_pairs", "out"], types=["int32_t", "int32_t", "int32_t", "qr_es * *"], bound=[i32, i32, i32, vpp],
        optional=True, in_version_comment="qr_es_*", source=ES, default_flags=True, vgpr_form=True, defines={"QR_ABI_VERSION": 3}, contract=CONTRACT,
        patterns=[r"typedef\s+struct\s+qr_es\s+qr_es\s*;", r"QR_ES_SHAPE_CENTERED_RANK\s*=\s*0\s*,\s*QR_ES_SHAPE_NONE\s*=\s*1",
                  r"double\s+w_gate\s*,\s*w_crash\s*,\s*w_timeout\s*,\s*w_return\s*,\s*w_lap\s*;\s*double\s+no_lap_steps\s*;\s*int32_t\s+reserved\[2\]\s*;"
                  r"\s*\}\s*qr_es_fitness_weights\s*;"],
        null_call=((13, 0, 1, None), _lib.QR_E_INVALID, b"qr_es_create")),
    row("qr_es_destroy", ["es"], types=["qr_es *"], bound=[vp], optional=True),
    row("qr_es_num_params", ["es"], types=["const qr_es *"], bound=[vp], optional=True, null_call=((None,), _lib.QR_E_INVALID, b"qr_es_num_params")),
    row("qr_es_noise", ["es", "seed", "generation", "eps_dev", "stream"], types=["qr_es *", "uint64_t", "uint64_t", "float *", "void *"],
        bound=[vp, u64, u64, vp, vp], optional=True, null_call=((None, 0, 0, None, None), _lib.QR_E_INVALID, b"qr_es_noise")),
    row("qr_es_perturb", ["es", "theta_dev", "sigma", "seed", "generation", "bank", "first_slot", "theta_pop_dev", "stream"],
        types=["qr_es *", "const float *", "float", "uint64_t", "uint64_t", "qr_policy_bank *", "int32_t", "float *", "void *"],
        bound=[vp, vp, f32, u64, u64, vp, i32, vp, vp], optional=True,
        null_call=((None, None, 0.1, 0, 0, None, 0, None, None), _lib.QR_E_INVALID, b"qr_es_perturb")),
    row("qr_es_fitness", ["es", "rec_dev", "recf_dev", "envs_per_policy", "w", "summary_dev", "fitness_dev", "stream"],
        types=["qr_es *", "const int32_t *", "const float *", "int32_t", "const qr_es_fitness_weights *", "double *", "double *", "void *"],
        bound=[vp, vp, vp, i32, vp, vp, vp, vp], optional=True,
        null_call=((None, None, None, 256, C.byref(_W), None, None, None), _lib.QR_E_INVALID, b"qr_es_fitness")),
    row("qr_es_update", ["es", "theta_dev", "adam_m_dev", "adam_v_dev", "fitness_dev", "sigma", "seed", "generation", "shaping", "lr", "beta1", "beta2",
                         "eps", "weight_decay", "adam_step", "util_dev", "stream"],
        types=["qr_es *", "float *", "float *", "float *", "const double *", "float", "uint64_t", "uint64_t", "int32_t", "float", "float", "float", "float",
               "float", "int32_t", "float *", "void *"],
        bound=[vp, vp, vp, vp, vp, f32, u64, u64, i32, f32, f32, f32, f32, f32, i32, vp, vp], optional=True,
        null_call=((None, None, None, None, None, 0.1, 0, 0, 0, 0.01, 0.9, 0.999, 1e-8, 0.0, 1, None, None), _lib.QR_E_INVALID, b"qr_es_update")),
]


# ---- header <-> _lib ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", ROWS, ids=lambda r: r["name"])
def test_es_entry_points_are_pinned(r):
    """argument names, declared types, ctypes types, optional, version comment, source and flags, contract words"""
    test_abi_host.test_pinned_entry_points(r)
    assert r["name"] in _lib.SIGNATURES and r["name"] in _lib.OPTIONAL_SYMBOLS


def test_every_declared_es_function_has_a_row():
    declared = sorted(f[0] for f in abi_decl.functions(abi_decl.header()[1], "qr_es_"))
    assert declared == sorted(r["name"] for r in ROWS) and len(declared) == 7


def test_fitness_weights_struct_matches_the_header():
    code = abi_decl.header()[1]
    body = code.split("qr_es_fitness_weights;")[0].rsplit("typedef struct {", 1)[1]
    names = [n.strip() for stmt in body.split(";") if stmt.strip().startswith("double") for n in stmt.strip()[len("double"):].split(",")]
    fields = _lib.QrEsFitnessWeights._fields_
    assert names == [n for n, t in fields if t is C.c_double] == ["w_gate", "w_crash", "w_timeout", "w_return", "w_lap", "no_lap_steps"]
    assert fields[-1][0] == "reserved" and C.sizeof(_lib.QrEsFitnessWeights) == 6 * 8 + 2 * 4
    assert (_lib.QR_ES_SHAPE_CENTERED_RANK, _lib.QR_ES_SHAPE_NONE) == (S.SHAPE_CENTERED_RANK, S.SHAPE_NONE) == (0, 1)


# ---- refusals that need no device ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [r for r in ROWS if "null_call" in r], ids=lambda r: r["name"])
def test_null_calls_are_refused(r):
    test_abi_host.test_null_handles_are_refused_without_a_device(r)


def test_create_checks_its_arguments_before_it_asks_for_a_device():
    L = _lib.load()
    h = C.c_void_p()
    for obs_len, pairs in ((14, 1), (0, 1), (13, 0), (13, 129), (13, -1)):
        assert L.qr_es_create(obs_len, 0, pairs, C.byref(h)) == _lib.QR_E_INVALID, (obs_len, pairs)
        assert b"qr_es_create" in L.qr_last_error() and not h.value
    assert L.qr_es_destroy(None) == _lib.QR_OK


def test_create_without_a_device_is_no_device():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = _lib.load()
    h = C.c_void_p()
    for obs_len in (13, 16, 24, 36):
        assert L.qr_es_create(obs_len, 0, 128, C.byref(h)) == _lib.QR_E_NO_DEVICE
        assert b"no HIP device" in L.qr_last_error() and not h.value


# ---- properties of the restatement -----------------------------------------------------------------------------------------------------------
def test_num_params_is_the_actor_block():
    from optimal_quad_control_rl_amd import es

    for L in (13, 16, 17, 20, 21, 24, 25, 28, 29, 32, 36):
        assert S.num_params(L) == es.num_params(L) == 120 * L + 29644 and S.num_params(L) % 4 == 0


def test_ranks_are_a_permutation_and_utilities_sum_to_zero():
    rng = np.random.default_rng(3)
    for P in (2, 6, 16, 256):
        F = rng.normal(size=P)
        F[rng.integers(0, P, P // 3)] = 1.5      # ties
        r = S.ranks(F)
        assert sorted(r.tolist()) == list(range(P))
        assert all(r[a] < r[b] for a in range(P) for b in range(P) if F[a] < F[b])
        u = S.utilities(F, S.SHAPE_CENTERED_RANK)
        assert u.dtype == np.float32 and abs(float(u.astype(np.float64).sum())) <= P * 2.0 ** -24
        assert float(u.min()) == -0.5 and float(u.max()) == 0.5
    assert np.array_equal(S.utilities([1.0, -2.5], S.SHAPE_NONE), np.array([1.0, -2.5], np.float32))


def test_ties_go_by_index_and_nan_ranks_below_everything():
    nan, inf = float("nan"), float("inf")
    assert S.ranks([1.0, 1.0, 0.0, 1.0]).tolist() == [1, 2, 0, 3]
    assert S.ranks([0.0, nan, -inf, nan, 5.0]).tolist() == [3, 0, 2, 1, 4]
    assert S.ranks([nan, nan]).tolist() == [0, 1]
    assert S.ranks([0.0, -0.0]).tolist() == [0, 1]          # equal: by index


def test_antithetic_members_are_symmetric_about_theta():
    n, pairs, sigma = 64, 3, 0.07
    eps64, u = S.noise(n, pairs, seed=5, generation=2)
    assert eps64.shape == (pairs, n) and all(x.shape == (pairs, n // 4) for x in u)
    theta = np.random.default_rng(0).normal(size=n).astype(np.float32)
    eps = eps64.astype(np.float32)
    pop = S.members(theta, sigma, eps)
    assert pop.shape == (2 * pairs, n) and pop.dtype == np.float32
    d = (np.float32(sigma) * eps).astype(np.float64)       # before the second rounding: exactly symmetric
    assert np.array_equal(theta.astype(np.float64) + d, 2.0 * theta.astype(np.float64) - (theta.astype(np.float64) - d))
    assert np.array_equal(pop[0::2], (theta.astype(np.float64) + d).astype(np.float32))
    assert np.array_equal(pop[1::2], (theta.astype(np.float64) - d).astype(np.float32))
    # roughly standard normal, and the three streams do not share their key
    big = S.noise(4096, 4, seed=9, generation=0)[0]
    assert abs(big.mean()) < 0.03 and abs(big.std() - 1.0) < 0.03
    import action_noise as N

    assert S.es_key(7) != N.noise_key(7) and S.es_key(7) != (7, 0) and all(t != 0 for t in S.ES_KEY_TWEAK)
    assert not set(S.ES_KEY_TWEAK) & set(N.NOISE_KEY_TWEAK)


def test_summary_order_and_score():
    rng = np.random.default_rng(1)
    E = 512
    rec = rng.integers(0, 50, size=(2 * E, S.REC_INTS)).astype(np.int32)
    rec[E:, 15:22] = 0                                      # policy 1: no flying lap
    recf = (rng.normal(size=(2 * E, 4)) * 1e3).astype(np.float32)
    s = S.summary(rec, recf, E)
    assert s[0, 5] == rec[:E, 15:22].sum() and s[0, 6] == rec[:E, 7:14].sum() and s[1, 5] == 0
    assert s[0, 3] == rec[:E, 14].sum() and s[0, 4] == rec[:E, 6].sum()
    exact = (recf[:E, 1].astype(np.float64) + recf[:E, 0].astype(np.float64))
    assert abs(s[0, 7] - float(np.sum(exact))) <= 1e-9 * np.abs(exact).sum()
    assert np.array_equal(S.summary(rec, None, E)[:, 7], [0.0, 0.0])
    w = S.lap_weights(1200, 100.0)
    F = S.score(s, w, E)
    assert F[0] == -100.0 * s[0, 1] / E + -1.0 * (s[0, 6] / s[0, 5]) and F[1] == -100.0 * s[1, 1] / E - 1200.0


# ---- EvolutionStrategy's argument checks ---------------------------------------------------------------------------------------------------
def test_evolution_strategy_argument_checks():
    import torch

    from optimal_quad_control_rl_amd import EvolutionStrategy

    actor = torch.nn.Sequential(torch.nn.Linear(24, 120), torch.nn.ReLU(), torch.nn.Linear(120, 120), torch.nn.ReLU(), torch.nn.Linear(120, 120),
                                torch.nn.ReLU(), torch.nn.Linear(120, 4))
    env = abi_decl.stub_env(2 * 4 * 256)
    bad = [dict(pairs=0), dict(pairs=129), dict(pairs=3), dict(envs_per_policy=128, pairs=8), dict(envs_per_policy=300), dict(sigma=0.0),
           dict(sigma=float("inf")), dict(sigma=float("nan")), dict(lr=-1e-3), dict(lr=float("nan")), dict(betas=(0.9,)), dict(betas=(0.9, 1.0)),
           dict(weight_decay=-1.0), dict(shaping="ranks"), dict(fitness="reward"), dict(fitness=dict(w_laps=1.0)), dict(n_eval_steps=0),
           dict(eval_seeds="random"), dict(eps=0.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            EvolutionStrategy(env, actor, **{**dict(pairs=4, envs_per_policy=256), **kw})


# ---- the sign convention: the spec alone climbs ----------------------------------------------------------------------------------------------
def test_spec_ascends_the_synthetic_score():
    """F_p = -|theta_p[:K] - target|^2 under centered ranks: the restated update moves theta TOWARDS the target (ascent on F), with the
    settings the device test reuses; the distance at least halves."""
    A = S.ASCENT
    K, pairs = A["K"], A["pairs"]
    target = S.ascent_offset()
    theta, m, v = np.zeros(K, np.float32), np.zeros(K, np.float32), np.zeros(K, np.float32)
    d0 = float(np.linalg.norm(theta - target))
    for g in range(A["generations"]):
        eps = S.noise(K, pairs, A["seed"], g)[0].astype(np.float32)
        F = S.ascent_score(S.members(theta, A["sigma"], eps), target)
        theta, m, v, u = S.update(theta, m, v, F, eps, A["sigma"], S.SHAPE_CENTERED_RANK, A["lr"], *A["betas"], A["eps"], 0.0, g + 1)
    d1 = float(np.linalg.norm(theta - target))
    print("spec ascent: |theta - target| %.3f -> %.3f" % (d0, d1))
    assert d1 <= 0.5 * d0
    # one step with the scores negated moves the other way
    eps = S.noise(K, pairs, A["seed"], 0)[0].astype(np.float32)
    z = np.zeros(K, np.float32)
    F = S.ascent_score(S.members(z, A["sigma"], eps), target)
    up = S.update(z, z, z, F, eps, A["sigma"], S.SHAPE_CENTERED_RANK, A["lr"], *A["betas"], A["eps"], 0.0, 1)[0]
    down = S.update(z, z, z, -F, eps, A["sigma"], S.SHAPE_CENTERED_RANK, A["lr"], *A["betas"], A["eps"], 0.0, 1)[0]
    assert np.dot(up, target) > 0 > np.dot(down, target)
