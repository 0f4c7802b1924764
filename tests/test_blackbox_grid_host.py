"""No GPU: the black box of the sensing-grid evaluator (qr_blackbox_policy_grid, csrc/quadrace_blackbox_grid.hip) as far as a host can see
it -- the declaration, the binding, the build list, a refusal that needs no device, the Python split of the buffers into cells, and the
ring / freeze model of tests/blackbox_spec.py applied to columns g M + j."""
import ctypes as C
import os

import numpy as np
import pytest

import abi_decl
import blackbox_spec as B
from optimal_quad_control_rl_amd import _lib, build

NAME, TWIN, MODEL = "qr_blackbox_policy_grid", "qr_evaluate_policy_history_grid", "qr_blackbox_policy"
OWN = ["trigger", "window", "rec_per_group", "ring_dev", "st_dev", "term_dev"]


def test_entry_point_is_declared_bound_and_optional():
    text, code = abi_decl.header_of(NAME)
    _, ret, names, types_ = abi_decl.declaration(code, NAME)
    _, _, twin_names, twin_types = abi_decl.declaration(code, TWIN)
    assert ret == "int" and twin_names[-1] == "stream"
    shared = len(twin_names) - 1                                                       # everything up to and including recf_dev
    assert twin_names[shared - 1] == "recf_dev"
    assert names[:shared] == twin_names[:shared] and types_[:shared] == twin_types[:shared], "the evaluator's list, names and types"
    assert names[shared:] == OWN + ["stream"]
    assert types_[shared:] == ["int32_t", "int32_t", "int32_t", "float *", "int32_t *", "float *", "void *"]
    _, _, model_names, model_types = abi_decl.declaration(code, MODEL)                   # the black box's own arguments keep their types
    for n, t in zip(names[shared:], types_[shared:]):
        if n in model_names:
            assert model_types[model_names.index(n)] == t, n
    restype, argtypes = _lib.SIGNATURES[NAME]
    twin_bound = _lib.SIGNATURES[TWIN][1]
    assert restype is C.c_int and len(argtypes) == len(names)
    assert list(argtypes[:shared]) == list(twin_bound[:shared]) and list(argtypes[shared:shared + 3]) == [C.c_int32] * 3
    for c_type, ctype in zip(types_, argtypes):
        assert abi_decl.binding_matches(c_type, ctype), (c_type, ctype)
    assert NAME in _lib.OPTIONAL_SYMBOLS and NAME in abi_decl.version_comment(text)
    assert abi_decl.define(code, "QR_ABI_VERSION") == 3
    assert NAME in open(os.path.join(build.CSRC, "exports.map")).read()
    comment = text.split("int %s(" % NAME)[0].rsplit("/*", 1)[1].replace("\n *", "")
    for word in ("CONTRACT (1)", "bit for bit", "`history` may be 0", "g M + j", "TRUE world state", "the command flown", "zeros for the episode's first d steps",
                 "(first_step + k) mod W", "Not recorded", "the step that freezes an env is also the step that clears its queue", "rec_per_group outside 1..envs_per_group", "[0, 4 - gates_ahead]"):
        assert word in comment, word
    assert hasattr(C.CDLL(build.build_native()), NAME)


def test_the_unit_is_built_with_the_flags_of_the_sensing_evaluator():
    src = "quadrace_blackbox_grid.hip"
    assert src in build.SOURCES and os.path.exists(os.path.join(build.CSRC, src))
    for s in (src, "quadrace_eval_sensing.hip"):
        assert s not in build.PER_SOURCE_FLAGS and s not in build.NO_VGPR_FORM
    text = open(os.path.join(build.CSRC, src)).read()
    assert "static_assert(blackbox_grid_lds_bytes<kE2E, 0, 4>() == 145280" in text and "160 * 1024" in text, "the LDS bound is pinned on the computed size"
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    assert "atomic" not in code.replace("__ATOMIC_", "").lower(), "no atomics (the fences of the tile helpers name a memory order, nothing else)"


def test_a_null_handle_is_refused_without_a_device():
    L = _lib.load()
    rc = L.qr_blackbox_policy_grid(*([None] * 5), 1, 256, None, None, None, None, 0, 1, 0, 0, 0, None, None, None, 1, 8, 1, None, None, None, None)
    assert rc == _lib.QR_E_INVALID and b"null env" in L.qr_last_error()


def test_blackbox_grid_refuses_its_arguments_before_it_touches_the_env():
    from optimal_quad_control_rl_amd import blackbox_grid, record_grid

    env = abi_decl.stub_env(512, gates_ahead=1, state_len=24, VARIANT=0)
    with pytest.raises(ValueError, match="trigger must be one of"):
        blackbox_grid([None], [None], [None], env, trigger="sometimes")
    with pytest.raises(ValueError, match="command_history"):
        blackbox_grid([None], [None], [None], env, command_history=4)
    with pytest.raises(ValueError, match="rec_per_cell"):
        blackbox_grid([None], [None], [None], env, rec_per_cell=257)
    with pytest.raises(ValueError, match="rec_per_cell"):
        record_grid([None], [None], [None], env, rec_per_cell=0)
    with pytest.raises(ValueError, match="multiple of 256"):
        record_grid([None], [None], [None], env, envs_per_cell=100)


def _rows(rng, K, cols, R):
    """recorder rows with end codes: most steps run on, some crash, some hit the time limit"""
    rows = rng.standard_normal((K, cols, R)).astype(np.float32)
    rows[..., R - 3] = rng.choice([0.0, 1.0, 2.0], p=[0.94, 0.03, 0.03], size=(K, cols)).astype(np.float32)
    return rows


@pytest.mark.parametrize("S", [16, 13])
def test_cells_give_back_their_own_columns(S):
    """ring [W][G M][R] of three cells; cell g of M columns is columns [g M, (g + 1) M) -- for two different M, so two different offsets"""
    from optimal_quad_control_rl_amd.blackbox import CrashLog, cell_columns

    rng = np.random.default_rng(S)
    R, W, G, K, first = S + 8, 8, 3, 21, 5
    for M in (3, 5):
        rows = _rows(rng, K, G * M, R)
        source, st, _ = B.run_arrays(rows, first, W, B.ON_CRASH)
        ring = B.ring_from_source(rows, source, np.nan)
        term = rng.standard_normal((G * M, S)).astype(np.float32)
        assert int(st[:, 0].sum()) >= 1 and int((st[:, 0] == 0).sum()) >= 1
        for g in range(G):
            cr, cs, ct = cell_columns(ring, st, term, g, M)
            assert cr.shape == (W, M, R) and cs.shape == (M, 4) and ct.shape == (M, S)
            # the cell alone, through the model: the same ring, status and flights
            src_g, st_g, _ = B.run_arrays(rows[:, g * M:(g + 1) * M], first, W, B.ON_CRASH)
            assert np.array_equal(cs, st_g) and np.array_equal(cr, B.ring_from_source(rows[:, g * M:(g + 1) * M], src_g, np.nan), equal_nan=True)
            assert np.array_equal(ct, term[g * M:(g + 1) * M])
            log = CrashLog(cr, cs, ct, first + K - 1, 0.01, evaluation={"envs": M})
            assert log.evaluation == {"envs": M} and log.num_envs == M
            for j in range(M):
                slots = B.valid_slots(cs[j], first, K, W)
                assert log.slots(j) == slots
                end = K - 1 if not cs[j, 0] else int(np.nonzero(rows[:, g * M + j, R - 3] == 1.0)[0][0])
                want = rows[end - len(slots) + 1:end + 1, g * M + j]
                assert np.array_equal(log.flight(j), want), (g, j)
        with pytest.raises(ValueError, match="lies outside"):
            cell_columns(ring, st, term, G, M)
    assert CrashLog(ring[:, :M], st[:M], None, 0, 0.01).evaluation is None              # the attribute is optional


def test_the_ring_model_on_columns_g_m_plus_j():
    """The kernel's addressing, restated: env g E + j with j < M writes column g M + j of slot (first_step + k) mod W while armed.  Rows of
    all G E envs in, columns out: the model applied to the recorded envs' rows is the model applied per group, side by side; continuation
    through the status gives the one-call result."""
    rng = np.random.default_rng(0)
    G, E, M, R, W, K, first = 4, 12, 5, 24, 8, 30, 2 ** 32 - 20
    rows = _rows(rng, K, G * E, R)
    recorded = np.concatenate([np.arange(g * E, g * E + M) for g in range(G)])
    assert recorded.tolist() == [g * E + j for g in range(G) for j in range(M)] and first % W != 0
    cols = rows[:, recorded]                                                          # column c = g M + j
    for trigger in (0, 1, 2, 3):
        source, st, _ = B.run_arrays(cols, first, W, trigger)
        ring = B.ring_from_source(cols, source, np.nan)
        for g in range(G):
            s_g, st_g, _ = B.run_arrays(rows[:, g * E:g * E + M], first, W, trigger)
            assert np.array_equal(st[g * M:(g + 1) * M], st_g)
            assert np.array_equal(ring[:, g * M:(g + 1) * M], B.ring_from_source(rows[:, g * E:g * E + M], s_g, np.nan), equal_nan=True)
        # two calls through the same status and ring
        s1, st1, _ = B.run_arrays(cols[:17], first, W, trigger)
        r1 = B.ring_from_source(cols[:17], s1, np.nan)
        s2, st2, _ = B.run_arrays(cols[17:], first + 17, W, trigger, status=st1)
        assert np.array_equal(st2, st) and np.array_equal(B.ring_from_source(cols[17:], s2, r1), ring, equal_nan=True)
        if trigger == 0:
            assert not st[:, 0].any() and (st[:, 1] == K).all()
        else:
            assert st[:, 0].any()
