"""CPU: the device-side prepare of a population round in the build, the package and the tool (qr_ppo_population_load_bank,
qr_policy_bank_read and qr_ppo_population_prepare themselves are pinned in tests/abi_table.py); the two structs of _lib.py have the header's
field order and layout; the Python-side refusals come before anything touches a GPU."""
import ctypes as C
import os
import re

import pytest

import abi_decl
from abi_decl import stub_env as _stub_env   # the GPU tests import it from here

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHARED_FIELDS = [("int32_t", ["K", "N", "E"]), ("const float *", ["obs", "act", "logp", "rew"]), ("const uint8_t *", ["done", "trunc"]),
                 ("const float *", ["last_obs"]), ("const float *", ["term_obs"])]
MEMBER_FIELDS = [("int32_t", ["first_env"]), ("float", ["gamma", "lam"]), ("float *", ["obs", "act", "old_logp", "rew", "done", "val"]),
                 ("float *", ["term_val"]), ("float *", ["last_val"]), ("float *", ["adv", "ret"]), ("float *", ["ep_ret", "ep_len", "ep_gates"])]


def test_structs_match_the_header():
    from optimal_quad_control_rl_amd import _lib

    _, code = abi_decl.header()
    for cname, expected, ctype in (("qr_ppo_prepare_shared", SHARED_FIELDS, _lib.QrPpoPrepareShared),
                                   ("qr_ppo_prepare_member", MEMBER_FIELDS, _lib.QrPpoPrepareMember)):
        declared = abi_decl.struct_fields(code, cname)
        assert declared == [(t, n) for t, names in expected for n in names], cname
        fields = ctype._fields_
        assert [n for n, _ in fields] == [n for _, n in declared], cname
        for (name, ct), (ctext, _) in zip(fields, declared):
            assert ct is {"int32_t": C.c_int32, "float": C.c_float}.get(ctext, C.c_void_p), (cname, name)
    # the C layout on this ABI: three ints + padding to the first pointer
    assert C.sizeof(_lib.QrPpoPrepareShared) == 16 + 8 * 8 and _lib.QrPpoPrepareShared.obs.offset == 16
    assert _lib.QrPpoPrepareShared.term_obs.offset == 16 + 7 * 8
    assert C.sizeof(_lib.QrPpoPrepareMember) == 16 + 13 * 8 and _lib.QrPpoPrepareMember.obs.offset == 16
    assert _lib.QrPpoPrepareMember.term_val.offset == 16 + 6 * 8 and _lib.QrPpoPrepareMember.ep_gates.offset == 16 + 12 * 8


def test_the_kernels_are_where_the_header_says_and_wait_for_nobody():
    from optimal_quad_control_rl_amd import build

    text = open(os.path.join(build.CSRC, "quadrace_population_prepare.hip")).read()
    for kernel in ("population_load_bank_kernel", "population_value_kernel", "population_gather_kernel", "population_gae_kernel",
                   "population_report_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\b" % kernel, text), kernel
    code = re.sub(r"//[^\n]*", "", text)
    for word in ("atomic", "s_sleep", "Cooperative", "__threadfence", "hipGraph", "hipDeviceSynchronize"):
        assert word not in code, word
    assert "policy_forward<L>" in code                                  # the values come from the header function the collect kernels use
    assert code.count("hipStreamSynchronize") == 3                       # two regrow paths and the round's one blocking read
    # the accessor that marks the slots is host code next to qr::bank_weights
    policy = open(os.path.join(build.CSRC, "quadrace_policy.hip")).read()
    assert "bank_mark_set" in policy and "qr_policy_bank_read" in policy


def prepare_grids(P, E, K):
    """The grid sizes of the value and the gather launch.  MIRRORS qr_ppo_population_prepare (csrc/quadrace_population_prepare.hip: cpe,
    roll, vtiles, spread, vgrid, ggrid) and must change with it; test_many_tile_shapes_walk_several_tiles_per_workgroup holds the
    source's three lines against this restatement."""
    cpe = E // 256
    roll = K * cpe                         # rollout tiles = gather tiles = term_obs tiles
    vtiles = 2 * roll + cpe                # rollout, last_obs and term_obs tiles of the value launch
    spread = max(1, 1024 // P)
    return dict(cpe=cpe, roll=roll, vtiles=vtiles, vgrid=min(vtiles, spread), ggrid=min(roll, 4 * spread))


def value_tile_kind(tile, g):
    """0 = rollout rows, 1 = last_obs rows, 2 = term_obs rows: population_value_kernel's decoding of a tile index"""
    return 0 if tile < g["roll"] else 1 if tile < g["roll"] + g["cpe"] else 2


# The prepare cases at which a workgroup walks SEVERAL tiles (tests/test_gpu_population_prepare.py flies them).  N = P E.
MANY_TILE_SHAPES = [dict(L=13, P=256, E=256, K=33), dict(L=36, P=64, E=512, K=70)]


def late_plants(P, E, K):
    """Where the non-finite values go so that a workgroup meets them on its second or a later tile, from the rule above.  Tiles are
    (step t, chunk c of 256 rows); a workgroup w walks tiles w, w + grid, w + 2 grid, ...
      gather: NaN observation element and an infinite action in gather tile ggrid (workgroup 0, second iteration); tile 2 ggrid (its
              third) stays clean.
      term:   term_obs tile q = 2 vgrid + 1 gets a truncated row with a plant; the same workgroup's tile before it, q - vgrid, is a
              term_obs tile too and loses every truncation.
      last:   a last_obs plant in another member than member 0.
    Members P - 1, P - 2, P - 3: none of them carries one of _Case's early plants (members 0 .. 3)."""
    g = prepare_grids(P, E, K)
    cpe = g["cpe"]
    tile = lambda q: (q // cpe, q % cpe)
    q_term = 2 * g["vgrid"] + 1
    return dict(gather=dict(member=P - 1, tile=tile(g["ggrid"]), next_tile=tile(2 * g["ggrid"]), obs_row=200, obs_col=-1, act_row=100, act_col=3),
                term=dict(member=P - 2, empty_tile=tile(q_term - g["vgrid"]), tile=tile(q_term), row=77, q=(q_term - g["vgrid"], q_term)),
                last=dict(member=P - 3, row=E - 5))


def test_many_tile_shapes_walk_several_tiles_per_workgroup():
    """The conditions under which the many-tile cases are many-tile cases, for the shapes the GPU test uses: a change of the launch rule
    that turns them back into one-tile-per-workgroup cases fails here."""
    from optimal_quad_control_rl_amd import build

    text = open(os.path.join(build.CSRC, "quadrace_population_prepare.hip")).read()
    for line in ("const long long roll = (long long)K * cpe, vtiles = 2 * roll + cpe;",
                 "const int spread = 1024 / P > 1 ? 1024 / P : 1;",
                 "const int vgrid = (int)(vtiles < spread ? vtiles : spread), ggrid = (int)(roll < 4 * spread ? roll : 4 * spread);"):
        assert line in text, "the launch rule changed: restate it in prepare_grids and re-derive MANY_TILE_SHAPES\n" + line
    assert text.count("tile += gridDim.x") == 2
    assert prepare_grids(2, 256, 9) == dict(cpe=1, roll=9, vtiles=19, vgrid=19, ggrid=9)          # one tile per workgroup: the older cases
    assert prepare_grids(8, 256, 256) == dict(cpe=1, roll=256, vtiles=513, vgrid=128, ggrid=256)  # a real round
    for sh in MANY_TILE_SHAPES:
        P, E, K = sh["P"], sh["E"], sh["K"]
        g = prepare_grids(P, E, K)
        print(sh, g, "value tiles per workgroup %.2f, gather tiles per workgroup %.2f" % (g["vtiles"] / g["vgrid"], g["roll"] / g["ggrid"]))
        assert 1 <= P <= 256 and E % 256 == 0 and sh["L"] in (13, 16, 17, 20, 21, 24, 25, 28, 29, 32, 36)
        assert g["vtiles"] >= 3 * g["vgrid"]                                                       # (a)
        kinds = [{value_tile_kind(t, g) for t in range(w, g["vtiles"], g["vgrid"])} for w in range(g["vgrid"])]
        assert any(k == {0, 1, 2} for k in kinds), "no value workgroup visits all three kinds of tile"
        assert g["roll"] >= 2 * g["ggrid"] + 1                                                     # (b): workgroup 0 gathers three tiles
        # the late plants land where they are meant to
        lp = late_plants(P, E, K)
        cpe, index = g["cpe"], lambda tc: tc[0] * g["cpe"] + tc[1]
        ga = lp["gather"]
        first, second = index(ga["tile"]), index(ga["next_tile"])
        assert first >= g["ggrid"] and second == first + g["ggrid"] and second < g["roll"]
        assert ga["tile"][0] not in (0, 1, K - 1) and ga["next_tile"][0] not in (0, 1) and ga["obs_row"] != ga["act_row"]
        te = lp["term"]
        q0, q1 = index(te["empty_tile"]), index(te["tile"])
        assert (q0, q1) == te["q"] and 0 <= q0 < q1 < g["roll"] and q1 - q0 == g["vgrid"]
        t0, t1 = g["roll"] + cpe + q0, g["roll"] + cpe + q1                                        # as tiles of the value launch
        assert value_tile_kind(t0, g) == value_tile_kind(t1, g) == 2 and t0 % g["vgrid"] == t1 % g["vgrid"] and t0 // g["vgrid"] >= 1
        assert len({ga["member"], te["member"], lp["last"]["member"]}) == 3 and min(ga["member"], te["member"], lp["last"]["member"]) >= 4
    assert any(sh["E"] // 256 >= 2 for sh in MANY_TILE_SHAPES) and any(sh["P"] == 256 for sh in MANY_TILE_SHAPES)   # (c)
    assert any(sh["L"] % 4 == 0 for sh in MANY_TILE_SHAPES) and any(sh["L"] % 4 != 0 for sh in MANY_TILE_SHAPES)    # both load paths


def batched_prepare_refusals(env_factory):
    """The ValueError cases of PopulationPPO(batched_prepare=True); env_factory(n) -> an env of n envs that is never used."""
    from optimal_quad_control_rl_amd.population import PopulationPPO

    two = [dict(seed=3), dict(seed=4, learning_rate=1e-4)]
    ok = dict(n_steps=16, batch_size=1024, n_epochs=2, native_update=True)
    with pytest.raises(ValueError, match="batched_update"):
        PopulationPPO(env_factory(512), two, batched_prepare=True, **ok)
    with pytest.raises(ValueError, match="batched_update"):
        PopulationPPO(env_factory(512), two, batched_update=False, batched_prepare=True, **ok)
    # everything batched_update refuses is refused with batched_prepare too
    with pytest.raises(ValueError, match="native_update"):
        PopulationPPO(env_factory(512), two, batched_update=True, batched_prepare=True, **{**ok, "native_update": False})
    with pytest.raises(ValueError, match="f32"):
        PopulationPPO(env_factory(512), two, batched_update=True, batched_prepare=True, update_precision="f32", **ok)
    with pytest.raises(ValueError, match="policy_forward|f32"):
        PopulationPPO(env_factory(512), two, batched_update=True, batched_prepare=True, policy_forward="f32class", **ok)
    q3 = env_factory(512)
    q3.KIND, q3.trainer_state = "hover", None
    with pytest.raises(ValueError, match="race envs"):
        PopulationPPO(q3, two, batched_update=True, batched_prepare=True, **ok)


def test_batched_prepare_refusals_come_before_the_env_is_used():
    batched_prepare_refusals(_stub_env)


def test_package_surface_and_tool():
    import importlib.util
    import inspect

    from optimal_quad_control_rl_amd import population, ppo

    assert inspect.signature(population.PopulationPPO.__init__).parameters["batched_prepare"].default is False
    assert inspect.signature(ppo.MfmaPpoPopulationUpdater.load_bank).parameters["first_slot"].default == 0
    for method in ("load_bank", "prepare", "epoch", "status", "close"):
        assert callable(getattr(ppo.MfmaPpoPopulationUpdater, method)), method
    for method in ("_train_prepare", "_train_views", "_native_begin", "_native_finish"):
        assert callable(getattr(ppo.PPO, method)), method
    assert "batched_prepare=False" in population.__doc__ and "batched_prepare=True" in population.__doc__
    spec = importlib.util.spec_from_file_location("train_population", os.path.join(ROOT, "tools", "train_population.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parser().parse_args(["--seeds", "0-2", "--batched-update", "--batched-prepare"])
    assert a.batched_prepare is True and a.batched_update is True
    assert tool.parser().parse_args(["--seeds", "0-2", "--batched-update"]).batched_prepare is False
    assert tool.parser().parse_args(["--seeds", "0-2", "--batched-prepare"]).batched_update is False    # it implies nothing else ...
    text = open(os.path.join(ROOT, "tools", "train_population.py")).read()
    assert "--batched-prepare needs --batched-update" in text                                            # ... and main() refuses it alone
