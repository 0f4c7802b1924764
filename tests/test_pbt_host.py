"""CPU: population-based training above the device -- `PBT.plan` (truncation selection: exact sources and destinations on hand-written
fitness lists), the refusals of `PopulationPPO(pbt=...)` and `PopulationPPO.exploit` before anything touches a GPU, and where the
exploit kernel lives (qr_ppo_population_exploit itself, with the one refusal of the C call that a box without a GPU can reach, is
pinned in tests/abi_table.py)."""
import math
import os
import re

import numpy as np
import pytest

from optimal_quad_control_rl_amd.population import INHERITED, PBT, PERTURBABLE, PopulationPPO, check_exploit
from abi_decl import stub_env as _stub_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#          member:  0    1    2    3    4    5    6    7
FITNESS_8 = [5.0, 1.0, 6.5, 7.0, 0.5, 3.0, 3.5, 0.0]      # ranking: 3 2 0 6 5 1 4 7


def _draws(seed, decision, per_destination, destinations):
    """What the schedule's documented generator gives: default_rng((seed, decision)), `per_destination` integers per destination in
    index order (the first picks the source among the top set, the last the sign of the shift)."""
    rng = np.random.default_rng((seed, decision))
    return {p: [int(rng.integers(hi)) for hi in per_destination] for p in sorted(destinations)}


def test_plan_p8_quarter_hand_written():
    pbt = PBT(quantile=0.25, seed=11)
    src_of, factors = pbt.plan(FITNESS_8, 0)
    top, bottom = [3, 2], [4, 7]                                   # ceil(0.25 * 8) = 2 of each
    d = _draws(11, 0, (2,), bottom)                                # the source only: no perturbed names, no shift, so no other draw
    want = list(range(8))
    for p in bottom:
        want[p] = top[d[p][0]]
    assert src_of == want
    assert [p for p in range(8) if src_of[p] != p] == bottom and all(src_of[p] in top for p in bottom)
    assert [f is not None for f in factors] == [p in bottom for p in range(8)]
    assert all(factors[p] == {"log_std_shift": 0.0} for p in bottom)
    # one of each: nothing is drawn that a hand cannot follow
    one = PBT(quantile=0.125).plan(FITNESS_8, 5)[0]
    assert one == [0, 1, 2, 3, 4, 5, 6, 3]
    # an odd population at the largest quantile: ceil(2.5) = 3 on each side would overlap in the middle member; the top set keeps it
    src5, _ = PBT(quantile=0.5).plan([1.0, 2.0, 3.0, 4.0, 5.0], 0)
    assert [p for p in range(5) if src5[p] != p] == [0, 1] and all(src5[p] in (2, 3, 4) for p in (0, 1))


def test_plan_ties_go_by_index():
    # six members tie at 1.0: the lower index ranks higher, so the top two are 0 and 1 and the bottom two 6 and 7
    src_of, _ = PBT(quantile=0.25).plan([1.0] * 8, 0)
    assert [p for p in range(8) if src_of[p] != p] == [6, 7] and all(src_of[p] in (0, 1) for p in (6, 7))
    src_of, _ = PBT(quantile=0.125).plan([2.0, 9.0, 9.0, 2.0, 2.0, 2.0, 2.0, 2.0], 0)
    assert src_of == [0, 1, 2, 3, 4, 5, 6, 1]                     # 1 before 2 at the top, 7 after every other 2.0 at the bottom


def test_plan_members_without_a_fitness_rank_last_and_are_never_sources():
    nan = float("nan")
    src_of, _ = PBT(quantile=0.25).plan([None, 4.0, nan, 2.0, 3.0, 1.0, 9.0, 8.0], 3)
    assert [p for p in range(8) if src_of[p] != p] == [0, 2] and all(src_of[p] in (6, 7) for p in (0, 2))
    # fewer members with a fitness than the top set has places: the one that has one is the only source, and is not overwritten
    src_of, _ = PBT(quantile=0.5).plan([None, None, 0.25, nan], 0)
    assert src_of == [0, 2, 2, 2]                                  # ranking 2 0 1 3: the bottom two are 1 and 3
    # nobody has one: nothing happens
    for fit in ([None] * 8, [nan] * 8, [None, nan] * 4):
        assert PBT().plan(fit, 0) == (list(range(8)), [None] * 8)


def test_plan_is_a_pure_function_of_seed_and_decision_index():
    kw = dict(quantile=0.5, perturb={"learning_rate": (0.8, 1.25), "ent_coef": (0.5, 2.0)}, log_std_shift=0.1)
    fit = [float(x) for x in range(16)]
    a, b = PBT(seed=4, **kw), PBT(seed=4, **kw)
    plans = [a.plan(fit, k) for k in range(6)]
    assert plans == [b.plan(fit, k) for k in range(6)] and plans == [a.plan(fit, k) for k in range(6)]    # no hidden state
    assert len({repr(p) for p in plans}) > 1                                                            # the index matters
    assert [PBT(seed=5, **kw).plan(fit, k) for k in range(6)] != plans                                   # and so does the seed
    # the documented draw order: per destination in index order -- source, one factor per name in sorted order, the sign
    d = _draws(4, 2, (8, 2, 2, 2), range(8))
    src_of, factors = plans[2]
    top = list(range(15, 7, -1))
    for p in range(8):
        assert src_of[p] == top[d[p][0]]
        assert factors[p] == {"ent_coef": (0.5, 2.0)[d[p][1]], "learning_rate": (0.8, 1.25)[d[p][2]], "log_std_shift": 0.1 if d[p][3] else -0.1}


def test_sources_are_never_destinations_and_results_stay_inside_bounds():
    rng = np.random.default_rng(0)
    pbt = PBT(quantile=0.5, perturb={"learning_rate": (0.8, 1.25), "clip_range": (0.5, 1.5)}, log_std_shift=0.2, seed=1,
              bounds={"learning_rate": (2.9e-4, 3.2e-4), "clip_range": (0.1, 0.25)})
    for k in range(40):
        P = int(rng.integers(2, 33))
        fit = [None if rng.random() < 0.2 else float(rng.integers(0, 4)) for _ in range(P)]
        src_of, factors = pbt.plan(fit, k)
        check_exploit(P, src_of, [0.0 if f is None else f["log_std_shift"] for f in factors])      # what the device call accepts
        for p in range(P):
            s = src_of[p]
            assert src_of[s] == s
            if s != p:
                assert fit[s] is not None and (fit[p] is None or fit[p] <= fit[s])
                assert factors[p]["learning_rate"] in (0.8, 1.25) and factors[p]["clip_range"] in (0.5, 1.5)
                assert factors[p]["log_std_shift"] in (0.2, -0.2)
                assert 2.9e-4 <= pbt.perturbed("learning_rate", 3e-4, factors[p]["learning_rate"]) <= 3.2e-4
                assert 0.1 <= pbt.perturbed("clip_range", 0.2, factors[p]["clip_range"]) <= 0.25
    assert pbt.perturbed("learning_rate", 3e-4, 1.25) == 3.2e-4 and pbt.perturbed("learning_rate", 3e-4, 0.8) == 2.9e-4
    assert pbt.perturbed("clip_range", 0.2, 0.5) == 0.1 and pbt.perturbed("ent_coef", 0.01, 2.0) == 0.02     # no bound given: none applied


def test_schedule_refusals_and_position():
    for bad in (dict(quantile=0.51), dict(quantile=0.0), dict(quantile=-0.1), dict(interval=0), dict(interval=2.5), dict(warmup_rounds=-1),
                dict(fitness="flying_lap"), dict(perturb={"gamma": (0.9, 1.1)}), dict(perturb={"learning_rate": (0.8,)}),
                dict(perturb={"learning_rate": (0.0, 1.25)}), dict(bounds={"learning_rate": (1.0, 0.5)}), dict(bounds={"n_steps": (1, 2)}),
                dict(log_std_shift=float("nan")), dict(log_std_shift=-0.1)):
        with pytest.raises(ValueError):
            PBT(**bad)
    assert PBT(quantile=0.5).quantile == 0.5 and callable(PBT(fitness=lambda pop: [0.0]).fitness)
    pbt = PBT(interval=3, warmup_rounds=2)
    assert [r for r in range(1, 13) if pbt.due(r)] == [5, 8, 11]
    assert [r for r in range(1, 7) if PBT(interval=2).due(r)] == [2, 4, 6]
    assert set(PERTURBABLE.values()) <= set(INHERITED) and set(PERTURBABLE) == {"learning_rate", "clip_range", "ent_coef"}


def test_population_refuses_a_bad_schedule_before_the_env_is_used():
    two = [dict(seed=3), dict(seed=4)]
    with pytest.raises(ValueError, match="PBT"):
        PopulationPPO(_stub_env(512), two, pbt=dict(interval=2))
    with pytest.raises(ValueError, match="two members"):
        PopulationPPO(_stub_env(256), [dict(seed=3)], pbt=PBT())
    import inspect

    assert inspect.signature(PopulationPPO.__init__).parameters["pbt"].default is None


def _bare_population(P, launch=None):
    """A PopulationPPO that owns nothing: what exploit() checks before it touches a member."""
    pop = object.__new__(PopulationPPO)

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the argument checks come before a member is used")

    pop.members, pop._launch, pop._pop_updater = [Untouchable() for _ in range(P)], launch, Untouchable()
    return pop


def test_exploit_refusals_come_before_anything_is_touched():
    pop = _bare_population(4)
    for src_of, shift in (([0, 0, 3], None),                       # a wrong length
                          ([0, 0, 3, 3], [0.0] * 3),
                          ([0, 4, 2, 3], None), ([0, -1, 2, 3], None),  # outside [0, P)
                          ([1, 2, 2, 3], None),                    # member 1 is a source and a destination
                          ([1, 0, 2, 3], None),                    # a swap
                          ([0, 0, 3, 3], [0.0, float("nan"), 0.0, 0.0]), ([0, 0, 3, 3], [0.0, 0.0, float("inf"), 0.0])):
        with pytest.raises(ValueError):
            pop.exploit(src_of, shift)
    with pytest.raises(ValueError, match="hyper"):
        pop.exploit([0, 0, 3, 3], None, hyper={1: dict(gamma=0.9)})
    with pytest.raises(ValueError, match="hyper"):
        pop.exploit([0, 0, 3, 3], None, hyper={7: dict(clip=0.1)})
    with pytest.raises(RuntimeError, match="train"):
        _bare_population(4, launch=dict()).exploit([0, 0, 3, 3])
    assert check_exploit(4, (0, 0, 3, 3)) == ([0, 0, 3, 3], [0.0] * 4)


def test_the_exploit_kernel_shares_the_gather_of_qr_ppo_pack():
    from optimal_quad_control_rl_amd import build, ppo

    assert callable(ppo.MfmaPpoPopulationUpdater.exploit)
    text = open(os.path.join(build.CSRC, "quadrace_ppo_population.hip")).read()
    assert re.search(r"__global__[^;{]*\bppo_population_exploit_kernel\b", text)
    # one gather for qr_ppo_pack and for the exploit kernel: the images cannot drift apart
    assert "pack_gather<L>" in text and "pack_gather<L>" in open(os.path.join(build.CSRC, "quadrace_ppo.hip")).read()


def test_tool_flags():
    import importlib.util

    spec = importlib.util.spec_from_file_location("train_population", os.path.join(ROOT, "tools", "train_population.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parser().parse_args(["--seeds", "0-3"])
    assert a.pbt_interval == 0                                     # off unless asked for
    a = tool.parser().parse_args(["--seeds", "0-3", "--pbt-interval", "10", "--pbt-quantile", "0.5", "--pbt-fitness", "gates",
                                  "--pbt-perturb-lr", "0.8,1.25", "--pbt-log-std-shift", "0.1"])
    assert (a.pbt_interval, a.pbt_quantile, a.pbt_fitness, a.pbt_perturb_lr, a.pbt_log_std_shift) == (10, 0.5, "gates", "0.8,1.25", 0.1)
    assert math.isclose(a.pbt_log_std_shift, 0.1)
