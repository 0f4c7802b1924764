"""CPU suite: the edge-case tables of tests/q3_edge_cases.py through the oracle alone (oracle/quad3d_oracle.c).

The GPU suite (tests/test_gpu_q3_edges.py) demands that the HIP kernels agree with the oracle on these rows.  That says something only
if the rows are what they claim to be: the row ON a threshold and its neighbours one ulp to either side must end differently, every
override combination must produce the reward and the end cause it was built for, the generated tracks must make a wrong gate row give a
wrong answer.  Those conditions are checked here, without a GPU."""
import numpy as np
import pytest

import q3_edge_cases as ec
import q3_eval_spec as spec

CAUSES = ("success", "timeout", "oob", "ground", "collision")


# ---- section 1: tracks and the constructed pass table -----------------------------------------------------------------------------------
@pytest.mark.parametrize("G", ec.TRACK_SIZES)
def test_tracks_have_distinct_rows_and_oblique_yaws(G):
    gp, gy, sp = ec.circle_track(G)
    assert gp.shape == (G, 3) and gy.shape == (G,) and gp.dtype == np.float32 and gy.dtype == np.float32
    assert np.hypot(gp[:, 0], gp[:, 1]).max() <= 6.0 and np.all(gp[:, 2] == np.float32(-1.5))
    n0, n1 = ec.gate_normals(gy)         # no normal along an axis: both components carry at least 1 cm per metre of offset
    assert min(np.abs(n0).min(), np.abs(n1).min()) > 0.01
    for a in range(G):
        for b in range(a + 1, G):       # a wrong row must move the gate by more than the window and turn the normal visibly
            assert np.linalg.norm(gp[a] - gp[b]) > 0.7 or abs(gy[a] - gy[b]) > 0.1, (a, b)
            assert not np.array_equal(gp[a], gp[b]) and gy[a] != gy[b]


@pytest.mark.parametrize("G", ec.TRACK_SIZES)
def test_reset_reaches_the_first_and_the_last_segment(G):
    trk = ec.circle_track(G)
    o = ec.oracle_env("gates", 4096, trk, seed=21)
    st = o.reset()
    seg = o.target.copy()
    assert seg.min() == 0 and seg.max() == G - 1
    pts = np.concatenate([trk[2][None], trk[0]])
    mid = (pts[seg] + pts[seg + 1]) / np.float32(2.0)
    for s in (0, G - 1):                # the midpoint of segment s is (points[s] + points[s + 1]) / 2, points = [start, gates...]
        dev = st[seg == s, :3] - mid[seg == s]
        assert np.abs(dev.mean(0)).max() < 0.1 * 5 / np.sqrt((seg == s).sum()) and np.abs(dev).max() < 0.6


@pytest.mark.parametrize("G", ec.TRACK_SIZES)
def test_pass_table_passes_and_collides_at_every_gate(G):
    trk = ec.circle_track(G)
    st, tg, sc, act, passes = ec.pass_table(trk)
    o = ec.oracle_env("gates", 2 * G, trk, seed=3)
    t = ec.oracle_trace(o, st, tg, sc, act[None])
    done, rew, target = t["done"][0], t["rew"][0], t["target"][0]
    last = tg == G - 1
    assert np.array_equal(done, ~passes | last)
    assert np.all(target[passes & ~last] == tg[passes & ~last] + 1)
    assert np.all(rew[passes & last] == 10.0) and np.all(rew[~passes] == -10.0)
    assert not t["trunc"].any()


# ---- section 3: exact thresholds -----------------------------------------------------------------------------------------------------------
def _run_table(t):
    o = ec.oracle_env(t.kind, t.n, t.track, t.thresholds, ec.EDGE_MAX_STEPS, ec.EDGE_DT, seed=9)
    return ec.oracle_trace(o, t.states, t.target if t.kind == "gates" else None, t.steps, t.actions[None])


def _causes(t, tr):
    cls = spec.classify(t.kind, tr["pre_states"][0], tr["pre_steps"][0], tr["rew"][0].astype(np.float32), tr["done"][0], tr["trunc"][0],
                        ec.EDGE_MAX_STEPS)
    out = [None] * t.n
    for name, m in zip(CAUSES, cls):
        for i in np.nonzero(m)[0]:
            assert out[i] is None
            out[i] = name
    return out


@pytest.mark.parametrize("which", ["hover", "hover_wide", "gates"])
def test_every_threshold_row_ends_as_built(which):
    t = ec.threshold_tables()[which]
    tr = _run_table(t)
    done, trunc, rew, target = tr["done"][0], tr["trunc"][0], tr["rew"][0], tr["target"][0]
    causes = _causes(t, tr)
    for i, name in enumerate(t.names):
        assert done[i] == t.done[i] and trunc[i] == t.trunc[i], (name, i, done[i], trunc[i])
        if np.isnan(t.reward[i]):
            assert rew[i] not in (100.0, -1.0, 10.0, -10.0), (name, rew[i])
        else:
            assert rew[i] == t.reward[i], (name, rew[i])
        assert causes[i] == t.cause[i], (name, causes[i])
        if t.kind == "gates" and not done[i]:
            assert target[i] == t.target_after[i], (name, target[i])
    # a row on a threshold and its neighbours: the two sides end differently, and the threshold row differs from at least one of them
    # (the window's edge, crossed and neither inside nor outside, differs from both)
    assert len(t.triples) >= (0 if which == "hover_wide" else 10)
    for name, (lo, on, hi) in t.triples:
        def outcome(i):
            return (bool(done[i]), causes[i], int(target[i]) if (t.kind == "gates" and not done[i]) else None)
        assert outcome(lo) != outcome(hi), name
        differs = [i for i in (lo, hi) if outcome(i) != outcome(on)]
        assert differs, name
        # ... and a neighbour it differs from really is one: the tested column moved by one ulp (or by the few that move x_new by one)
        for other in differs:
            d = t.states[on] != t.states[other]
            assert d.sum() == 1
            col = int(np.nonzero(d)[0][0])
            a, b = t.states[on, col], t.states[other, col]
            assert abs(a - b) <= 16 * np.spacing(max(abs(a), abs(b))), name


def test_every_end_cause_occurs_at_least_twice():
    tabs = ec.threshold_tables()
    hover = tabs["hover"].cause + tabs["hover_wide"].cause
    for c in ("success", "timeout", "oob"):
        assert hover.count(c) >= 2, c
    for c in CAUSES:
        assert tabs["gates"].cause.count(c) >= 2, c
    # the combined rows decide the order of the evaluator's classification and of the reward overrides
    g = tabs["gates"]
    by = {n: i for i, n in enumerate(g.names)}
    assert g.cause[by["collision and ground"]] == "ground" and g.cause[by["final pass and ground"]] == "success"
    assert g.reward[by["final pass and ground"]] == 10.0 and g.cause[by["oob and collision"]] == "oob"
    assert np.isnan(g.reward[by["oob and pass"]]) and g.cause[by["oob and ground"]] == "ground"
    w = tabs["hover_wide"]
    assert w.reward[w.names.index("goal and oob, phi=3.5")] == -1.0


def test_the_crossed_but_neither_rows_keep_their_target():
    t = ec.threshold_tables()["gates"]
    tr = _run_table(t)
    rows = [i for i, n in enumerate(t.names) if n in ("y-gy=+0.5", "y-gy=-0.5", "z-gz=-0.5", "x_new-gx=0.5") and t.steps[i] == 0]
    on = [i for _, (lo, o, hi) in t.triples for i in (o,) if i in rows]
    assert len(on) == 4
    gp = t.track[0]
    for i in on:
        new = tr["states"][0][i, :3] - gp[0]
        assert np.abs(new).max() == np.float32(0.5) and t.states[i, 0] < 0 < new[0]       # crossed the plane, on the window's edge
        assert not tr["done"][0][i] and tr["target"][0][i] == 0


# ---- section 2: thresholds binding -----------------------------------------------------------------------------------------------------------
def test_set_thresholds_reaches_the_oracle():
    z = np.zeros((2, 16))
    z[1, 0] = 0.4
    a = np.zeros((1, 2, 4), np.float32)
    o = ec.oracle_env("hover", 2)
    assert list(ec.oracle_trace(o, z, None, np.zeros(2, np.int32), a)["rew"][0] == 100.0) == [True, False]     # default 0.3
    o = ec.oracle_env("hover", 2, thresholds=(0.5, 1.0, 0.5, 2.0))
    assert list(ec.oracle_trace(o, z, None, np.zeros(2, np.int32), a)["rew"][0] == 100.0) == [True, True]
    o = ec.oracle_env("hover", 2, thresholds=(0.5, 1.0, 0.5, 0.0))
    assert not ec.oracle_trace(o, z, None, np.zeros(2, np.int32), a)["done"].any()


# ---- section 4: non-finite rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hover", "gates"])
def test_nonfinite_table_shape_and_fate(kind):
    trk = ec.circle_track(2) if kind == "gates" else None
    st, tg, sc, act = ec.nonfinite_table(kind, trk)
    n = 16 * 3 + 4 * 3 + 8
    assert st.shape == (n, 16) and act.shape == (n, 4)
    assert (~np.isfinite(st)).sum() == 48 and (~np.isfinite(act)).sum() == 12 and (~np.isfinite(st)).any(axis=1).sum() == 48
    assert np.abs(act[np.isfinite(act).all(axis=1)]).max() == 1e6
    assert tg.min() >= 0 and tg.max() < (2 if kind == "gates" else 1)
    o = ec.oracle_env(kind, n, trk, max_steps=ec.NONFINITE_MAX_STEPS, seed=4)
    t = ec.oracle_trace(o, st, tg if kind == "gates" else None, sc, np.repeat(act[None], 3, axis=0), force_steps=True)
    assert t["done"][2].all() and t["trunc"][2].all() and np.isfinite(t["states"][2]).all()
    nan_rows = np.isnan(t["states"][1]).any(axis=1)
    assert nan_rows.sum() >= 12 and not t["done"][1][nan_rows].any()      # a NaN state persists until max_steps, as upstream


# ---- section 6: episode counter wrap ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hover", "gates"])
def test_episode_counter_wraps_to_zero(kind):
    trk = ec.circle_track(2) if kind == "gates" else None
    n = 6
    o, fresh = ec.oracle_env(kind, n, trk, seed=8), ec.oracle_env(kind, n, trk, seed=8)
    o.episode[:] = np.array([0xFFFFFFFE, 0xFFFFFFFF, 0] * 2, np.uint32)
    o.reset()
    s2 = o.reset()
    assert list(o.episode) == [0, 1, 2] * 2                     # 0xFFFFFFFE -> 0xFFFFFFFF -> 0; 0xFFFFFFFF -> 0 -> 1
    s3 = o.reset()
    f1 = fresh.reset()
    f2 = fresh.reset()
    # the draw is a function of the counter's value: behind the wrap an env repeats what a fresh handle draws at episodes 0 and 1
    assert np.array_equal(s2[1], f1[1]) and np.array_equal(s2[2], f2[2])
    assert np.array_equal(s3[0], f1[0]) and np.array_equal(s3[1], f2[1])
    assert not np.array_equal(s2[0], f1[0]) and not np.array_equal(s2[0], f2[0])
