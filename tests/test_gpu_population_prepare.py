"""GPU: the device-side prepare of a population round (csrc/quadrace_population_prepare.hip) against what it replaces.

Bank load (qr_ppo_population_load_bank) against qr_policy_bank_set, image by image through qr_policy_bank_read.  Prepare
(qr_ppo_population_prepare) against the composition of the existing calls, built here: slices .contiguous(), qr_ppo_forward(net 1), the torch
lines of ppo.PPO._sanitise_buffers / _train_prepare and qr_ppo_gae.  No tolerance on tensors: int32 views are compared, so NaN and -0.0
count.  The report's counts are exact; its sums are compared with a NumPy restatement that forms the float32 per-step terms as the kernel
does and adds them in float64, within n * 2^-52 * sum |terms| (n terms): the bound for re-ordering a double sum.

A note on the planted 3e38 rows of last_obs / term_obs: the forward saturates its inputs and activations to the f16 range, so with finite
weights these values come out finite; the nan_to_num of last_val / term_val is reached through a member whose value net carries an
infinite output bias (every one of its values is +inf, so every one of its rows is zeroed).

Shapes: the older cases give every workgroup of the value and the gather launch one tile.  test_prepare_with_many_tiles_per_workgroup flies
the two shapes of test_population_prepare_host.MANY_TILE_SHAPES (P = 256 and E = 512), where a workgroup walks rollout, last_obs and
term_obs tiles in turn and gathers three tiles, with plants in tiles it reaches late; every obs_len of dispatch_L is run once by the bank
load and once by the prepare."""
import ctypes as C
import math
import statistics
import time

import numpy as np
import pytest
import torch

from test_population_prepare_host import MANY_TILE_SHAPES, _stub_env, batched_prepare_refusals, late_plants, prepare_grids

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
OBS_LENS = (24, 17, 16, 13, 20, 21, 25, 28, 29, 32, 36)     # every length dispatch_L instantiates
GAMMA = (0.999, 0.99, 0.95, 0.9)
LAM = (0.95, 0.9, 1.0, 0.8)
H = 120


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()))


def _members(L, P, max_b=256):
    from optimal_quad_control_rl_amd.ppo import ActorCritic, MfmaPpoPopulationUpdater, MfmaPpoUpdater

    ups = []
    for p in range(P):
        torch.manual_seed(40 + p)
        policy = ActorCritic(L, 4).to(DEV)
        ups.append(MfmaPpoUpdater(policy, L, DEV, max_b))
        ups[-1].policy = policy     # its parameters are views of the updater's theta
    return ups, MfmaPpoPopulationUpdater(ups)


def _close(ups, pop, *more):
    pop.close()
    for u in ups:
        u.close()
    for m in more:
        m.close()


def _image_bytes(L):
    return (4 * ((L + 1 + 15) // 16) * 64 + 2 * 4 * 8 * 64 + 8 * 64) * 16


def _read(lib, bank, slot, which, L):
    out = np.zeros(_image_bytes(L) // 2, dtype=np.uint16)
    rc = lib.qr_policy_bank_read(bank._h, slot, which, out.ctypes.data_as(C.c_void_p), out.nbytes)
    return rc, out


# ------------------------------------------------------------------------------------------------------------------------ bank load
def _plant(theta, L):
    """weights at the edges of f16 in the actor block (layout of qr_ppo_num_params: w1, b1, w2, b2, w3, b3, w4, b4)"""
    w2, b2 = H * L + H, H * L + H + H * H
    w3 = b2 + H
    w4 = w3 + H * H + H
    with torch.no_grad():
        theta[5], theta[6] = 70000.0, -70000.0          # beyond f16
        theta[w2 + 7], theta[w2 + 8] = 65504.0, 65520.0  # the rounding boundary
        theta[w3 + 3], theta[w3 + 4] = 6e-8, 1e-9        # f16 subnormal, then underflow
        theta[w4 + 1] = -0.0
        theta[b2 + 9] = math.nan


@pytest.mark.parametrize("L", OBS_LENS)
def test_bank_load_equals_bank_set(L):
    from optimal_quad_control_rl_amd import _lib
    from optimal_quad_control_rl_amd.policy import MfmaPolicyBank

    ups, pop = _members(L, 3)
    lib = ups[0]._L
    _plant(ups[1].theta, L)
    ref, got, wide = MfmaPolicyBank(L, 3, 0), MfmaPolicyBank(L, 3, 0), MfmaPolicyBank(L, 6, 0)
    for p, u in enumerate(ups):
        ref.load_torch(p, u.policy.pi)     # qr_policy_bank_set with the eight arrays theta holds (the planted ones included)
    pop.load_bank(got)
    pop.load_bank(wide, first_slot=2)
    for p in range(3):
        for which in (0, 1):
            rc_r, r = _read(lib, ref, p, which, L)
            rc_g, g = _read(lib, got, p, which, L)
            rc_w, w = _read(lib, wide, 2 + p, which, L)
            assert rc_r == rc_g == rc_w == _lib.QR_OK
            assert np.array_equal(r, g), (p, which, int((r != g).sum()))
            assert np.array_equal(r, w), (p, which, int((r != w).sum()))
    planted = _read(lib, got, 1, 0, L)[1]
    assert (planted == 0x7C00).any() and (planted == 0xFC00).any() and (planted == 0x7E00).any() and (planted == 0x0001).any()
    for slot in (0, 1, 5):   # never loaded: still unset
        assert _read(lib, wide, slot, 0, L)[0] == _lib.QR_E_INVALID
    # read-back refusals
    buf = np.zeros(_image_bytes(L) // 2, dtype=np.uint16)
    assert lib.qr_policy_bank_read(wide._h, 2, 0, buf.ctypes.data_as(C.c_void_p), buf.nbytes - 16) == _lib.QR_E_INVALID
    assert lib.qr_policy_bank_read(wide._h, 2, 2, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == _lib.QR_E_INVALID
    assert lib.qr_policy_bank_read(wide._h, 6, 0, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == _lib.QR_E_INVALID
    # load refusals leave a set slot as it was
    before = [_read(lib, wide, 2, which, L)[1] for which in (0, 1)]
    with torch.no_grad():
        ups[0].theta[:1000] += 1.0     # a load that went through would be seen
    other = MfmaPolicyBank(20 if L != 20 else 24, 6, 0)
    thetas = lambda edit=None: (C.c_void_p * 3)(*[None if edit == p else u.theta.data_ptr() for p, u in enumerate(ups)])
    st = pop._stream()
    for what, rc in (("NULL entry", lib.qr_ppo_population_load_bank(pop._h, thetas(1), wide._h, 2, st)),
                     ("NULL theta_dev", lib.qr_ppo_population_load_bank(pop._h, None, wide._h, 2, st)),
                     ("NULL bank", lib.qr_ppo_population_load_bank(pop._h, thetas(), None, 2, st)),
                     ("NULL pop", lib.qr_ppo_population_load_bank(None, thetas(), wide._h, 2, st)),
                     ("first_slot < 0", lib.qr_ppo_population_load_bank(pop._h, thetas(), wide._h, -1, st)),
                     ("first_slot + P > capacity", lib.qr_ppo_population_load_bank(pop._h, thetas(), wide._h, 4, st)),
                     ("another obs_len", lib.qr_ppo_population_load_bank(pop._h, thetas(), other._h, 0, st))):
        assert rc == _lib.QR_E_INVALID and len(lib.qr_last_error()) > 0, what
    for which in (0, 1):
        assert np.array_equal(before[which], _read(lib, wide, 2, which, L)[1]), which
    assert _read(lib, wide, 5, 0, L)[0] == _lib.QR_E_INVALID and _read(lib, other, 0, 0, 20 if L != 20 else 24)[0] == _lib.QR_E_INVALID
    _close(ups, pop, ref, got, wide, other)


@pytest.fixture(scope="module")
def members_256():
    """256 members of obs_len 13 and their population object, made once for the tests that need the largest population"""
    t0 = time.perf_counter()
    ups, pop = _members(13, 256)
    torch.cuda.synchronize()
    print("256 members and their population object: %.2f s" % (time.perf_counter() - t0))
    yield ups, pop
    _close(ups, pop)


def test_bank_load_of_256_members_behind_a_first_slot(members_256):
    """the 2 KB of parameter-vector pointers in the kernel arguments and blockIdx.y up to 255, into slots 37 .. 292 of a 300-slot bank"""
    from optimal_quad_control_rl_amd import _lib
    from optimal_quad_control_rl_amd.policy import MfmaPolicyBank

    L, P, first = 13, 256, 37
    ups, pop = members_256
    lib = ups[0]._L
    kept = ups[200].theta.clone()
    _plant(ups[200].theta, L)
    ref, got = MfmaPolicyBank(L, P, 0), MfmaPolicyBank(L, 300, 0)
    for p, u in enumerate(ups):
        ref.load_torch(p, u.policy.pi)
    pop.load_bank(got, first_slot=first)
    images = {}
    for p in range(P):
        for which in (0, 1):
            (rc_r, r), (rc_g, g) = _read(lib, ref, p, which, L), _read(lib, got, first + p, which, L)
            assert rc_r == rc_g == _lib.QR_OK
            assert np.array_equal(r, g), (p, which, int((r != g).sum()))
            images[p] = images.get(p, b"") + g.tobytes()
    assert len(set(images.values())) == P                                   # 256 different members: a slot filled from another member fails above
    planted = _read(lib, got, first + 200, 0, L)[1]
    assert (planted == 0x7C00).any() and (planted == 0xFC00).any() and (planted == 0x7E00).any() and (planted == 0x0001).any()
    for slot in (0, first - 1, first + P, 299):                             # outside [first, first + P): still unset
        assert _read(lib, got, slot, 0, L)[0] == _lib.QR_E_INVALID
    with torch.no_grad():
        ups[200].theta.copy_(kept)                                          # the members are shared with other tests of this module
    ref.close(); got.close()


# --------------------------------------------------------------------------------------------------------------------------- prepare
class _Case:
    """Synthetic outputs of one collect launch and P members on it."""

    def __init__(self, L, N, E, K, firsts, term_obs=True, no_term_member=None, inf_value_member=None, seed=0, members=None, on_device=False,
                 late=None):
        """members: (ups, pop) made elsewhere (and closed there); on_device: the big arrays come from a seeded generator on the GPU (the
        CPU's randn dominates the time of the large cases); late: test_population_prepare_host.late_plants(P, E, K)"""
        self.L, self.N, self.E, self.K, self.firsts = L, N, E, K, list(firsts)
        P = len(firsts)
        self.own_members = members is None
        self.ups, self.pop = _members(L, P) if members is None else members
        if inf_value_member is not None:     # the value net's output bias: the last parameter before log_std
            with torch.no_grad():
                self.ups[inf_value_member].theta[-5] = math.inf
            self.ups[inf_value_member].pack()
        g = torch.Generator(device="cpu").manual_seed(1234 + seed)
        if on_device:
            gd = torch.Generator(device=DEV).manual_seed(1234 + seed)
            r = lambda *s: torch.randn(s, generator=gd, device=DEV)
            u = lambda *s: torch.rand(s, generator=gd, device=DEV)
        else:
            r = lambda *s: torch.randn(s, generator=g)
            u = lambda *s: torch.rand(s, generator=g)
        obs, act, logp, rew = r(K, N, L), r(K, N, 4), r(K, N), 3.0 * r(K, N)
        done = u(K, N) < 0.125
        done[0, ::5] = True
        done[K - 1, 1::7] = True
        trunc = done & (u(K, N) < 0.5)
        last_obs, term = r(N, L), r(K, N, L)
        f = self.firsts
        t1 = min(1, K - 1)
        obs[t1, f[0] + 3, 2] = math.nan                       # one plant per member (round robin when P < 4)
        act[K - 1, f[1 % P] + 7, 1] = math.inf
        logp[0, f[2 % P] + 9] = -math.inf
        rew[t1, f[3 % P] + 11] = math.nan
        last_obs[f[0] + 5] = 3e38
        trunc[t1, f[0] + 13] = done[t1, f[0] + 13] = True
        term[t1, f[0] + 13] = 3e38                            # a truncated row
        if late is not None:                                  # plants a workgroup meets on its second or a later tile
            ga, te, la = late["gather"], late["term"], late["last"]
            (t, c), fm = ga["tile"], f[ga["member"]]
            obs[t, fm + c * 256 + ga["obs_row"], ga["obs_col"]] = math.nan
            act[t, fm + c * 256 + ga["act_row"], ga["act_col"]] = math.inf
            (t, c), fm = te["empty_tile"], f[te["member"]]
            trunc[t, fm + c * 256:fm + (c + 1) * 256] = False  # done stays: an episode end that is no time limit
            (t, c) = te["tile"]
            row = fm + c * 256 + te["row"]
            trunc[t, row] = done[t, row] = True
            term[t, row] = 3e38
            last_obs[f[la["member"]] + la["row"]] = 3e38
        term[~trunc] = math.nan                               # must not leak
        self.shared = dict(E=E, obs=obs.to(DEV), act=act.to(DEV), logp=logp.to(DEV), rew=rew.to(DEV), done=done.to(torch.uint8).to(DEV),
                           trunc=trunc.to(torch.uint8).to(DEV), last_obs=last_obs.to(DEV), term_obs=term.to(DEV) if term_obs else None)
        self.with_term = [term_obs and p != no_term_member for p in range(P)]
        self.ep0 = [(torch.rand(E, generator=g).to(DEV) * 4.0, torch.randint(0, 30, (E,), generator=g).float().to(DEV),
                     torch.randint(0, 3, (E,), generator=g).float().to(DEV)) for _ in range(P)]
        self.hyper = [(GAMMA[p % 4], LAM[p % 4]) for p in range(P)]

    def member_args(self, sentinel=7.0):
        K, E, L = self.K, self.E, self.L
        full = lambda *s: torch.full(s, sentinel, dtype=torch.float32, device=DEV)
        args = []
        for p, f in enumerate(self.firsts):
            er, el, eg = (t.clone() for t in self.ep0[p])
            args.append(dict(first_env=f, gamma=self.hyper[p][0], lam=self.hyper[p][1], obs=full(K, E, L), act=full(K, E, 4), old_logp=full(K, E),
                             rew=full(K, E), done=full(K, E), val=full(K, E), term_val=full(K, E) if self.with_term[p] else None, last_val=full(E),
                             adv=full(K, E), ret=full(K, E), ep_ret=er, ep_len=el, ep_gates=eg))
        return args

    def composition(self, p):
        """member p through the existing calls, as ppo.PPO.collect_fused + _train_prepare compose them"""
        K, E, L, sh, up = self.K, self.E, self.L, self.shared, self.ups[p]
        sl = slice(self.firsts[p], self.firsts[p] + E)
        obs, act, lp, rew = (sh[k][:, sl].contiguous() for k in ("obs", "act", "logp", "rew"))
        done = sh["done"][:, sl].contiguous().to(torch.float32)
        trunc = sh["trunc"][:, sl].contiguous()
        value = lambda o: up.forward(1, o.contiguous()).contiguous()
        term_val = None
        if self.with_term[p]:
            term_val = torch.zeros((K, E), dtype=torch.float32, device=DEV)
            rows = trunc.view(-1).nonzero().squeeze(1)
            if rows.numel():
                term_val.view(-1)[rows] = value(sh["term_obs"][:, sl].contiguous().view(K * E, -1)[rows])
        val = value(obs.view(K * E, -1)).view(K, E).clone()
        last_val = value(sh["last_obs"][sl])
        bad = ~(torch.isfinite(obs).all(-1) & torch.isfinite(act).all(-1) & torch.isfinite(lp) & torch.isfinite(rew) & torch.isfinite(val))
        for t in (obs, act, lp, rew, val):
            t[bad] = 0.0
        last_val = torch.nan_to_num(last_val, nan=0.0, posinf=0.0, neginf=0.0)
        if term_val is not None:
            term_val.nan_to_num_(nan=0.0, posinf=0.0, neginf=0.0)
        er, el, eg = (t.clone() for t in self.ep0[p])
        fin = torch.zeros(4, dtype=torch.float32, device=DEV)
        adv, ret = up.gae(rew, done, val, last_val, self.hyper[p][0], self.hyper[p][1], (er, el, eg), fin, term_val=term_val)
        adv = adv.masked_fill(bad, 0.0)
        ret = torch.where(bad, val, ret)
        return dict(obs=obs, act=act, old_logp=lp, rew=rew, done=done, val=val, term_val=term_val, last_val=last_val, adv=adv, ret=ret,
                    ep_ret=er, ep_len=el, ep_gates=eg), bad, trunc

    def report_reference(self, p, comp, bad, trunc):
        """counts, and (sum, bound) of the five sums: float32 per-step terms as the kernel forms them, added in float64"""
        rew, done = comp["rew"].cpu().numpy(), comp["done"].cpu().numpy()
        er, el, eg = (t.cpu().numpy().copy() for t in self.ep0[p])
        terms = [[], [], [], [], []]
        one, zero = np.float32(1.0), np.float32(0.0)
        for t in range(self.K):
            r, d = rew[t], done[t]
            er = er + r
            el = el + one
            eg = eg + np.where(r > np.float32(5.0), one, zero)
            for k, x in enumerate((er * d, el * d, eg * d, d, r)):
                terms[k].append(x.astype(np.float32))
            keep = one - d
            er, el, eg = er * keep, el * keep, eg * keep
        sums = []
        for k in range(5):
            x = np.stack(terms[k]).astype(np.float64)
            sums.append((float(x.sum()), x.size * 2.0 ** -52 * float(np.abs(x).sum())))
        return int(bad.sum()), int(trunc.sum()), sums

    def check(self, where):
        args = self.member_args()
        report = self.pop.prepare(self.shared, args)
        for p in range(len(self.firsts)):
            comp, bad, trunc = self.composition(p)
            for key, want in comp.items():
                if want is None:
                    assert args[p][key] is None
                else:
                    _same(args[p][key], want, (where, "member %d" % p, key))
            n_bad, n_trunc, sums = self.report_reference(p, comp, bad, trunc)
            r = report[p]
            print("%s member %d report %r" % (where, p, r))
            assert r[0] == n_bad and r[1] == n_trunc and r[7] == 0.0, (where, p, r, n_bad, n_trunc)
            for got, (want, bound) in zip((r[2], r[3], r[4], r[5], r[6]), sums):
                assert abs(got - want) <= bound, (where, p, got, want, bound)
            assert r[5] == float(comp["done"].sum())
        return args, report

    def close(self):
        if self.own_members:
            _close(self.ups, self.pop)


def test_prepare_equals_the_composition():
    c = _Case(24, 1024, 256, 5, (512, 0, 256))     # out of order, one group of columns unused
    args, report = c.check("N 1024, E 256, K 5")
    assert report[0][0] >= 2 and sum(r[0] for r in report) >= 4 and all(r[5] > 0 and r[1] > 0 for r in report)
    assert not bool(torch.isnan(args[0]["term_val"]).any())
    # the same call again (episode state put back): the same report, bit for bit
    again = c.member_args()
    report2 = c.pop.prepare(c.shared, again)
    assert [[x.hex() for x in r] for r in report] == [[x.hex() for x in r] for r in report2]
    for p in range(3):
        for key in args[p]:
            if args[p][key] is not None and torch.is_tensor(args[p][key]):
                _same(args[p][key], again[p][key], ("second call", p, key))
    c.close()


@pytest.mark.parametrize("kw", [dict(L=24, N=1024, E=512, K=5, firsts=(512, 0)),                       # two workgroups per member
                                dict(L=24, N=1024, E=256, K=1, firsts=(512, 0, 256)),                  # one step
                                dict(L=24, N=1024, E=256, K=5, firsts=(512, 0, 256), term_obs=False),  # no time-limit bootstrap at all
                                dict(L=24, N=1024, E=256, K=5, firsts=(512, 0, 256), no_term_member=1),
                                dict(L=24, N=512, E=256, K=5, firsts=(256,)),                          # P = 1
                                dict(L=17, N=512, E=256, K=3, firsts=(0, 256)),                        # an obs_len that is no multiple of 4
                                dict(L=24, N=512, E=256, K=4, firsts=(256, 0), inf_value_member=1)],   # every value of one member +inf
                         ids=["E512", "K1", "no_term_obs", "one_member_without_term_val", "P1", "L17", "inf_values"])
def test_prepare_corollaries(kw):
    c = _Case(**kw)
    args, report = c.check(repr(kw))
    if kw.get("inf_value_member") is not None:
        m = args[1]
        assert report[1][0] == c.K * c.E and float(m["val"].abs().sum()) == 0.0 and float(m["last_val"].abs().sum()) == 0.0
        assert float(m["term_val"].abs().sum()) == 0.0 and float(m["adv"].abs().sum()) == 0.0 and report[0][0] < c.K * c.E
    c.close()


@pytest.mark.parametrize("L", OBS_LENS)
def test_prepare_at_every_obs_len(L):
    """every instantiation of dispatch_L: the float4 path (L % 4 == 0) and the scalar one, badrow[(k 256 + tid) / L], the image of each size"""
    c = _Case(L, 512, 256, 3, (256, 0), seed=L)
    _, report = c.check("L %d" % L)
    assert sum(r[0] for r in report) >= 4 and all(r[5] > 0 and r[1] > 0 for r in report)
    c.close()


@pytest.mark.parametrize("shape", MANY_TILE_SHAPES, ids=["P%(P)d-E%(E)d-K%(K)d-L%(L)d" % s for s in MANY_TILE_SHAPES])
def test_prepare_with_many_tiles_per_workgroup(shape, members_256):
    """The tile loops of the value and the gather launch walked several times by one workgroup (the conditions are asserted on the CPU:
    test_population_prepare_host.test_many_tile_shapes_walk_several_tiles_per_workgroup), with non-finite values in tiles a workgroup
    reaches on its second or a later iteration.  The members' columns lie in the shared arrays in reverse order."""
    L, P, E, K = shape["L"], shape["P"], shape["E"], shape["K"]
    g, late = prepare_grids(P, E, K), late_plants(P, E, K)
    firsts = [(P - 1 - p) * E for p in range(P)]
    t0 = time.perf_counter()
    c = _Case(L, P * E, E, K, firsts, members=members_256 if (L, P) == (13, 256) else None, on_device=True, late=late)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    sh = c.shared
    ga, te, la = late["gather"], late["term"], late["last"]
    tile_of = lambda name, m, tc: sh[name][tc[0], firsts[m] + tc[1] * 256:firsts[m] + (tc[1] + 1) * 256]
    # the inputs are what the plan says: a term_obs tile without a truncation before a tile with one, in one workgroup of the value launch
    assert int(tile_of("trunc", te["member"], te["empty_tile"]).sum()) == 0 and int(tile_of("done", te["member"], te["empty_tile"]).sum()) > 0
    assert int(tile_of("trunc", te["member"], te["tile"])[te["row"]]) == 1
    assert (g["roll"] + g["cpe"] + te["q"][0]) % g["vgrid"] == (g["roll"] + g["cpe"] + te["q"][1]) % g["vgrid"]
    src_next = tile_of("obs", ga["member"], ga["next_tile"]).clone()
    assert bool(torch.isfinite(src_next).all()) and bool(torch.isfinite(tile_of("act", ga["member"], ga["next_tile"])).all())
    args, report = c.check(repr(shape))
    t2 = time.perf_counter()
    print("%r: grids %r, inputs %.2f s, prepare + %d compositions %.2f s" % (shape, g, t1 - t0, P, t2 - t1))
    member_tile = lambda name, m, tc: args[m][name][tc[0], tc[1] * 256:(tc[1] + 1) * 256]
    # gather: exactly the two planted rows of the late tile are zeroed, and the tile the same workgroup does next comes out as it went in
    m = ga["member"]
    bad = member_tile("obs", m, ga["tile"]).eq(0.0).all(-1).nonzero().flatten().tolist()
    assert bad == sorted((ga["obs_row"], ga["act_row"])), bad
    assert float(member_tile("act", m, ga["tile"])[bad].abs().sum()) == 0.0 and float(member_tile("adv", m, ga["tile"])[bad].abs().sum()) == 0.0
    _same(member_tile("obs", m, ga["next_tile"]), src_next, "the clean tile after the planted one")
    assert int(member_tile("obs", m, ga["next_tile"]).eq(0.0).all(-1).sum()) == 0
    assert report[m][0] == 2.0                                      # the member's non-finite rows: the two late plants and nothing else
    # term: the tile without a truncation is all zero, the planted row of the next one was evaluated
    m = te["member"]
    assert float(member_tile("term_val", m, te["empty_tile"]).abs().sum()) == 0.0
    v = float(member_tile("term_val", m, te["tile"])[te["row"]])
    assert math.isfinite(v) and v != 0.0
    # last_obs: the planted row of a member other than member 0 went through the saturating forward
    m = la["member"]
    assert m != 0 and float(sh["last_obs"][firsts[m] + la["row"], 0]) > 1e38 and math.isfinite(float(args[m]["last_val"][la["row"]]))
    assert all(r[5] > 0 and r[1] > 0 for r in report)
    c.close()


def test_prepare_again_with_another_K_regrows_the_scratch():
    c = _Case(24, 512, 256, 2, (256, 0))
    c.check("K 2")
    pop, ups = c.pop, c.ups
    d = _Case(24, 512, 256, 9, (256, 0), seed=1)
    d.pop.close()
    for u in d.ups:
        u.close()
    d.pop, d.ups = pop, ups     # the SAME population object, a longer rollout
    d.check("K 9 on the same object")
    c.check("K 2 again")
    c.close()


def test_prepare_refusals_launch_nothing():
    from optimal_quad_control_rl_amd import _lib

    c = _Case(24, 1024, 256, 3, (512, 0, 256))
    lib, pop, sh_t = c.ups[0]._L, c.pop, c.shared
    args_t = c.member_args(sentinel=-3.0)
    tensors = [t for a in args_t for t in a.values() if torch.is_tensor(t)]
    before = [t.clone() for t in tensors]
    report = (C.c_double * 24)(*([123.0] * 24))

    def call(edit_sh=None, edit_m=None, pop_h=pop._h, null=None, stream=None):
        sh = _lib.QrPpoPrepareShared()
        sh.K, sh.N, sh.E = c.K, c.N, c.E
        for name in ("obs", "act", "logp", "rew", "done", "trunc", "last_obs", "term_obs"):
            setattr(sh, name, sh_t[name].data_ptr())
        args = (_lib.QrPpoPrepareMember * 3)()
        for a, m in zip(args, args_t):
            a.first_env, a.gamma, a.lam = m["first_env"], m["gamma"], m["lam"]
            for name, t in m.items():
                if torch.is_tensor(t):
                    setattr(a, name, t.data_ptr())
        if edit_sh:
            edit_sh(sh)
        if edit_m:
            edit_m(args)
        return lib.qr_ppo_population_prepare(pop_h, None if null == "sh" else C.byref(sh), None if null == "members" else args,
                                             None if null == "report" else report, pop._stream() if stream is None else stream)

    def refused(rc, what):
        assert rc == _lib.QR_E_INVALID, (what, rc)
        assert len(lib.qr_last_error()) > 0, what
        torch.cuda.synchronize()
        for t, b in zip(tensors, before):
            assert torch.equal(t, b), what
        assert all(x == 123.0 for x in report), what

    def set_(obj, **kw):
        for k, v in kw.items():
            setattr(obj, k, v)

    refused(call(pop_h=None), "NULL pop")
    for null in ("sh", "members", "report"):
        refused(call(null=null), "NULL " + null)
    refused(call(edit_sh=lambda s: set_(s, K=0)), "K < 1")
    refused(call(edit_sh=lambda s: set_(s, E=128)), "E < 256")
    refused(call(edit_sh=lambda s: set_(s, E=384)), "E % 256")
    refused(call(edit_sh=lambda s: set_(s, E=768)), "N % E")
    refused(call(edit_m=lambda a: set_(a[1], first_env=128)), "first_env not a multiple of E")
    refused(call(edit_m=lambda a: set_(a[1], first_env=1024)), "first_env beyond N")
    refused(call(edit_m=lambda a: set_(a[1], first_env=-256)), "first_env negative")
    refused(call(edit_m=lambda a: set_(a[2], first_env=512)), "two members with one first_env")
    for field in ("obs", "act", "old_logp", "rew", "done", "val", "last_val", "adv", "ret"):
        refused(call(edit_m=lambda a, f=field: set_(a[2], **{f: None})), "NULL " + field)
    refused(call(edit_m=lambda a: set_(a[0], ep_len=None)), "ep_* in part")
    refused(call(edit_m=lambda a: set_(a[0], ep_ret=None, ep_gates=None)), "ep_* in part")
    refused(call(edit_sh=lambda s: set_(s, term_obs=None)), "term_val without term_obs")
    refused(call(edit_m=lambda a: set_(a[1], gamma=math.nan)), "NaN gamma")
    refused(call(edit_m=lambda a: set_(a[1], lam=math.inf)), "inf lam")
    side = torch.cuda.Stream(DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="relaxed"):
        rc = call(stream=C.c_void_p(side.cuda_stream))
    refused(rc, "a stream that is being captured")
    del graph
    # ... and the valid call runs: term_val and the three ep_* may be NULL
    assert call(edit_m=lambda a: (set_(a[1], term_val=None), set_(a[2], ep_ret=None, ep_len=None, ep_gates=None))) == _lib.QR_OK
    assert float(args_t[0]["val"][0, 0]) != -3.0 and report[7] == 0.0 and report[16 + 5] == 0.0
    c.close()


# --------------------------------------------------------------------------------------------------------------------------- trainer
def _trainer_env(n, max_steps):
    from optimal_quad_control_rl_amd.conditions import Condition
    from test_gpu_rollout_conditions import _conditions, _handle

    c = _conditions("e2e")[0]
    return _handle("e2e", n, 1, Condition(c.name, c.gate_pos, c.gate_yaw, c.start_pos, c.disturbance_ranges, c.disturbance_scale, max_steps,
                                          c.gates_per_lap), seed=21)


EPISODE_STATS = ("ep_rew_mean", "ep_len_mean", "gates_per_episode", "reward_per_step")


def _same_population(x, y, where):
    lib = x.members[0]._updater._L
    L = x.env.state_len
    for p, (a, b) in enumerate(zip(x.members, y.members)):
        for name in ("theta", "m", "v"):
            _same(getattr(a._updater, name), getattr(b._updater, name), (where, p, name))
        assert a._updater.step == b._updater.step and a._updater.shuffle_state() == b._updater.shuffle_state(), (where, p)
        assert a._updater.status() == b._updater.status(), (where, p)
        for name in ("buf_obs", "buf_act", "buf_lp", "buf_rew", "buf_val", "buf_done", "buf_term_val", "last_val", "ep_ret", "ep_len", "ep_gates"):
            s, t = getattr(a, name), getattr(b, name)
            assert (s is None) == (t is None), (where, p, name)
            if s is not None:
                _same(s, t, (where, p, name))
        for k in (0, 1):
            _same(a._adv_ret[k], b._adv_ret[k], (where, p, "adv / ret", k))
        assert (a.num_timesteps, a.noise_step) == (b.num_timesteps, b.noise_step), (where, p)
        assert set(a.stats) == set(b.stats), (where, p, sorted(a.stats), sorted(b.stats))
        for key in a.stats:
            if key in EPISODE_STATS:   # the sequential side sums its finished episodes with float atomics: order-dependent
                assert a.stats[key] == pytest.approx(b.stats[key], rel=1e-5), (where, p, key, a.stats[key], b.stats[key])
            else:
                assert a.stats[key] == b.stats[key], (where, p, key, a.stats[key], b.stats[key])
        for which in (0, 1):
            (rc_a, ia), (rc_b, ib) = _read(lib, x.bank, p, which, L), _read(lib, y.bank, p, which, L)
            assert rc_a == rc_b == 0 and np.array_equal(ia, ib), (where, p, "bank image", which)
    for s, t in zip(x.env.get_state_tensors(), y.env.get_state_tensors()):
        assert (s is None) == (t is None)
        if s is not None:
            assert torch.equal(s, t), (where, "env state")


def test_population_ppo_batched_prepare_equals_the_members_own_prepare():
    from optimal_quad_control_rl_amd import PopulationPPO

    E = 256
    shared = dict(n_steps=16, batch_size=1024, n_epochs=2, native_update=True, batched_update=True)
    kw = [dict(seed=3, learning_rate=3e-4), dict(seed=4, learning_rate=1e-3, target_kl=1e-4),
          dict(seed=5, learning_rate=1e-3, ent_coef=0.01, gamma=0.99, gae_lambda=0.9, truncation_bootstrap=False)]
    envs = [_trainer_env(3 * E, 10) for _ in range(4)]      # a time limit of 10 steps: truncations and resets inside every round
    seq = PopulationPPO(envs[0], kw, envs_per_member=E, **shared)
    bat = PopulationPPO(envs[1], kw, envs_per_member=E, batched_prepare=True, **shared)
    loads = []
    for m in bat.members:   # the members' own MfmaPolicy is not loaded on this path
        m._mfma.load_torch = lambda *a, **k: loads.append(1)
    for r in range(3):
        for q in (seq, bat):
            q.collect()
            q.train()
        _same_population(seq, bat, "round %d" % r)
        print("round %d: truncations %s, episodes %s, updates %s, early stop %s" % (
            r, [m.stats.get("truncations") for m in bat.members], [m.stats.get("episodes") for m in bat.members],
            [m.stats["updates"] for m in bat.members], [m.stats.get("early_stop") for m in bat.members]))
        assert all(m.stats["truncations"] > 0 for m in bat.members[:2]) and all(m.stats["episodes"] > 0 for m in bat.members)
    assert not loads and "truncations" not in bat.members[2].stats
    # a state_dict of one kind loads into the other and the next round is equal again
    seq2 = PopulationPPO(envs[2], kw, envs_per_member=E, **shared).load_state_dict(bat.state_dict())
    bat2 = PopulationPPO(envs[3], kw, envs_per_member=E, batched_prepare=True, **shared).load_state_dict(seq.state_dict())
    for q in (seq, bat, seq2, bat2):
        q.collect()
        q.train()
    _same_population(seq, bat, "round 3")
    _same_population(seq, seq2, "prepared checkpoint -> sequential prepare")
    _same_population(seq, bat2, "sequential checkpoint -> batched prepare")
    for q in (seq, bat, seq2, bat2):
        q.close()
    for e in envs:
        e.close()
    batched_prepare_refusals(_stub_env)     # the ValueError cases of the constructor, on an env that must not be touched


def test_batched_prepare_round_is_no_slower():
    """P = 8 x 256 envs, n_steps 256 (65 536 rows per member, four minibatches, one epoch).  A round = collect() + train(); the two kinds
    alternate on envs of their own, one warm-up round each, medians of 7, host clock around a stream synchronise.  The feature exists to be
    faster than what it replaces: batched_prepare=True <= batched_prepare=False is a condition."""
    from optimal_quad_control_rl_amd import PopulationPPO

    P, E = 8, 256
    shared = dict(n_steps=256, batch_size=16384, n_epochs=1, native_update=True, batched_update=True)
    kw = [dict(seed=s) for s in range(P)]
    envs = [_trainer_env(P * E, 250) for _ in range(2)]
    old = PopulationPPO(envs[0], kw, envs_per_member=E, **shared)
    new = PopulationPPO(envs[1], kw, envs_per_member=E, batched_prepare=True, **shared)

    def timed(q):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        q.collect()
        q.train()
        torch.cuda.current_stream(DEV).synchronize()
        return (time.perf_counter() - t0) * 1e3

    timed(new); timed(old)
    tn, to = [], []
    for _ in range(7):
        tn.append(timed(new))
        to.append(timed(old))
    a, b = statistics.median(tn), statistics.median(to)
    print("round with batched_prepare %.3f ms, without %.3f ms, ratio %.3f (P = 8, 256 envs, n_steps 256)" % (a, b, a / b))
    for q in (old, new):
        q.close()
    for e in envs:
        e.close()
    assert a <= 1.0 * b, (a, b)
