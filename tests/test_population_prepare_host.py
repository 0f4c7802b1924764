"""CPU: the device-side prepare of a population round (qr_ppo_population_load_bank, qr_policy_bank_read, qr_ppo_population_prepare) exists
at every layer -- header, library, ctypes table, build, package, tool -- without an ABI bump; the two structs of _lib.py have the header's
field order and layout; the Python-side refusals come before anything touches a GPU."""
import ctypes as C
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = {
    "qr_ppo_population_load_bank": (["pop", "theta_dev", "bank", "first_slot", "stream"],
                                    ["qr_ppo_population *", "const float * const *", "qr_policy_bank *", "int32_t", "void *"]),
    "qr_policy_bank_read": (["bank", "slot", "which", "out_host", "bytes"], ["const qr_policy_bank *", "int32_t", "int32_t", "void *", "size_t"]),
    "qr_ppo_population_prepare": (["pop", "sh", "members", "report_host", "stream"],
                                  ["qr_ppo_population *", "const qr_ppo_prepare_shared *", "const qr_ppo_prepare_member *", "double *", "void *"]),
}
SHARED_FIELDS = [("int32_t", ["K", "N", "E"]), ("const float *", ["obs", "act", "logp", "rew"]), ("const uint8_t *", ["done", "trunc"]),
                 ("const float *", ["last_obs"]), ("const float *", ["term_obs"])]
MEMBER_FIELDS = [("int32_t", ["first_env"]), ("float", ["gamma", "lam"]), ("float *", ["obs", "act", "old_logp", "rew", "done", "val"]),
                 ("float *", ["term_val"]), ("float *", ["last_val"]), ("float *", ["adv", "ret"]), ("float *", ["ep_ret", "ep_len", "ep_gates"])]


def _header():
    hdr = open(os.path.join(ROOT, "include", "quadrace.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def _declaration(code, name):
    m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, code)
    assert m, "include/quadrace.h does not declare %s" % name
    parts = [a.replace("*", " * ").split() for a in m.group(1).split(",")]
    return [p[-1] for p in parts], [" ".join(p[:-1]) for p in parts]


def _struct_fields(code, name):
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, code)
    assert body, "include/quadrace.h does not define %s" % name
    declared = []
    for stmt in body.group(1).split(";"):
        if stmt.strip():
            base = re.match(r"\s*((?:const\s+)?\w+)", stmt)
            for item in stmt[base.end():].split(","):
                item = item.strip()
                declared.append((base.group(1) + (" *" if item.startswith("*") else ""), item.lstrip("* ")))
    return declared


def test_entry_points_are_declared_exported_bound_and_built():
    from optimal_quad_control_rl_amd import _lib, build

    hdr, code = _header()
    assert re.search(r"#define\s+QR_ABI_VERSION\s+3\b", code)
    version_comment = hdr.split("#define QR_ABI_VERSION")[1].split("*/")[0]
    for name in ENTRY_POINTS:
        assert name in version_comment, name                                                  # the version comment names it
    contract = hdr.split("typedef struct {   /* the ONE collect launch's outputs")[0].rsplit("/*", 1)[1]
    for word in ("CONTRACT", "bit for bit", "Refused before anything is launched", "captured", "ONE blocking", "qr_policy_bank_set", "no atomic"):
        assert word in contract, word
    build.build_native()
    L = C.CDLL(build.LIB)
    exports = open(os.path.join(build.CSRC, "exports.map")).read()
    assert "qr_*;" in exports
    ctype_of = {"int32_t": C.c_int32, "void *": C.c_void_p, "size_t": C.c_size_t, "double *": C.POINTER(C.c_double),
                "qr_ppo_population *": C.c_void_p, "qr_policy_bank *": C.c_void_p, "const qr_policy_bank *": C.c_void_p,
                "const float * const *": C.POINTER(C.c_void_p), "const qr_ppo_prepare_shared *": C.POINTER(_lib.QrPpoPrepareShared),
                "const qr_ppo_prepare_member *": C.POINTER(_lib.QrPpoPrepareMember)}
    for name, (args, types_) in ENTRY_POINTS.items():
        assert _declaration(code, name) == (args, types_), name
        assert hasattr(L, name), "libquadrace.so does not export %s" % name
        rt, at = _lib.SIGNATURES[name]
        assert rt is C.c_int and at == [ctype_of[t] for t in types_], name
        assert name in _lib.OPTIONAL_SYMBOLS
    assert _lib.load().qr_abi_version() == 3
    # a translation unit of its own with the default flags, through the same rewrite and lint
    src = "quadrace_population_prepare.hip"
    assert src in build.SOURCES and os.path.exists(os.path.join(build.CSRC, src))
    assert src not in build.PER_SOURCE_FLAGS and src not in build.NO_VGPR_FORM


def test_structs_match_the_header():
    from optimal_quad_control_rl_amd import _lib

    _, code = _header()
    for cname, expected, ctype in (("qr_ppo_prepare_shared", SHARED_FIELDS, _lib.QrPpoPrepareShared),
                                   ("qr_ppo_prepare_member", MEMBER_FIELDS, _lib.QrPpoPrepareMember)):
        declared = _struct_fields(code, cname)
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


def _stub_env(n):
    def touched(*a, **k):
        raise AssertionError("the argument checks come before the env is used")

    return types.SimpleNamespace(num_envs=n, state_len=24, device=None, VARIANT=0, reset_device=touched, condition_reset=touched,
                                 set_terminal_obs_buffer=touched)


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
