"""CPU: the population update in the build, the package and the tool (qr_ppo_population_create / _destroy / _epoch / _status
themselves are pinned in tests/abi_table.py); the member-argument struct of _lib.py has the header's layout; the Python-side
refusals come before anything touches a GPU."""
import ctypes as C
import os
import re
import tempfile

import pytest

import abi_decl
from abi_decl import stub_env as _stub_env   # the GPU tests import it from here

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MEMBER_FIELDS = [("float *", ["theta_dev", "adam_m_dev", "adam_v_dev"]),
                 ("const float *", ["obs_dev", "act_dev", "old_logp_dev", "adv_dev", "ret_dev"]),
                 ("int32_t *", ["perm_dev"]),
                 ("float", ["clip", "vf_coef", "ent_coef", "max_grad_norm", "lr", "beta1", "beta2", "eps"]),
                 ("float *", ["stats_dev"])]


def test_member_argument_struct_matches_the_header():
    from optimal_quad_control_rl_amd import _lib

    declared = abi_decl.struct_fields(abi_decl.header()[1], "qr_ppo_member_args")
    assert declared == [(t, n) for t, names in MEMBER_FIELDS for n in names]
    fields = _lib.QrPpoMemberArgs._fields_
    assert [n for n, _ in fields] == [n for _, n in declared]
    for (name, ctype), (ctext, _) in zip(fields, declared):
        assert ctype is (C.c_float if ctext == "float" else C.c_void_p), name
    # the C layout on this ABI: nine pointers, eight floats, one pointer -- no padding anywhere
    assert C.sizeof(_lib.QrPpoMemberArgs) == 9 * 8 + 8 * 4 + 8
    assert _lib.QrPpoMemberArgs.clip.offset == 72 and _lib.QrPpoMemberArgs.eps.offset == 100 and _lib.QrPpoMemberArgs.stats_dev.offset == 104


def test_the_device_table_entry_and_the_kernels_are_where_the_header_says():
    from optimal_quad_control_rl_amd import build

    # a translation unit with the flags quadrace_ppo.hip gets; the shared header is a dependency of the build
    assert "quadrace_ppo.hip" not in build.PER_SOURCE_FLAGS
    assert "quadrace_ppo_device.hpp" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "quadrace_ppo_device.hpp"))
    text = open(os.path.join(build.CSRC, "quadrace_ppo_population.hip")).read()
    for kernel in ("ppo_population_reduce_kernel", "ppo_population_step_kernel", "ppo_population_lr_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\b" % kernel, text), kernel
    # the gradient kernel is the one both PPO units share: a template with a member mode in the shared header, instantiated here
    shared = open(os.path.join(build.CSRC, "quadrace_ppo_device.hpp")).read()
    assert re.search(r"template\s*<[^>]*\bbool kMember\b[^>]*>\s*__global__[^;{]*\bppo_grad_kernel\b", shared)
    code = re.sub(r"//[^\n]*", "", text)
    assert len(re.findall(r"ppo_grad_kernel<L, \w+, true>\), dim3\(wgs, 2, P\)", code)) == 2
    # no inter-workgroup wait of any kind in the new unit
    for word in ("atomic", "s_sleep", "Cooperative", "__threadfence", "arrive", "barrier_timeouts"):
        assert word not in code, word
    assert "dim3(wgs, 2, P)" in code and code.count("dim3(kWorkgroups, P)") == 2


def batched_update_refusals(env_factory):
    """The four ValueError cases of PopulationPPO(batched_update=True); env_factory(n) -> an env of n envs that is never used."""
    import torch.distributed as dist

    from optimal_quad_control_rl_amd.population import PopulationPPO
    from optimal_quad_control_rl_amd.ppo import MfmaPpoUpdater

    two = [dict(seed=3), dict(seed=4, learning_rate=1e-4)]
    ok = dict(n_steps=16, batch_size=1024, n_epochs=2, native_update=True, batched_update=True)
    with pytest.raises(ValueError, match="native_update"):
        PopulationPPO(env_factory(512), two, **{**ok, "native_update": False})
    with pytest.raises(ValueError, match="native_update"):
        PopulationPPO(env_factory(512), [dict(seed=3), dict(seed=4, native_update=False)], **ok)
    with pytest.raises(ValueError, match="f32"):
        PopulationPPO(env_factory(512), two, update_precision="f32", **ok)
    with pytest.raises(ValueError, match="policy_forward|f32"):
        PopulationPPO(env_factory(512), two, policy_forward="f32class", **ok)
    with pytest.raises(ValueError, match="batch_size"):
        PopulationPPO(env_factory(512), [dict(seed=3), dict(seed=4, batch_size=512)], **ok)
    with pytest.raises(ValueError, match="n_epochs"):
        PopulationPPO(env_factory(512), [dict(seed=3, n_epochs=3), dict(seed=4)], **ok)
    assert not dist.is_initialized()
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(tmp, "store"), rank=0, world_size=1)
        MfmaPpoUpdater.force_data_parallel = True
        try:
            with pytest.raises(ValueError, match="data-parallel"):
                PopulationPPO(env_factory(512), two, **ok)
        finally:
            MfmaPpoUpdater.force_data_parallel = False
            dist.destroy_process_group()


def test_batched_update_refusals_come_before_the_env_is_used():
    batched_update_refusals(_stub_env)


def test_population_updater_refusals_need_no_device():
    from optimal_quad_control_rl_amd.ppo import MfmaPpoPopulationUpdater, MfmaPpoUpdater

    fake = object.__new__(MfmaPpoUpdater)          # no handle, no device: the checks run before either is asked for
    fake.precision, fake._h = "f16-operands", None
    f32 = object.__new__(MfmaPpoUpdater)
    f32.precision, f32._h = "f32", None
    for bad in ([], [fake] * 257, [fake, object()], [fake, f32], [fake, fake]):
        with pytest.raises(ValueError):
            MfmaPpoPopulationUpdater(bad)


def test_package_surface_and_tool():
    import importlib.util
    import inspect

    from optimal_quad_control_rl_amd import population, ppo

    assert inspect.signature(population.PopulationPPO.__init__).parameters["batched_update"].default is False
    for method in ("epoch", "status", "close"):
        assert callable(getattr(ppo.MfmaPpoPopulationUpdater, method)), method
    for method in ("_train_prepare", "_native_begin", "_native_finish", "_train_native", "train"):
        assert callable(getattr(ppo.PPO, method)), method
    assert "batched_update=False" in population.__doc__ and "batched_update=True" in population.__doc__
    spec = importlib.util.spec_from_file_location("train_population", os.path.join(ROOT, "tools", "train_population.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.parser().parse_args(["--seeds", "0-2", "--batched-update"]).batched_update is True
    assert tool.parser().parse_args(["--seeds", "0-2"]).batched_update is False
