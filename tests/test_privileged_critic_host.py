"""CPU-side checks of the privileged critic (qr_rollout_policy_privileged, qr_ppo_grad_privileged, qr_ppo_minibatch_privileged,
qr_ppo_epoch_privileged): the four entry points in the header, the ctypes table and the build -- each its twin's list with the new
pointer(s) directly behind obs -- NULL handles, the argument validation of PPO(privileged_critic=True) before the env is touched, and the
flag of tools/train_ppo.py.  No GPU."""
import ctypes as C
import os
import subprocess
import sys
import types

import pytest
import torch

import abi_decl
from optimal_quad_control_rl_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLLOUT = "qr_rollout_policy_privileged"
# name -> (twin, {argument of the twin: the argument that sits directly behind it})
TWINS = {ROLLOUT: ("qr_rollout_policy_history", {"obs_out_dev": "critic_obs_out_dev", "last_obs_dev": "critic_last_obs_dev"}),
         "qr_ppo_grad_privileged": ("qr_ppo_grad", {"obs_dev": "critic_obs_dev"}),
         "qr_ppo_minibatch_privileged": ("qr_ppo_minibatch", {"obs_dev": "critic_obs_dev"}),
         "qr_ppo_epoch_privileged": ("qr_ppo_epoch", {"obs_dev": "critic_obs_dev"})}


@pytest.mark.parametrize("name", sorted(TWINS))
def test_entry_point_is_declared_bound_exported_and_optional(name):
    twin_name, extra = TWINS[name]
    text, code = abi_decl.header_of(name)
    _, ret, names, types_ = abi_decl.declaration(code, name)
    _, _, twin_names, twin_types = abi_decl.declaration(abi_decl.header_of(twin_name)[1], twin_name)
    want_names, want_types, want_bound = [], [], []
    for arg, typ, bound in zip(twin_names, twin_types, _lib.SIGNATURES[twin_name][1]):
        want_names.append(arg); want_types.append(typ); want_bound.append(bound)
        if arg in extra:
            want_names.append(extra[arg]); want_types.append(typ); want_bound.append(C.c_void_p)
    assert names == want_names and types_ == want_types and ret == "int", "the twin's list with the new pointer(s) directly behind obs"
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int and list(argtypes) == want_bound
    assert name in _lib.OPTIONAL_SYMBOLS and name in abi_decl.version_comment(text)
    assert abi_decl.define(code, "QR_ABI_VERSION") == 3
    assert name in open(os.path.join(build.CSRC, "exports.map")).read()
    src = "quadrace_rollout_privileged.hip"
    assert src in build.SOURCES and src not in build.PER_SOURCE_FLAGS and src not in build.NO_VGPR_FORM and os.path.exists(os.path.join(build.CSRC, src))
    assert hasattr(C.CDLL(build.build_native()), name)
    with pytest.raises(_lib.QuadraceError, match="%s.*rebuild" % name):          # a library built from older sources
        _lib.require(types.SimpleNamespace(), name)


def test_the_abi_comments_are_definitions():
    text, _ = abi_decl.header_of(ROLLOUT)
    flat = lambda c: c.replace("\n *", "")
    comment = flat(text.split("int qr_rollout_policy_privileged(")[0].rsplit("/*", 1)[1])
    for word in ("DEFINITION", "CONTRACT", "bit for bit", "[0, 4 - gates_ahead]", "BEFORE the sensor's noise", "[num_steps][N][L']", "or NULL",
                 "Refused before anything is launched", "directly behind the check of obs_out_dev", "all sigmas zero", "TERMINAL"):
        assert word in comment, word
    comment = flat(text.split("int qr_ppo_grad_privileged(")[0].rsplit("/*", 1)[1])
    for word in ("DEFINITION", "SPLIT", "TWIN", "COMPOSE", "bit for bit", "[rows][obs_len]", "part of the graph's key", "QR_PPO_NO_EPOCH_GRAPH",
                 "a NULL critic_obs_dev", "qr_ppo_grad_f32class", "population"):
        assert word in comment, word
    for name in ("qr_ppo_minibatch_privileged", "qr_ppo_epoch_privileged"):       # declared under the same block
        assert text.index("int qr_ppo_grad_privileged(") < text.index("int %s(" % name) < text.index("the update of a POPULATION of learners")


def test_null_handles_are_refused_without_a_device():
    L = _lib.load()
    rc = L.qr_rollout_policy_privileged(*([None] * 5), 1, 256, None, None, None, 0, 1, None, 0, 0, 0, *([None] * 11))
    assert rc == _lib.QR_E_INVALID and b"qr_rollout_policy_privileged" in L.qr_last_error() and b"null env" in L.qr_last_error()
    rc = L.qr_ppo_grad_privileged(*([None] * 9), 64, 0.2, 0.5, 0.0, None, None, None)
    assert rc == _lib.QR_E_INVALID and b"null argument" in L.qr_last_error()
    rc = L.qr_ppo_minibatch_privileged(*([None] * 11), 64, 0.2, 0.5, 0.0, 0.5, 3e-4, 0.9, 0.999, 1e-5, 0, None, None)
    assert rc == _lib.QR_E_INVALID and b"null argument" in L.qr_last_error()
    rc = L.qr_ppo_epoch_privileged(*([None] * 11), 64, 1, 1, 0, 0.2, 0.5, 0.0, 0.5, 3e-4, 0.9, 0.999, 1e-5, None, None)
    assert rc == _lib.QR_E_INVALID and b"null argument" in L.qr_last_error()


# ---- Python arguments ----------------------------------------------------------------------------------------------------------------------
def _stub_env(gates_ahead=1, q3=False):
    """an env that has nothing to touch: any use beyond the attributes below raises AttributeError"""
    env = types.SimpleNamespace(num_envs=512, device=torch.device("cpu"), gates_ahead=gates_ahead, state_len=24, VARIANT=0)
    if q3:
        env.KIND, env.trainer_state = "hover", lambda: None
        del env.gates_ahead
    return env


def test_ppo_refuses_what_the_privileged_critic_cannot_do_before_it_touches_the_env(monkeypatch):
    from optimal_quad_control_rl_amd.ppo import PPO, MfmaPpoUpdater

    ok = dict(fused_collect=True, native_update=True, privileged_critic=True)
    with pytest.raises(ValueError, match="privileged_critic needs fused_collect=True on a race env"):
        PPO(_stub_env(), **{**ok, "fused_collect": False})
    with pytest.raises(ValueError, match="privileged_critic needs fused_collect=True on a race env"):
        PPO(_stub_env(q3=True), **ok)
    with pytest.raises(ValueError, match="privileged_critic needs native_update=True: the torch update"):
        PPO(_stub_env(), **{**ok, "native_update": False})
    with pytest.raises(ValueError, match="privileged_critic needs update_precision='f16-operands': the f32-class gradient kernels"):
        PPO(_stub_env(), update_precision="f32", **ok)
    monkeypatch.setattr(MfmaPpoUpdater, "data_parallel", staticmethod(lambda: True))
    with pytest.raises(ValueError, match="privileged_critic has no data-parallel form"):
        PPO(_stub_env(), **ok)
    monkeypatch.undo()
    # ... and composes with a command history: that argument's own refusal is reached first, the env still untouched
    with pytest.raises(ValueError, match="command_history must be 0 or an integer in 1 .. 4 - gates_ahead"):
        PPO(_stub_env(1), command_history=4, **ok)
    with pytest.raises(AttributeError):          # every argument accepted: the constructor goes on to the env (which the stub does not have)
        PPO(_stub_env(1), command_history=2, **ok)


def test_the_updater_refuses_the_paths_without_a_privileged_form():
    from optimal_quad_control_rl_amd.ppo import MfmaPpoUpdater

    up = object.__new__(MfmaPpoUpdater)          # no handle: _critic_rows reads `precision` and nothing else before it refuses
    up.precision = "f32"
    rows = torch.zeros((64, 24))
    for what in ("grad", "minibatch", "epoch"):
        with pytest.raises(ValueError, match=r"%s\(critic_obs=...\): the f32-class gradient kernels \(qr_ppo_grad_f32class\) have no privileged-critic form" % what):
            up._critic_rows(rows, rows, what)
    up.precision = "f16-operands"
    with pytest.raises(ValueError, match="f32-class"):
        up._critic_rows(rows, rows, "grad", precision="f32")
    up._h = None


def test_train_ppo_names_the_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_ppo.py"), "--help"], check=True, capture_output=True, text=True).stdout
    assert "--privileged-critic" in out and "qr_rollout_policy_privileged" in out.replace("\n", " ").replace("  ", " ")
