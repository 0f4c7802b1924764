"""CPU-side checks (no GPU needed): the C-ABI library builds, loads and exports every symbol that
include/quadrace.h and include/quad3d.h declare; every row of the ctypes table binds its declaration compatibly
(tests/abi_decl.py reads the headers); what is pinned about single entry points (tests/abi_table.py) holds; host-side helpers
behave like the reference's; and -- on a box without a GPU -- the product fails loudly instead of falling back."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_decl
import abi_table
from optimal_quad_control_rl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARED = {f[0]: f for name, prefix in (("quadrace.h", "qr_"), ("quad3d.h", "q3_")) for f in abi_decl.functions(abi_decl.header(name)[1], prefix)}


def header_functions():
    return sorted(DECLARED)


@pytest.fixture(scope="module")
def exported():
    """the built library as the dynamic loader sees it: no argtypes, nothing from _lib.py"""
    from optimal_quad_control_rl_amd import build

    build.build_native()
    return C.CDLL(build.LIB)


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_every_declared_function_is_bound_compatibly(name, exported):
    """A wrong width or a dropped argument in a row of _lib.SIGNATURES loads and runs: this is what stops it."""
    _, ret, _, types_ = DECLARED[name]
    restype, argtypes = _lib.SIGNATURES[name]
    assert abi_decl.binding_matches(ret, restype), (ret, restype)
    assert len(argtypes) == len(types_), (types_, argtypes)
    for k, (c_type, ctype) in enumerate(zip(types_, argtypes)):
        assert abi_decl.binding_matches(c_type, ctype), "argument %d: %s bound as %s" % (k, c_type, ctype)
    assert hasattr(exported, name), "%s declared in include/*.h but not exported" % name
    fn = getattr(_lib.load(), name)
    assert fn.restype is restype and list(fn.argtypes) == list(argtypes)


def _part(seq, span):
    return seq[span[0]:span[1]]


@pytest.mark.parametrize("row", abi_table.ROWS, ids=lambda r: r["name"])
def test_pinned_entry_points(row):
    from optimal_quad_control_rl_amd import build

    name = row["name"]
    text, code = abi_decl.header_of(name)
    _, ret, names, types_ = abi_decl.declaration(code, name)
    restype, argtypes = _lib.SIGNATURES[name]
    assert names == row["args"] and ret == "int" and restype is C.c_int and len(argtypes) == len(names)
    for column, actual in (("types", types_), ("bound", argtypes)):
        pinned = row.get(column, {})
        for k, want in pinned.items() if isinstance(pinned, dict) else enumerate(pinned):
            assert actual[k] == want, (column, k, actual[k], want)
        assert isinstance(pinned, dict) or len(pinned) == len(actual), column
    if row.get("optional"):
        assert name in _lib.OPTIONAL_SYMBOLS
    exports = open(os.path.join(build.CSRC, "exports.map")).read()
    assert name[:3] + "*;" in exports and row.get("in_exports", "") in exports
    if "in_version_comment" in row:
        assert row["in_version_comment"] in abi_decl.version_comment(text)
    if "source" in row:
        assert row["source"] in build.SOURCES and os.path.exists(os.path.join(build.CSRC, row["source"]))
        assert not (row.get("default_flags") and row["source"] in build.PER_SOURCE_FLAGS)
        assert not (row.get("vgpr_form") and row["source"] in build.NO_VGPR_FORM)
    for define, value in row.get("defines", {}).items():
        assert abi_decl.define(code, define) == value, define
    for pattern in row.get("patterns", []):
        assert re.search(pattern, code), pattern
    anchor, words = row.get("contract", (None, []))
    comment = text if anchor is None else text.split(anchor)[0].rsplit("/*", 1)[1]
    for word in words:
        assert word in comment, word
    for mine, other, theirs in row.get("same_as", []):
        assert _part(names, mine) == _part(abi_decl.declaration(abi_decl.header_of(other)[1], other)[2], theirs), other


@pytest.mark.parametrize("row", [r for r in abi_table.ROWS if "null_call" in r], ids=lambda r: r["name"])
def test_null_handles_are_refused_without_a_device(row):
    """A NULL handle is refused, not dereferenced -- before the library asks for a device."""
    L = _lib.load()
    args, code, message = row["null_call"]
    rc = getattr(L, row["name"])(*args)
    assert rc != _lib.QR_OK and code in (None, rc), rc
    assert message is None or message in L.qr_last_error()


def test_every_optional_symbol_is_a_signature():
    assert set(_lib.OPTIONAL_SYMBOLS) <= set(_lib.SIGNATURES) and len(set(_lib.OPTIONAL_SYMBOLS)) == len(_lib.OPTIONAL_SYMBOLS)


@pytest.mark.parametrize("name", _lib.OPTIONAL_SYMBOLS)
def test_a_library_without_an_optional_symbol_is_reported_by_name(name):
    class Old:   # a library built from older sources: no such attribute
        pass

    with pytest.raises(_lib.QuadraceError, match=name):
        _lib.require(Old(), name)
    assert _lib.require(_lib.load(), name) is not None


def test_library_builds_and_exports_every_header_symbol():
    from optimal_quad_control_rl_amd import _lib, build

    build.build_native()
    L = C.CDLL(build.LIB)
    names = header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/*.h but not exported"
    assert sorted(_lib.SIGNATURES) == names, "ctypes table and header disagree"
    assert _lib.load().qr_abi_version() == 3


def test_dynamic_symbol_table_holds_the_c_abi_only():
    """libquadrace.so is built with -fvisibility=hidden and a linker version script: `nm -D` lists the qr_* / q3_* entry
    points of include/*.h and nothing else (no C++ launchers, kernel handles or std:: template instantiations)."""
    import subprocess

    from optimal_quad_control_rl_amd import build

    build.build_native()
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB], text=True)
    syms = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    assert syms and all(s.startswith(("qr_", "q3_")) for s in syms), [s for s in syms if not s.startswith(("qr_", "q3_"))]
    assert sorted(syms) == header_functions()


def test_no_cpu_fallback():
    """Without a GPU the product must refuse to run (the oracle is test infrastructure, never a fallback)."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from optimal_quad_control_rl_amd import _lib

    L = _lib.load()
    cfg = _lib.QrConfig(0, 16, 1, 0, 0, 0, 0)
    h = C.c_void_p()
    rc = L.qr_create(C.byref(cfg), C.byref(h))
    assert rc == _lib.QR_E_NO_DEVICE, rc
    assert b"no HIP device" in L.qr_last_error()
    from optimal_quad_control_rl_amd import Quadcopter3DGates, zigzag_track

    with pytest.raises(RuntimeError):
        Quadcopter3DGates(4, *zigzag_track())
    # the predecessor envs (include/quad3d.h) behave the same way
    rc = L.q3_create(0, 16, 0, 0, C.byref(h))
    assert rc == _lib.QR_E_NO_DEVICE, rc
    from optimal_quad_control_rl_amd.quad3d import Quadcopter3DVec

    with pytest.raises(RuntimeError):
        Quadcopter3DVec(4)
    # ... and so do the policy / PPO-update kernels
    assert L.qr_policy_create(17, 0, C.byref(h)) == _lib.QR_E_NO_DEVICE
    assert L.qr_ppo_create(17, 0, 4096, C.byref(h)) == _lib.QR_E_NO_DEVICE
    assert b"no CPU fallback" in L.qr_last_error()


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "optimal_quad_control_rl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("CPU oracle", "").replace("the oracle", "") or f == "build.py", \
                    f"{f} mentions the oracle"


def test_tracks_match_reference_constants():
    from optimal_quad_control_rl_amd import TRAIN_DISTURBANCE_RANGES, square_track, zigzag_track

    d = np.load(os.path.join(ROOT, "tests", "golden", "tracks.npz"))
    for name, fn in (("zigzag", zigzag_track), ("square", square_track)):
        gp, gy, sp = fn()
        np.testing.assert_array_equal(gp, d[name + "_gate_pos"])
        np.testing.assert_array_equal(gy, d[name + "_gate_yaw"])
        np.testing.assert_array_equal(sp, d[name + "_start_pos"])
    assert TRAIN_DISTURBANCE_RANGES.shape == (6, 2)


def test_residual_blob_is_the_reference_weights():
    from optimal_quad_control_rl_amd.vec_env import default_residual_blob

    b = default_residual_blob()
    assert b.shape == (740,) and b.dtype == np.float32
    # first weights of nn_thrust_weights_fc1 (c_code/nn_thrust.c:6)
    np.testing.assert_allclose(b[:3], [0.6684572696685791, 0.27626726031303406, -0.14709796011447906], rtol=1e-7)


def test_box_stub():
    from optimal_quad_control_rl_amd.vec_env import Box

    b = Box(-1, 1, shape=(4,))
    assert b.shape == (4,) and b.contains(b.sample())


def test_kernel_sincos_algorithm_accuracy():
    """The kernel's branch-free sincos (qr_sincos), emulated op-for-op in NumPy float32: abs error <= 8e-8 vs float64
    over the argument range the env can reach -- the same accuracy class as NumPy's float32 sin/cos that the
    reference evaluates."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_sincos import sincos32

    rng = np.random.default_rng(1)
    for R in (0.4, 3.2, 300.0, 20000.0):
        x = rng.uniform(-R, R, 200_000).astype(np.float32)
        s, c = sincos32(x)
        assert np.abs(s - np.sin(x.astype(np.float64))).max() < 8e-8
        assert np.abs(c - np.cos(x.astype(np.float64))).max() < 8e-8
    # constants in the kernel source are the ones that were checked
    src = open(os.path.join(ROOT, "optimal_quad_control_rl_amd", "csrc", "quadrace_device.hpp")).read()
    for const in ("0.6366197723675814f", "1.5707963705062866f", "-4.371139000186241e-8f", "-1.7151245100059e-15f",
                  "2.7183114939898219e-6f", "-0.49999999725103100f"):
        assert const in src


def test_library_reads_no_environment_variable():
    """Kernel forms are chosen through the ABI (qr_set_rollout_form, qr_ppo_create_ex), never through getenv: the library does not
    even import the symbol."""
    import subprocess

    from optimal_quad_control_rl_amd import build

    lib = build.build_native_locked()
    und = subprocess.run(["nm", "-D", "--undefined-only", lib], check=True, capture_output=True, text=True).stdout
    assert "getenv" not in und
    # ... and neither does the Python package select a kernel form, a precision or a code path from the environment:
    # the only read left is QR_PROBE_LIB in _lib.py, which lets the forensic tools load an older build whose ABI lacks round-5 entries
    import glob
    import os
    import re

    pkg = os.path.dirname(build.__file__)
    for path in sorted(glob.glob(os.path.join(pkg, "*.py"))):
        with open(path) as f:
            src = f.read()
        reads = re.findall(r"(?:os\.environ|getenv\()[^\n]*", src)
        if os.path.basename(path) == "_lib.py":
            assert all("QR_PROBE_LIB" in r for r in reads), reads
        else:
            assert not reads, (path, reads)

