"""The one place in tests/ that reads include/quadrace.h and include/quad3d.h: the declared functions with normalised types, struct
fields, #define values, the version comment, and the rule by which a ctypes type may bind a declared C type.  tests/abi_table.py holds
what is pinned about single entry points, tests/test_abi_host.py the checks.  A plain helper module: no fixtures, nothing at import."""
import ctypes as C
import os
import re
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name="quadrace.h"):
    """(text, code): code is text without /* */ and // comments"""
    with open(os.path.join(ROOT, "include", name)) as f:
        text = f.read()
    return text, re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


def header_of(name):
    return header("quad3d.h" if name.startswith("q3_") else "quadrace.h")


def _spelling(c_type):
    """one spelling per type: "const float *", "const float * const *", "qr_policy *" (also for `struct qr_policy*`)"""
    return " ".join(re.sub(r"\bstruct\b", "", c_type).replace("*", " * ").split())


def functions(code, prefix):
    """every declared function whose name starts with prefix: (name, return type, [argument names], [argument types])"""
    out = []
    for ret, name, params in re.findall(r"((?:const\s+)?\w+[\s*]+)(%s\w+)\s*\(([^()]*)\)\s*;" % prefix, code):
        names, types_ = [], []
        for param in map(_spelling, params.split(",")):
            if param not in ("", "void"):
                typ, arg = param.rsplit(" ", 1)
                if "[" in arg:                                    # const float start_pos[3]: an array parameter is a pointer
                    typ, arg = typ + " *", arg.split("[")[0]
                names.append(arg)
                types_.append(typ)
        out.append((name, _spelling(ret), names, types_))
    return out


def declaration(code, name):
    rows = [f for f in functions(code, name[:3]) if f[0] == name]
    assert len(rows) == 1, "include/*.h does not declare %s (once)" % name
    return rows[0]


def struct_fields(code, name):
    """[(type, field name)] of `typedef struct { ... } name;`, one entry per declarator"""
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


def define(code, name):
    m = re.search(r"#define\s+%s\s+(-?\d+)\b" % name, code)
    assert m, "no #define %s <integer>" % name
    return int(m.group(1))


def version_comment(text):
    """the comment behind #define QR_ABI_VERSION: the list of what was added without a bump"""
    return text.split("#define QR_ABI_VERSION")[1].split("*/")[0]


SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double,
           "size_t": C.c_size_t}
STRUCTS = {"qr_config": "QrConfig", "qr_ppo_member_args": "QrPpoMemberArgs", "qr_ppo_prepare_shared": "QrPpoPrepareShared",
           "qr_ppo_prepare_member": "QrPpoPrepareMember"}    # typedef -> the Structure of _lib.py


def binding_matches(c_type, ctype):
    """May the ctypes type bind the declared C type?  Scalars exactly; a pointer as c_void_p (handles and device buffers travel that way
    by design), POINTER(its pointee's exact scalar) or POINTER(the _lib Structure of its typedef); a pointer to pointer as
    POINTER(c_void_p) or c_void_p; const char * as c_char_p.  Nothing else."""
    from optimal_quad_control_rl_amd import _lib

    words = [w for w in c_type.split() if w != "const"]
    stars, base = words.count("*"), " ".join(w for w in words if w != "*")
    if stars == 0:
        return base in SCALARS and ctype is SCALARS[base]
    if base == "char":
        return stars == 1 and ctype is C.c_char_p
    if stars == 2:
        return ctype in (C.POINTER(C.c_void_p), C.c_void_p)
    typed = SCALARS.get(base) or getattr(_lib, STRUCTS.get(base, ""), None)
    return stars == 1 and (ctype is C.c_void_p or (typed is not None and ctype is C.POINTER(typed)))


def stub_env(n, **over):
    """An env of n envs that must not be used: the constructors under test check their arguments first.  Keyword arguments add or
    replace fields."""
    def touched(*a, **k):
        raise AssertionError("the argument checks come before the env is used")

    fields = dict(num_envs=n, state_len=24, device=None, VARIANT=0, reset_device=touched, condition_reset=touched, set_terminal_obs_buffer=touched)
    return types.SimpleNamespace(**{**fields, **over})
