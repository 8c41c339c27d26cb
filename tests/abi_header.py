"""A reader of include/gm_hip.h for the ABI tests: its structs (field names in order), its #defines, its enum constants
and its prototypes, and the one table that says which ctypes type a C parameter type binds to.  The header is regular
C (one declaration style, no function pointers, no nested braces), so regular expressions read all of it."""
import ctypes
import os
import re
import shutil
import subprocess

from generative_models_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "gm_hip.h")

_DECLARATOR = r"\**\s*(\w+)\s*(?:\[\w+\])?"


def text():
    """The header without comments, line continuations joined."""
    t = open(HEADER).read().replace("\\\n", " ")
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", t, flags=re.S))


def structs():
    """{C name: [field names in declaration order]} of every `typedef struct gm_x { ... } gm_x;`."""
    out = {}
    for name, body, alias in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text(), flags=re.S):
        assert name == alias, (name, alias)
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = decl.split(",")
            fields.append(re.search(_DECLARATOR + r"\s*$", first).group(1))
            fields += [re.fullmatch(r"\s*" + _DECLARATOR + r"\s*", m).group(1) for m in more]
        out[name] = fields
    return out


def defines():
    """({object-like GM_* macro: its text}, {function-like GM_* macro: its parameter names}), the include guard left out."""
    plain, fn = {}, {}
    for name, params, body in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(GM_\w+)(\([^)]*\))?[ \t]*(.*)$", text(), flags=re.M):
        if params:
            fn[name] = [p.strip() for p in params[1:-1].split(",")]
        elif body.strip():                                   # the guard defines nothing
            plain[name] = body.strip()
    return plain, fn


def enum_constants():
    """The names of every enumerator of the header's (anonymous) enums."""
    return [n for body in re.findall(r"\benum\s*\{(.*?)\}", text(), flags=re.S) for n in re.findall(r"\b(GM_\w+)\s*=", body)]


def prototypes():
    """{function: (return type, [parameter types])} as normalised C type strings: no `const`, no parameter names, `T*`."""
    t = re.sub(r"\{.*?\}", "{}", text(), flags=re.S)        # struct and enum bodies out of the way
    t = re.sub(r"^[ \t]*#.*$", "", t, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([\w \t\*]+?)\b(gm_\w+)\s*\(([^)]*)\)\s*;", t):
        assert name not in out, name
        ps = [] if params.strip() in ("", "void") else [_c_type(p, named=True) for p in params.split(",")]
        out[name] = (_c_type(ret, named=False), ps)
    return out


def _c_type(decl, named):
    decl = re.sub(r"\bconst\b", " ", decl).strip()
    if named:
        decl = re.sub(r"\w+\s*$", "", decl)                  # the parameter's name
    return re.sub(r"\s+", " ", decl.strip()).replace(" *", "*")


def declared_symbols():
    """Every function the header declares, sorted."""
    return sorted(prototypes())


SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double,
           "unsigned int": ctypes.c_uint, "unsigned long long": ctypes.c_ulonglong}


def ctypes_forms(c_type, result=False):
    """The ctypes types a C parameter (or, with `result`, return) type may be bound to."""
    if result and c_type == "char*":
        return (ctypes.c_char_p,)
    if c_type in SCALARS:
        return (SCALARS[c_type],)
    if c_type in _abi.STRUCTS:                               # by value
        return (_abi.STRUCTS[c_type],)
    if c_type == "void*":                                    # streams, events, graphs, communicators, untyped buffers
        return (ctypes.c_void_p,)
    if c_type.endswith("**"):
        return (ctypes.POINTER(ctypes.c_void_p),)
    if c_type.endswith("*") and c_type[:-1] in _abi.STRUCTS:
        return (ctypes.POINTER(_abi.STRUCTS[c_type[:-1]]),)
    if c_type.endswith("*") and c_type[:-1] in SCALARS:      # a device buffer or a host out-parameter: the header
        return (ctypes.c_void_p, ctypes.POINTER(SCALARS[c_type[:-1]]))     # does not say which
    raise AssertionError("no ctypes form for the C type %r" % c_type)


def host_cc():
    return shutil.which("gcc") or shutil.which("cc")


def run_c(tmp_path, name, body_lines):
    """Compile `int main` of body_lines against the header with the host C compiler, run it, return its output lines."""
    src = tmp_path / (name + ".c")
    src.write_text("\n".join(['#include <stdio.h>', '#include <stddef.h>', '#include "gm_hip.h"', 'int main(void) {']
                             + body_lines + ['return 0;', '}']))
    exe = tmp_path / name
    subprocess.run([host_cc(), "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
