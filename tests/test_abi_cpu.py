"""The Python declarations of the C-ABI (generative_models_amd/_abi.py) against include/gm_hip.h, whole and in one place
(no GPU): every struct's layout and field names, every prototype's parameter and return types, every #define's and
enumerator's value, and that a struct pointer of the wrong type is refused before the library is entered."""
import ctypes
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import abi_header as H  # noqa: E402
from generative_models_amd import _abi, _lib, bgan, metrics, ops_fused  # noqa: E402

needs_cc = pytest.mark.skipif(H.host_cc() is None, reason="no host C compiler")

# the one struct pointer that stays untyped: gm_linear_plan's descriptor is a gm_fwd_args, gm_dx_args or gm_dw_adam_args
# by mode, `const void*` in the header and c_void_p here (ops.linear_plan casts)
UNTYPED_STRUCT_POINTERS = {("gm_linear_plan", 1)}

LOSS_ENUM = {"GM_LOSS_NS": "ns", "GM_LOSS_MM": "mm", "GM_LOSS_W": "w", "GM_LOSS_LS": "ls", "GM_LOSS_RA": "ra",
             "GM_LOSS_FISHER": "fisher", "GM_LOSS_F_TV": "f_total_variation", "GM_LOSS_F_FKL": "f_forward_kl",
             "GM_LOSS_F_RKL": "f_reverse_kl", "GM_LOSS_F_PEARSON": "f_pearson", "GM_LOSS_F_HELLINGER": "f_hellinger",
             "GM_LOSS_F_JS": "f_jensen_shannon"}
# a #define or enumerator GM_<NAME> is mirrored by the integer _abi.<NAME>, except these: integers of _abi under another
# name ...
RENAMED = {"GM_EINVAL": "GM_EINVAL", "GM_EUNSUPPORTED": "GM_EUNSUPPORTED", "GM_PLAN_FIELDS": "PLAN_INTS",
           "GM_SN_STAT_SIGMA": "SN_SIGMA", "GM_SN_STAT_NW2": "SN_NW2", "GM_SN_STAT_NT": "SN_NT", "GM_SN_STAT_NR": "SN_NR"}
# ... and entries of _abi's tables, or a model's own name for the limit
ELSEWHERE = dict(
    {"GM_NOISE_SALT_PEPPER": _abi.NOISE["salt_pepper"], "GM_NOISE_GAUSSIAN": _abi.NOISE["gaussian"],
     "GM_BGAN_MAX_J": bgan.MAX_J, "GM_PARZEN_MAX_SIGMAS": metrics.MAX_SIGMAS},
    **{"GM_PLAN_MODE_" + k.upper(): v for k, v in _abi.PLAN_MODE.items()},
    **{"GM_PLAN_" + v.upper(): k for k, v in _abi.PLAN_FAMILY.items()},
    **{"GM_PLAN_F_" + f.upper(): i for i, f in enumerate(_abi.PLAN_FIELDS)},
    **{c: _abi.LOSS[k] for c, k in LOSS_ENUM.items()})
# in the header for the C side alone: Python passes no such number and checks no such limit
HEADER_ONLY = {"GM_NOISE_NONE", "GM_PARZEN_CHUNK", "GM_SGHMC_MAX_SEGS", "GM_STAGE_MAX_SEGS"}
# upper-case integers of _abi that the header does not name
PYTHON_ONLY = set()
# the header's function-like macros, their Python forms and where to compare them
MACROS = {"GM_IAF_PART_STRIDE": (ops_fused.iaf_part_stride, [(2, 4, 0), (8, 16, 6), (32, 64, 32)]),
          "GM_IAF_PARTS": (ops_fused.iaf_nparts, [(1, 1), (100, 1), (100, 3), (64, 64), (65, 64), (7, 100)])}


@needs_cc
def test_every_struct_has_the_headers_layout_and_field_names(tmp_path):
    parsed = H.structs()
    assert set(_abi.STRUCTS) == set(parsed), set(_abi.STRUCTS) ^ set(parsed)
    lines = []
    for cname, ct in _abi.STRUCTS.items():
        assert ct.c_name == cname
        assert [f for f, _ in ct._fields_] == parsed[cname], "%s (%s): fields differ from the header's" % (ct.__name__, cname)
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f) for f in parsed[cname]]
    out = H.run_c(tmp_path, "layout", lines)
    assert len(out) == len(lines)
    for line in out:
        cname, field, val = line.split()
        ct = _abi.STRUCTS[cname]
        got = ctypes.sizeof(ct) if field == "size" else getattr(ct, field).offset
        assert got == int(val), "%s (%s): %s is %d in ctypes and %s in C" % (ct.__name__, cname, field, got, val)
    print("structs checked:", len(_abi.STRUCTS))
    assert len(_abi.STRUCTS) >= 53


def test_every_prototype_has_the_headers_parameter_and_return_types():
    protos = H.prototypes()
    assert set(protos) == set(_abi._SIGNATURES), set(protos) ^ set(_abi._SIGNATURES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _abi._SIGNATURES[name]
        assert restype in H.ctypes_forms(ret, result=True), "%s returns %s, bound as %s" % (name, ret, restype)
        assert len(argtypes) == len(params), "%s takes %d parameters, bound with %d" % (name, len(params), len(argtypes))
        for i, (c_type, bound) in enumerate(zip(params, argtypes)):
            forms = H.ctypes_forms(c_type)
            if c_type.endswith("*") and c_type[:-1] in _abi.STRUCTS:
                assert len(forms) == 1 and forms[0] is ctypes.POINTER(_abi.STRUCTS[c_type[:-1]])
            assert bound in forms, "%s: parameter %d is %s, bound as %s" % (name, i, c_type, bound)
    for name, i in UNTYPED_STRUCT_POINTERS:
        assert protos[name][1][i] == "void*" and _abi._SIGNATURES[name][1][i] is ctypes.c_void_p
    print("prototypes checked:", len(protos))
    assert len(protos) >= 180


@needs_cc
def test_every_constant_has_the_headers_value(tmp_path):
    plain, macros = H.defines()
    enums = H.enum_constants()
    names = list(plain) + enums
    assert len(set(names)) == len(names)
    lines = ['printf("%s %%lld\\n", (long long)(%s));' % (n, n) for n in names]
    calls = [(m, args) for m, (_, cases) in MACROS.items() for args in cases]
    lines += ['printf("%s %%lld\\n", (long long)%s(%s));' % (m, m, ", ".join(map(str, args))) for m, args in calls]
    out = H.run_c(tmp_path, "constants", lines)
    assert len(out) == len(names) + len(calls)
    mirrored = set()
    for name, line in zip(names, out):
        value = int(line.split()[1])
        assert line.split()[0] == name
        attr = RENAMED.get(name, name[3:])
        places = [name in HEADER_ONLY, name in ELSEWHERE, isinstance(getattr(_abi, attr, None), int)]
        assert sum(places) == 1, "%s must be header-only, or mirrored in one place: %s" % (name, places)
        if name in HEADER_ONLY:
            continue
        mirror = ELSEWHERE[name] if name in ELSEWHERE else getattr(_abi, attr)
        assert mirror == value, "%s is %d in the header and %r in Python" % (name, value, mirror)
        mirrored.add(attr)
    assert HEADER_ONLY <= set(names)
    for (m, args), line in zip(calls, out[len(names):]):
        assert MACROS[m][0](*args) == int(line.split()[1]), (m, args)
    assert set(macros) == set(MACROS)
    # and the other way: every upper-case integer of _abi is one of the header's
    for py, v in vars(_abi).items():
        if py.isupper() and isinstance(v, int) and not isinstance(v, bool):
            assert py in mirrored or py in PYTHON_ONLY, "_abi.%s corresponds to no define" % py
    print("defines checked: %d object-like (%d mirrored, %d header-only) + %d function-like; enumerators: %d"
          % (len(plain), len(plain) - len(HEADER_ONLY), len(HEADER_ONLY), len(macros), len(enums)))
    assert len(plain) >= 131 and len(enums) >= 19


@pytest.mark.skipif(not os.path.isfile(_lib.LIB_PATH), reason="libgm_hip.so not built")
def test_a_block_of_the_wrong_struct_is_refused_before_the_library_is_entered():
    lib = _lib.load()
    with pytest.raises(ctypes.ArgumentError):
        lib.gm_iaf_step(None, ctypes.byref(_abi.FlowStepArgs()))
    noise, tables, out = _abi.DdpmNoise(), _abi.DdpmTables(), _abi.DdpmOut()
    with pytest.raises(ctypes.ArgumentError):
        lib.gm_ddpm_qsample(None, ctypes.byref(tables), ctypes.byref(noise), ctypes.byref(out), None, 0, 0, 0)
