"""The Python binding is read from the headers of include/ (bunmpc_amd/_abi.py, one table per header in bunmpc_amd/_lib.py).  Three
witnesses that it reads them right, none of which needs a GPU: the tables recorded before the reader and before the one binding module
(tests/golden/abi*.json), a C compiler's sizeof / offsetof of every struct and field, and the reader on small headers that hold one
construct of its subset each.  And the checks of the header table at import, and the dispatch knobs derived from it."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

from bunmpc_amd import _abi, _lib
from bunmpc_amd import build as hip_build
from tests.util import knob_setter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_abi  # noqa: E402


GOLDEN = {"bunmpc.h": "abi.json", "bunmpc_goals.h": "abi_goals.json", "bunmpc_turn.h": "abi_turn.json", "bunmpc_foot_pairs.h": "abi_foot_pairs.json"}
COUNTS = {"bunmpc.h": (164, 18), "bunmpc_goals.h": (5, 3), "bunmpc_turn.h": (3, 1), "bunmpc_foot_pairs.h": (2, 0)}      # functions, structs
INCLUDE = os.path.dirname(hip_build.INCLUDE)


def test_binding_equals_the_recorded_table():
    """tests/golden/abi.json was written by tools/record_abi.py on the commit whose _lib.py declared every signature and struct by
    hand, the side headers' tables on the commits that bound each header in a module of its own; an ABI change is re-recorded with
    that tool and reviewed as a diff of the file"""
    for header, abi in _lib.HEADERS.items():
        with open(os.path.join(ROOT, "tests", "golden", GOLDEN[header])) as f:
            assert record_abi.dump(abi) == f.read(), header
        assert (len(abi.functions), len(abi.structs)) == COUNTS[header]


def test_one_module_binds_every_header():
    assert list(_lib.HEADERS) == list(GOLDEN) == list(_lib.HEADER_NAMES)
    assert {os.path.join(INCLUDE, h) for h in _lib.HEADERS} <= set(hip_build.dependencies())
    tables = list(_lib.HEADERS.values())
    for i, a in enumerate(tables):                           # no header declares what another does
        for b in tables[i + 1:]:
            assert not set(a.functions) & set(b.functions) and not set(a.structs) & set(b.structs)
    assert len(_lib._SIGS) == 174 and _lib.exported_symbols() == sorted(f for a in tables for f in a.functions)
    lib = _lib.lib()                                         # every declared symbol is in the library, and the structs have their sizes
    assert lib.bmpc_turn_struct_size() == C.sizeof(_lib.Turn) == 16
    assert lib.bmpc_cc_goal_batch_struct_size() == C.sizeof(_lib.CcGoalBatch)


def test_every_struct_has_its_python_name():
    for header, names in _lib.HEADER_NAMES.items():
        for cname, pyname in names.items():
            cls = getattr(_lib, pyname)
            assert cls is _lib.HEADERS[header].structs[cname] and cls.__name__ == pyname and cls.__doc__ == cname


def _tree(tmp_path, **extra):
    """a copy of include/ with further headers {stem: text}"""
    shutil.copytree(INCLUDE, tmp_path / "include")
    for stem, text in extra.items():
        (tmp_path / "include" / (stem + ".h")).write_text(text)
    return str(tmp_path / "include")


def test_a_header_without_a_row_is_an_import_error(tmp_path):
    include = _tree(tmp_path, bunmpc_fifth="int bmpc_fifth(void);\n")
    with pytest.raises(ImportError, match="bunmpc_fifth.h"):
        _lib.read_headers(include, _lib.HEADER_NAMES)
    with pytest.raises(ImportError, match="bunmpc_turn.h"):      # and a row without a header
        _lib.read_headers(INCLUDE, {h: n for h, n in _lib.HEADER_NAMES.items() if h != "bunmpc_turn.h"} | {"bunmpc_fifth.h": {}})
    assert list(_lib.read_headers(include, _lib.HEADER_NAMES | {"bunmpc_fifth.h": {}})["bunmpc_fifth.h"].functions) == ["bmpc_fifth"]


@pytest.mark.parametrize("text,rows,words", [      # a fifth header, its rows of the table, what the message names
    ("int bmpc_set_force_foot_pairs(int on);\n", {}, ("function bmpc_set_force_foot_pairs", "bunmpc_fifth.h", "bunmpc_foot_pairs.h")),
    ("typedef struct { int a; } bmpc_turn_t;\n", {"bmpc_turn_t": "Fifth"}, ("struct bmpc_turn_t", "bunmpc_fifth.h", "bunmpc_turn.h")),
    ("typedef struct { int a; } bmpc_fifth_t;\n", {"bmpc_fifth_t": "Turn"}, ("class name Turn", "bunmpc_fifth.h", "bunmpc_turn.h")),
    ("#define BMPC_BAD_ARG 7\n", {}, ("BMPC_BAD_ARG", "bunmpc_fifth.h", "bunmpc.h")),
    ("typedef struct { int a; } bmpc_other_t;\n", {"bmpc_fifth_t": "Fifth"}, ("bunmpc_fifth.h", "bmpc_fifth_t", "bmpc_other_t")),
])
def test_what_two_headers_declare_is_an_import_error(tmp_path, text, rows, words):
    with pytest.raises(ImportError) as e:
        _lib.read_headers(_tree(tmp_path, bunmpc_fifth=text), _lib.HEADER_NAMES | {"bunmpc_fifth.h": rows})
    assert all(w in str(e.value) for w in words), str(e.value)


def test_a_define_repeated_with_its_value_is_no_error(tmp_path):
    _lib.read_headers(_tree(tmp_path, bunmpc_fifth="#define BMPC_BAD_ARG 1\n"), _lib.HEADER_NAMES | {"bunmpc_fifth.h": {}})
    assert _lib.BAD_ARG == 1


def test_the_knobs_are_the_setters_of_the_headers():
    assert sorted(_lib.KNOBS) == sorted(
        "certified_steps exact_step_decisions latency_mapping_max_batch loop_constants_in_lds steal_grid three_per_wave two_waves_per_simd "
        "work_stealing force_foot_pairs ik_all_steps ik_blocking_waits ik_calcdiff_one_wave_above ik_express_capacity ik_express_near "
        "ik_fused_direct_max ik_gains_wave_below ik_profile ik_spec_one_wave_above ik_speculative_below".split())
    assert all(_lib.KNOBS[k] == ("bmpc_ik_set_" + k[3:] if k.startswith("ik_") else "bmpc_set_" + k) for k in _lib.KNOBS)
    assert _lib._SIGS[_lib.KNOBS["ik_express_near"]] == (C.c_double, [C.c_double]) and "device" not in _lib.KNOBS
    with pytest.raises(TypeError, match="no_such_knob"):
        with _lib.knobs(three_per_wave=1, no_such_knob=0):
            pass
    with knob_setter() as set_, pytest.raises(TypeError, match="bmpc_set_device"):      # the fixture's calling form, by setter name
        set_("bmpc_set_device", 0)


def test_knobs_are_restored_when_the_block_raises():
    lib = _lib.lib()

    def current(setter, probe):
        old = setter(probe)
        setter(old)
        return old
    before = current(lib.bmpc_set_three_per_wave, 0), current(lib.bmpc_ik_set_express_near, 0.5)
    inside = 0 if before[0] else 1, before[1] + 0.25
    with pytest.raises(ZeroDivisionError):
        with _lib.knobs(three_per_wave=inside[0], ik_express_near=inside[1], two_waves_per_simd=1):
            assert (current(lib.bmpc_set_three_per_wave, 0), current(lib.bmpc_ik_set_express_near, 0.5)) == inside
            1 / 0
    assert (current(lib.bmpc_set_three_per_wave, 0), current(lib.bmpc_ik_set_express_near, 0.5)) == before


def _compiler():
    """the clang that ships beside hipcc (bin/amdclang, or lib/llvm/bin/clang of the same ROCm tree), else the system's cc"""
    rocm_bin = os.path.dirname(os.path.realpath(hip_build.HIPCC))
    for clang in (os.path.join(rocm_bin, "amdclang"), os.path.join(rocm_bin, "..", "lib", "llvm", "bin", "clang")):
        if os.path.exists(clang):
            return clang
    return shutil.which("cc")


@pytest.mark.parametrize("header", list(_lib.HEADERS))
def test_a_c_compiler_lays_the_structs_out_as_ctypes_does(tmp_path, header):
    """a C program prints sizeof of every struct and offsetof / sizeof of every field the reader found; a field the reader missed
    shows as a wrong sizeof or a shifted offset.  The header must also compile on its own as C and as C++."""
    cc = _compiler()
    if cc is None:
        pytest.skip("no C compiler on this machine")
    want, lines = [], []
    for cname, cls in _lib.HEADERS[header].structs.items():
        want.append("%s %d" % (cname, C.sizeof(cls)))
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            want.append("%s.%s %d %d" % (cname, field, getattr(cls, field).offset, getattr(cls, field).size))
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (cname, field, cname, field, cname, field))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n%s\nreturn 0;\n}\n' % (header, "\n".join(lines)))
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(tmp_path / "layout"), str(src)])
    got = subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")[:-1]
    assert got == want
    for lang in ("c", "c++"):
        subprocess.check_call([cc, "-x", lang, "-fsyntax-only", "-Wall", "-Werror", os.path.join(INCLUDE, header)])


def test_the_headers_compile_in_one_translation_unit(tmp_path):
    cc = _compiler()
    if cc is None:
        pytest.skip("no C compiler on this machine")
    src = tmp_path / "all.c"
    src.write_text("".join('#include "%s"\n' % h for h in _lib.HEADERS) + "int main(void) { return 0; }\n")
    subprocess.check_call([cc, "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-I", INCLUDE, str(src)])


# ---- the reader on small headers ----------------------------------------------------------------------------------------------------

def _fields(cls):
    return [(f, t, getattr(cls, f).offset) for f, t in cls._fields_]


def test_names_that_contain_a_qualifier():
    abi = _abi.parse("typedef struct { int status; const char *kernel; int loop_constants_in_lds; unsigned unsigned_count; } plan_t;\n"
                     "int set_loop_constants_in_lds(int loop_constants_in_lds, const plan_t *const constant_plan, long unsigned_n);\n")
    assert _fields(abi.structs["plan_t"]) == [("status", C.c_int, 0), ("kernel", C.c_char_p, 8), ("loop_constants_in_lds", C.c_int, 16),
                                              ("unsigned_count", C.c_uint, 20)]
    assert abi.functions == {"set_loop_constants_in_lds": (C.c_int, [C.c_int, C.c_void_p, C.c_long])}


def test_several_declarators_and_declarations_per_line():
    abi = _abi.parse("typedef struct { unsigned a, b; const double *x, *y; long n; int *p, q; } s_t;")
    assert _fields(abi.structs["s_t"]) == [("a", C.c_uint, 0), ("b", C.c_uint, 4), ("x", C.c_void_p, 8), ("y", C.c_void_p, 16),
                                           ("n", C.c_long, 24), ("p", C.c_void_p, 32), ("q", C.c_int, 40)]


def test_arrays():
    s = _abi.parse("typedef struct {\n  double m[4][2];   /* rows */\n  char k[24];\n  int f[4]; // feet\n} s_t;").structs["s_t"]
    assert [(f, C.sizeof(t), o) for f, t, o in _fields(s)] == [("m", 64, 0), ("k", 24, 64), ("f", 16, 88)]
    v = s()
    assert len(v.m) == 4 and len(v.m[0]) == 2 and s._fields_[1][1] is C.c_char * 24 and s._fields_[2][1] is C.c_int * 4
    v.k = b"ik_state"
    assert v.k == b"ik_state"


def test_nested_struct_by_value_and_class_names():
    abi = _abi.parse("typedef struct { int a; } in_t;\ntypedef struct { char c; in_t in; const in_t *ptr; } out_t;", names={"in_t": "In"})
    inner, outer = abi.structs["in_t"], abi.structs["out_t"]
    assert list(abi.structs) == ["in_t", "out_t"] and (inner.__name__, inner.__doc__, outer.__name__) == ("In", "in_t", "out_t")
    assert _fields(outer) == [("c", C.c_char, 0), ("in", inner, 4), ("ptr", C.c_void_p, 8)]


def test_prototypes():
    abi = _abi.parse("typedef struct h h_t;\n"
                     "const char *name_of(const char *key, int);\n"
                     "int version(void);\n"
                     "void destroy(h_t *h);\n"
                     "h_t *create(double m,\n            const double out3[3], long *offsets8, void *stream);\n"
                     "double mass(const h_t *h);\n")
    assert abi.structs == {} and abi.functions == {
        "name_of": (C.c_char_p, [C.c_char_p, C.c_int]), "version": (C.c_int, []), "destroy": (None, [C.c_void_p]),
        "create": (C.c_void_p, [C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]), "mass": (C.c_double, [C.c_void_p])}


def test_defines_and_the_cplusplus_wrapper():
    abi = _abi.parse("#ifndef X_H\n#define X_H\n#ifdef __cplusplus\nextern \"C\" {\n#endif\n#define X_OK 0\n#define X_MASK 0x10\n"
                     "#define X_L0 2.25e6   /* biconvex.cpp:20 */\n#define X_NOTHING\nint f(void);\n#ifdef __cplusplus\n}\n#endif\n#endif\n")
    assert abi.defines == {"X_OK": 0, "X_MASK": 16, "X_L0": 2.25e6} and type(abi.defines["X_OK"]) is int and list(abi.functions) == ["f"]


@pytest.mark.parametrize("text,word", [
    ("typedef struct { int a; int flag : 3; } s_t;", "int flag : 3"),                    # a bit-field
    ("typedef struct { later_t x; } s_t;\ntypedef struct { int a; } later_t;", "later_t"),   # a struct before its definition
    ("int f(const later_t *p);\ntypedef struct { int a; } later_t;", "later_t"),
    ("typedef struct h h_t;\ntypedef struct { h_t by_value; } s_t;", "h_t"),              # an opaque handle by value
    ("typedef struct { unsigned int a; } s_t;", "unsigned int a"),
    ("typedef struct { double m[]; } s_t;", "double m[]"),
    ("int f(unsigned int);", "unsigned int"),
    ("extern int f(void);", "extern int f(void)"),
    ("typedef int (*callback_t)(int);", "callback_t"),
    ("int x;", "int x"),
    ("int f(void)", "int f(void)"),                                                      # no semicolon
    ("#define TWICE(x) (2 * (x))\n", "TWICE"),
    ("#define X_NAME \"x\"\n", "X_NAME"),
    ("#include <stddef.h>\n", "#include"),
])
def test_what_the_reader_cannot_read_raises_and_names_it(text, word):
    with pytest.raises(_abi.HeaderError) as e:
        _abi.parse(text)
    assert word in str(e.value)


def test_the_header_has_no_workarounds_left():
    text = open(hip_build.INCLUDE).read()
    assert text.count("extern") == 1 and 'extern "C" {' in text and "BMPC_ADDITIVE" not in text
