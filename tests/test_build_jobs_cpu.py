"""The build's job table (bunmpc_amd/build.py: compile_jobs, the one list of the library's objects), its staleness check, and the
symbol-wise comparison of tools/device_asm_diff.py on small synthetic listings.  No compiler runs here."""
import glob
import os
import sys

import pytest

from bunmpc_amd import build

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import device_asm_diff as dad  # noqa: E402


def test_compile_jobs_name_every_object_once():
    jobs = build.compile_jobs()
    names = [name for name, _, _ in jobs]
    assert len(set(names)) == len(names)
    assert len({build.object_path(j, build.FLAGS) for j in jobs}) == len(jobs)
    assert all(os.path.exists(os.path.join(build.CSRC, src)) for _, src, _ in jobs)
    assert {src for _, src, _ in jobs} == {os.path.basename(p) for p in glob.glob(os.path.join(build.CSRC, "*.hip"))}
    # the centroidal units: twelve compilations of one source, the first in the list, no two with the same defines
    units = [j for j in jobs if j[1] == "biconvex_admm.hip"]
    assert units == jobs[:12]
    defines = [frozenset(f for f in flags if f.startswith("-D")) for _, _, flags in units]
    assert all(len(d) == 3 for d in defines) and len(set(defines)) == len(units)
    assert build.job("ik_ddp") == ("ik_ddp", "ik_ddp.hip", ["-ffp-contract=on"])


def test_object_path_follows_the_flags():
    j = build.job("admm_diag_f32_e2")
    assert build.object_path(j, build.FLAGS) != build.object_path(j, build.FLAGS + ["-DBWD_PROFILE"])
    assert build.object_path(j, build.FLAGS) != build.object_path((j[0], j[1], j[2] + ["-g"]), build.FLAGS)


def test_new_header_makes_the_library_stale(tmp_path, monkeypatch):
    """a header that no list names: every *.h under csrc/ is a dependency"""
    csrc = tmp_path / "pkg" / "csrc"
    csrc.mkdir(parents=True)
    for _, src, _ in build.compile_jobs():
        (csrc / src).write_text("")
    (csrc / "old.h").write_text("")
    include = tmp_path / "bunmpc.h"
    include.write_text("")
    lib = tmp_path / "pkg" / "libbunmpc_hip.so"
    monkeypatch.setattr(build, "CSRC", str(csrc))
    monkeypatch.setattr(build, "OBJ", str(csrc / "_obj"))
    monkeypatch.setattr(build, "INCLUDE", str(include))
    monkeypatch.setattr(build, "LIB", str(lib))
    assert build.is_stale()                                  # no library
    lib.write_text("")
    t = os.path.getmtime(build.__file__)                     # (build.py is a dependency itself: every time below is set, relative to its own)
    for d in build.dependencies():
        if d.startswith(str(tmp_path)):
            os.utime(d, (t - 100, t - 100))
    os.utime(lib, (t + 100, t + 100))
    assert not build.is_stale()
    (csrc / "new_shape.h").write_text("")
    os.utime(csrc / "new_shape.h", (t + 200, t + 200))
    assert build.is_stale()
    os.utime(csrc / "new_shape.h", (t - 100, t - 100))
    assert not build.is_stale()
    os.utime(include, (t + 200, t + 200))
    assert build.is_stale()


def listing(kernels):
    """a hipcc -S listing in miniature: kernels = [(symbol, function index, instruction)]"""
    text = "\t.text\n"
    for name, n, inst in kernels:
        text += ("\t.globl\t%(k)s\n%(k)s:                                   ; @%(k)s\n; %%bb.0:\n\ts_load_dword s0, s[0:1], 0x0\n"
                 ".LBB%(n)d_1:                                ; =>This Inner Loop Header: Depth=1\n\t%(i)s\n\ts_cbranch_scc1 .LBB%(n)d_1\n"
                 "\ts_endpgm\n\t.section\t.rodata\n\t.amdhsa_kernel %(k)s\n\t\t.amdhsa_next_free_vgpr 4\n\t.end_amdhsa_kernel\n\t.text\n"
                 ".Lfunc_end%(n)d:\n") % {"k": name, "n": n, "i": inst}
    text += "\t.amdgpu_metadata\n---\namdhsa.kernels:\n"
    for name, _, _ in kernels:
        text += "  - .args:           []\n    .name:           %s\n    .vgpr_count:     4\n" % name
    return text + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n"


def test_kernels_compared_by_symbol_over_the_tree(tmp_path):
    files = {"p_a": listing([("k_moves", 0, "v_add_f64 v[0:1], v[0:1], v[2:3]"), ("k_stays", 1, "v_mul_f64 v[0:1], v[0:1], v[2:3]"),
                             ("k_changes", 2, "v_fma_f64 v[0:1], v[0:1], v[2:3], v[0:1]"), ("k_leaves", 3, "s_nop 0")]),
             "p_host": "\t.text\n",
             "t_a": listing([("k_changes", 0, "v_fma_f64 v[0:1], v[2:3], v[0:1], v[0:1]"), ("k_stays", 1, "v_mul_f64 v[0:1], v[0:1], v[2:3]")]),
             "t_b": listing([("k_comes", 0, "s_nop 1"), ("k_moves", 7, "v_add_f64 v[0:1], v[0:1], v[2:3]")])}
    for name, text in files.items():
        (tmp_path / name).write_text(text)
    assert set(dad.kernels_of(str(tmp_path / "p_a"))) == {"k_moves", "k_stays", "k_changes", "k_leaves"}
    assert dad.kernels_of(str(tmp_path / "p_host")) == {}
    assert "LBB7" not in dad.kernels_of(str(tmp_path / "t_b"))["k_moves"] and "Loop Header" not in dad.kernels_of(str(tmp_path / "t_b"))["k_moves"]
    parent = dad.kernels_of_tree([("a", str(tmp_path / "p_a")), ("host", str(tmp_path / "p_host"))])
    this = dad.kernels_of_tree([("a", str(tmp_path / "t_a")), ("b", str(tmp_path / "t_b"))])
    assert dad.compare(parent, this) == [
        ("k_changes", "a", "a", "DIFFERS"),
        ("k_comes", None, "b", "DIFFERS (only in the this tree)"),
        ("k_leaves", "a", None, "DIFFERS (only in the parent tree)"),
        ("k_moves", "a", "b", "same"),                  # another unit, another function index in its labels
        ("k_stays", "a", "a", "same"),
    ]
    assert all(v == "same" for _, _, _, v in dad.compare(parent, parent))
    with pytest.raises(ValueError):                   # one symbol in two units of a tree
        dad.kernels_of_tree([("a", str(tmp_path / "p_a")), ("again", str(tmp_path / "p_a"))])
