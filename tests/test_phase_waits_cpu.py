"""tools/phase_waits.py: its parser and its counts on small hand-written listings in hipcc's format -- one loop at two depths each: one
with a masked single-read block, one with a batch read unconditionally, one with a scratch reload between a batch of global loads and
their first use."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pw():
    spec = importlib.util.spec_from_file_location("phase_waits", os.path.join(ROOT, "tools", "phase_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


HEAD = """\t.text
_Z6kernelv:                             ; @_Z6kernelv
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v1, 0
\tscratch_store_dword off, v0, off ; 4-byte Folded Spill
.LBB0_1:                                ; =>This Loop Header: Depth=1
                                        ;     Child Loop BB0_4 Depth 2
"""
INNER = """.LBB0_4:                                ;   Parent Loop BB0_1 Depth=1
                                        ; =>  This Inner Loop Header: Depth=2
\tv_fma_f64 v[2:3], v[4:5], v[6:7], v[2:3]
\tds_read_b64 v[8:9], v1 offset:8
\ts_waitcnt lgkmcnt(0)
\tv_add_f64 v[2:3], v[2:3], v[8:9]
\ts_cbranch_scc1 .LBB0_4
; %bb.5:                                ;   in Loop: Header=BB0_1 Depth=1
\tglobal_store_dwordx2 v1, v[2:3], s[0:1]
\ts_cbranch_scc1 .LBB0_1
; %bb.6:
\ts_endpgm
.Lfunc_end0:
\t.size\t_Z6kernelv, .Lfunc_end0-_Z6kernelv
"""
# two elements read as `ok ? p[l] : 0`: an exec-masked block each, with the address reloaded and waited for in it
MASKED = HEAD + """\ts_and_saveexec_b64 s[2:3], s[8:9]
\ts_cbranch_execz .LBB0_3
; %bb.2:                                ;   in Loop: Header=BB0_1 Depth=1
\tscratch_load_dword v1, off, off       ; 4-byte Folded Reload
\ts_waitcnt vmcnt(0)
\tds_read_b64 v[4:5], v1 offset:16
.LBB0_3:                                ;   in Loop: Header=BB0_1 Depth=1
\ts_or_b64 exec, exec, s[2:3]
\ts_and_saveexec_b64 s[2:3], s[8:9]
\ts_cbranch_execz .LBB0_7
; %bb.8:                                ;   in Loop: Header=BB0_1 Depth=1
\tglobal_load_dwordx2 v[6:7], v[10:11], off
\ts_waitcnt vmcnt(0)
\tv_add_f64 v[6:7], v[6:7], -v[4:5]
.LBB0_7:                                ;   in Loop: Header=BB0_1 Depth=1
\ts_or_b64 exec, exec, s[2:3]
\ts_waitcnt lgkmcnt(0)
""" + INNER
# the same two elements and two more as one batch, one wait each counter, selects behind
BATCH = HEAD + """\tds_read2_b64 v[4:7], v1 offset0:2 offset1:3
\tds_read_b64 v[12:13], v1 offset:32
\tglobal_load_dwordx4 v[14:17], v10, s[0:1]
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tv_cndmask_b32_e64 v4, 0, v4, s[8:9]
\tv_cndmask_b32_e64 v5, 0, v5, s[8:9]
""" + INNER
# a batch of global loads, then a scratch reload whose vmcnt(0) waits for the whole batch in front of an LDS access; the masked block
# behind it holds a store, not a single read
RELOAD = HEAD + """\tglobal_load_dwordx4 v[14:17], v10, s[0:1]
\tglobal_load_dwordx4 v[18:21], v10, s[0:1] offset:16
\tglobal_load_dwordx2 v[22:23], v10, s[0:1] offset:32
\tscratch_load_dword v1, off, off       ; 4-byte Folded Reload
\ts_waitcnt vmcnt(0)
\tds_read_b64 v[4:5], v1 offset:16
\ts_and_saveexec_b64 s[2:3], s[8:9]
\ts_cbranch_execz .LBB0_3
; %bb.2:                                ;   in Loop: Header=BB0_1 Depth=1
\tds_read_b64 v[6:7], v1 offset:24
\ts_waitcnt lgkmcnt(0)
\tds_write_b64 v1, v[6:7] offset:24
.LBB0_3:                                ;   in Loop: Header=BB0_1 Depth=1
\ts_or_b64 exec, exec, s[2:3]
""" + INNER


def _analyse(pw, text):
    body = pw.kernel_body(text.split("\n"), "kernel")
    per_level, per_loop, blocks = pw.analyse(body)
    return per_level, per_loop, blocks


def test_levels_and_loops_are_told_apart(pw):
    per_level, per_loop, blocks = _analyse(pw, MASKED)
    assert sorted(per_level) == [0, 1, 2]
    assert [k for k in per_loop] == [(0, None), (1, "BB0_1"), (2, "BB0_4")]
    assert per_level[0]["blocks"] == 3 and per_level[0]["scratch_st"] == 1 and per_level[0]["instr"] == 4      # entry, %bb.0, %bb.6
    inner = per_level[2]
    assert (inner["blocks"], inner["instr"], inner["valu"], inner["lds"], inner["wait_lgkm"], inner["wait_vm"]) == (1, 5, 2, 1, 1, 0)
    assert per_level[1]["global_st"] == 1 and per_level[2]["global_st"] == 0      # (%bb.5 behind the inner loop is the outer loop's)


def test_masked_single_read_blocks(pw):
    per_level, _, blocks = _analyse(pw, MASKED)
    one = per_level[1]
    assert one["masked_single_reads"] == 2 and per_level[0]["masked_single_reads"] == 0 and per_level[2]["masked_single_reads"] == 0
    assert (one["blocks"], one["scratch_ld"], one["global_ld"], one["lds"], one["wait_vm"], one["wait_lgkm"]) == (6, 1, 1, 1, 2, 1)
    assert one["valu"] == 1
    assert pw.memseq(blocks, 1) == "rWdLWw/s"


def test_a_batch_has_none(pw):
    per_level, _, blocks = _analyse(pw, BATCH)
    one = per_level[1]
    assert one["masked_single_reads"] == 0
    assert (one["blocks"], one["scratch_ld"], one["global_ld"], one["lds"], one["wait_vm"], one["wait_lgkm"], one["valu"]) == (2, 0, 1, 2, 1, 1, 2)
    assert pw.memseq(blocks, 1) == "dLW/s"      # (a wait on both counters shows as W)


def test_a_reload_between_a_batch_and_its_use(pw):
    per_level, _, blocks = _analyse(pw, RELOAD)
    one = per_level[1]
    assert one["masked_single_reads"] == 0      # (the masked block reads AND writes: a read-modify-write, not a single read)
    assert (one["global_ld"], one["scratch_ld"], one["wait_vm"], one["lds"], one["wait_lgkm"]) == (3, 1, 1, 3, 1)
    seq = pw.memseq(blocks, 1)
    assert seq == "LLLrWdwd/s" and "LrW" in seq      # the reload's wait stands behind the whole run of loads; the write behind the w is a run of its own
    assert pw.memseq(blocks, 2) == "dw" and pw.memseq(blocks, 0) == "p"
