"""The scalar side of the headline kernel's certified loops ("Certified loops: scalar diet"), as far as a CPU can
check it: the LDS bank model's verdict on where the loop constants lie, and the rule that replaced the per-iteration counters -- a
problem's FISTA iteration count is the index at which its bit left `act`, or the index at which the loop ended."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


bank = _tool("lds_bank_model")


# ---------------------------------------------------------------- the bank model itself
def test_model_counts_the_textbook_cases():
    """unit stride of doubles: conflict-free in both instructions; every lane on one bank with distinct addresses: a group's lanes less one
    per group; one address for all: a broadcast; lanes that are off take no part"""
    unit = [2 * k for k in range(64)]
    assert bank.conflict_cycles("ds_read_b64", unit) == 0 and bank.conflict_cycles("ds_read2_b64", unit) == 0
    same_bank = [64 * k for k in range(64)]
    assert bank.conflict_cycles("ds_read_b64", same_bank) == 2 * 31
    assert bank.conflict_cycles("ds_read2_b64", same_bank) == 4 * 15
    assert bank.conflict_cycles("ds_read_b64", [640] * 64) == 0
    assert bank.conflict_cycles("ds_read_b64", [64 * k if k % 32 == 0 else None for k in range(64)]) == 0
    # a stride of 32 dwords meets itself in ds_read2_b64's 32 banks and not in ds_read_b64's 64 until the third lane
    assert bank.conflict_cycles("ds_read2_b64", [0, 32] + [None] * 62) == 1
    assert bank.conflict_cycles("ds_read_b64", [0, 32] + [None] * 62) == 0


def test_constants_match_the_kernel_headers():
    text = open(os.path.join(ROOT, "bunmpc_amd", "csrc", "biconvex_kernels.h")).read()
    for name, value in (("kLdsZeros", bank.K_LDS_ZEROS), ("kSegLds", bank.K_SEG_LDS), ("kLoopConstLds", bank.K_LOOP_CONST)):
        assert "constexpr int %s = %d;" % (name, value) in text, name
    assert "constexpr int knot_lds(int E) { return 27 + 3 * E; }" in text


# ---------------------------------------------------------------- its verdict on the two layouts
@pytest.mark.parametrize("H", range(16, 21))
@pytest.mark.parametrize("loop", ["motion", "force"])
def test_chosen_layout_is_conflict_free(H, loop):
    for alive in ((True, True), (True, False)):
        assert bank.iteration_conflicts(H, loop, "chosen", segments_alive=alive) == 0, alive
    assert bank.zeros_read_are_zeros(H, "chosen")


def test_parent_layout_conflicts_as_measured():
    """every idle lane at element 0: the model must find the conflicts the counters found (49.4 K cycles per wave over about 2 549
    iterations at H = 20, 19.4 per iteration), or it is wrong"""
    m, f = bank.iteration_conflicts(20, "motion", "parent"), bank.iteration_conflicts(20, "force", "parent")
    assert m > 0 and f > 0
    assert 17.0 <= min(m, f) and max(m, f) <= 21.0, (m, f)      # (whatever the split of the iterations between the loops)
    assert any(bank.iteration_conflicts(H, loop, "parent") > 0 for H in range(16, 21) for loop in ("motion", "force"))


def test_no_lds_is_added():
    """the wave's LDS at H = 20, four feet: 20 160 bytes, under the 20 480 that let eight waves share a CU; the idle lanes' reads end
    inside the zeros"""
    assert 8 * (bank.K_LDS_ZEROS + 2 * (bank.K_SEG_LDS + 21 * bank.knot_lds(4)) + 2 * 21 * bank.K_LOOP_CONST) == 20160
    assert 31 + bank.K_LOOP_CONST <= bank.K_LDS_ZEROS


# ---------------------------------------------------------------- iteration counts from the exit index
def _per_iteration(done, act0, maxit, hand_over_at):
    """the counters the loops kept: one increment per iteration and problem whose bit is in `act` at its end"""
    act, n = act0.copy(), np.zeros(2, int)
    for i in range(maxit):
        if not act.any():
            break
        if i == hand_over_at:      # nothing of this iteration is kept
            return n, act, i
        n += act
        act &= ~done[i]
    return n, act, maxit


def _from_exit(done, act0, maxit, hand_over_at):
    """the kernel's rule: c[p] = i + 1 where problem p's bit falls, and the problems still in `act` behind the loop get the index at
    which it ended (i0: the hand-over's iteration, or maxit)"""
    act, c, i0 = act0.copy(), np.zeros(2, int), maxit
    if act.any() and maxit > 0:
        i = 0
        while True:
            if i == hand_over_at:
                i0 = i
                break
            latch = act & done[i]
            if latch.any():
                c[latch] = i + 1
                act &= ~done[i]
                if not act.any():
                    break
            i += 1
            if i >= maxit:
                break
    return np.where(act, i0, c), act, i0


def _check(done, act0, maxit, hand_over_at=-1):
    a, b = _per_iteration(done, act0, maxit, hand_over_at), _from_exit(done, act0, maxit, hand_over_at)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (done[:maxit].tolist(), act0, maxit, hand_over_at, a, b)
    if a[1].any():      # (with nobody left the index at which the loop ended is not used)
        assert a[2] == b[2]
    return a[0]


def test_iteration_count_named_cases():
    maxit = 7
    never = np.zeros((maxit, 2), bool)
    both = np.array([True, True])
    assert _check(never, both, maxit).tolist() == [7, 7]                                   # never: the loop ends by maxit
    d = never.copy(); d[0, 0] = True
    assert _check(d, both, maxit).tolist() == [1, 7]                                       # an exit at iteration 0
    d = never.copy(); d[maxit - 1, 1] = True
    assert _check(d, both, maxit).tolist() == [7, 7]                                       # an exit at exactly maxit - 1
    d = never.copy(); d[3] = True
    assert _check(d, both, maxit).tolist() == [4, 4]                                       # both problems in the same iteration
    d = never.copy(); d[2, 0] = True; d[5, 1] = True
    assert _check(d, both, maxit).tolist() == [3, 6]
    assert _check(d, both, maxit, hand_over_at=4).tolist() == [3, 4]                       # a hand-over: the wave-mate has the loop's end
    assert _check(d, both, maxit, hand_over_at=0).tolist() == [0, 0]
    assert _check(d, np.array([False, True]), maxit).tolist() == [0, 6]                    # a segment without a problem
    assert _check(d, np.array([False, False]), maxit).tolist() == [0, 0]
    assert _check(never, both, 0).tolist() == [0, 0]
    d = never.copy(); d[:, 0] = True      # done bits of a problem that has left (or never was there) stay without effect
    assert _check(d, both, maxit).tolist() == [1, 7]


def test_iteration_count_random_sequences():
    rng = np.random.default_rng(7)
    for _ in range(4000):
        maxit = int(rng.integers(0, 9))
        done = rng.random((max(maxit, 1), 2)) < rng.choice([0.0, 0.05, 0.3, 1.0])
        act0 = rng.random(2) < 0.8
        hand = int(rng.integers(0, maxit)) if maxit and rng.random() < 0.3 else -1
        _check(done, act0, maxit, hand)
