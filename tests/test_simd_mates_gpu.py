"""The loop-constants build in workgroups of eight waves whose SIMD-mates keep level by priority (bmpc_set_simd_mate_balance; DESIGN.md
section 9 item 4; biconvex_admm_body.h: MATES).  A wave's problems, its LDS area, the workgroup's barrier and the mailbox are new; the
arithmetic is not, and priorities decide nothing but time -- so nothing may show in any output: mode 1 (and 3, the geometry without
the rule) against mode 0, the one-wave workgroups, by value (np.array_equal, NaN-aware) on X, F, P, stats, L_x, L_f, trace, hist,
dyn_viol and the certificate counts, with the helpers of tests/test_loop_constants_gpu.py.  The shapes are the smallest at which the
addressing, the barrier and the mailbox can go wrong: one full workgroup (16 problems), a second workgroup with one live wave (half-empty
and full) and seven waves that only meet the barrier, a workgroup that is not full, and the other record strides.  The setter and the
getter of the last launch's block size are exported but declared in no header: bound here."""
import ctypes as C

import numpy as np
import pytest

from bunmpc_amd import problems
from tests.test_loop_constants_gpu import KEYS, _same, _solve, knobs  # noqa: F401  (knobs: the fixture)
from tests.util import launch_record

pytestmark = pytest.mark.gpu


@pytest.fixture
def mates(hiplib, knobs):
    """set(mode): bmpc_set_simd_mate_balance for this test, restored afterwards; block(): threads per workgroup of the last launch"""
    setter, getter = hiplib.bmpc_set_simd_mate_balance, hiplib.bmpc_biconvex_last_block_size
    setter.argtypes, setter.restype, getter.argtypes, getter.restype = [C.c_int], C.c_int, [], C.c_int
    old = setter(0)
    try:
        yield setter, getter
    finally:
        setter(old)


def _modes(mates, solve, what=""):
    """solve() on one-wave workgroups (the returned run), on the eight-wave geometry with the rule and without it: every output equal"""
    set_, block = mates
    set_(0)
    ref = solve()
    assert block() == 64
    for mode in (1, 3):
        set_(mode)
        got = solve()
        assert block() == 512
        _same(got, ref, "%s mode %d" % (what, mode))
    set_(0)
    return ref


@pytest.mark.parametrize("B", [16, 17, 18, 1, 2, 15, 33])
def test_batch_sizes(mates, B):
    b = problems.make_batch("solo12_trot", B, H=20)
    ref = _modes(mates, lambda: _solve(b, num_iters=3), "B = %d" % B)
    assert np.all(ref["stats"][:, 5] == 0) and np.all(ref["stats"][:, 0] == 3)


@pytest.mark.parametrize("H", [16, 17])
def test_other_record_strides(mates, H):
    b = problems.make_batch("solo12_trot", 32, H=H)
    _modes(mates, lambda: _solve(b, num_iters=3), "H = %d" % H)


@pytest.mark.parametrize("maxit", [1, 2])
def test_iteration_caps(mates, maxit):
    b = problems.make_batch("solo12_trot", 18, H=20)
    ref = _modes(mates, lambda: _solve(b, num_iters=3, maxit=maxit))
    assert np.all(ref["stats"][:, 1] == 3 * maxit)


def test_exits_inside_the_loops(mates):
    b = problems.make_batch("solo12_trot", 18, H=20)
    ref = _modes(mates, lambda: _solve(b, num_iters=3, tol=1e-3))
    assert np.any(ref["stats"][:, 1:3] < 3 * 150)


def test_floor_hand_over(mates):
    """tol = 1e-30: every paired force phase replays on four feet and hands over to the tested loop"""
    b = problems.make_batch("solo12_trot", 18, H=20)
    _modes(mates, lambda: _solve(b, num_iters=2, tol=1e-30, maxit=4000))


def test_a_diverged_problem_as_wave_mate_and_as_simd_mate(mates):
    """problem 0 starts at a velocity of 1e200 and is NaN after two iterations: problem 1 shares its wave, and whichever wave shares its SIMD
    is one of the workgroup's other seven -- all of them return the bits of the clean batch"""
    clean = problems.make_batch("solo12_trot", 16, H=20)
    bad = problems.make_batch("solo12_trot", 16, H=20)
    bad.x_init[0, 3] = 1e200
    ref = _modes(mates, lambda: _solve(clean, num_iters=10), "clean")
    got = _modes(mates, lambda: _solve(bad, num_iters=10), "diverged")
    assert got["stats"][:, 5].tolist() == [2] + [0] * 15
    for k in KEYS:
        assert np.array_equal(got[k][1:], ref[k][1:], equal_nan=True), k
    assert np.all(np.isfinite(got["X"][1:]))


def test_warm_start_with_swing_forces(mates):
    """the warm start of tests/test_phase_setup_gpu.py: the first force phase is not eligible for two feet per lane"""
    b = problems.make_batch("solo12_trot", 18, H=20)
    c = _solve(b, num_iters=4)
    F = c["F"].reshape(18, 20, 4, 3).copy()
    F[:, :, :, 2] = np.where(b.cnt_plan[:, :, :, 0] == 0, 0.5, F[:, :, :, 2])
    warm = dict(warm=(c["X"], F.reshape(18, -1), c["P"]), L_x=c["L_x"], L_f=c["L_f"])
    _modes(mates, lambda: _solve(b, num_iters=3, **warm))


def test_mixed_gaits(mates):
    b = problems.make_batch("solo12_mixed", 32, H=20)
    _modes(mates, lambda: _solve(b, num_iters=3))


def test_the_launch_record_does_not_depend_on_the_mode(hiplib, mates):
    set_, block = mates
    b = problems.make_batch("solo12_trot", 16, H=20)
    set_(0)
    _solve(b, num_iters=1)
    one = launch_record(hiplib)
    set_(1)
    _solve(b, num_iters=1)
    assert launch_record(hiplib) == one == ("biconvex_admm_kernel", 32, 2)
    assert block() == 512


def test_when_it_pays_is_not_at_sixteen_problems(mates):
    """mode 2 takes the eight-wave geometry only where the batch fills the chip exactly once: B = 16 keeps one-wave workgroups"""
    set_, block = mates
    b = problems.make_batch("solo12_trot", 16, H=20)
    set_(2)
    _solve(b, num_iters=1)
    assert block() == 64
    set_(1)
    _solve(b, num_iters=1)
    assert block() == 512
