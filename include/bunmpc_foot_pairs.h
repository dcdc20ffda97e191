/* bunmpc_foot_pairs.h -- the switch and the telemetry of the headline kernel's force loop with two feet per lane: the fourth header of
 * libbunmpc_hip.so.  A header of its own, as bunmpc_turn.h and bunmpc_goals.h are: the table of bunmpc.h (tests/golden/abi.json) is held
 * to its recorded size by tests/test_abi_cpu.py, so what is added to the library's interface is declared beside it.  It includes
 * nothing; bunmpc_amd/_lib.py reads it with the reader of bunmpc.h.
 *
 * The loop-constants build of the benchmark's kernel (bmpc_set_loop_constants_in_lds in bunmpc.h; DESIGN.md section 4, "Force loop: two
 * feet per lane"): a swing foot's force is +0 throughout a certified force loop, so a force phase whose two problems need at most 32
 * lanes each with two contact feet per lane, and whose swing feet start at +0.0, runs on the contact feet alone; every other phase runs
 * the four-feet loop.  Same values in every output (a sum that is an exact zero could at most differ in sign; none does, see
 * tests/test_foot_pairs_cpu.py). */
#ifndef BUNMPC_FOOT_PAIRS_H
#define BUNMPC_FOOT_PAIRS_H
#ifdef __cplusplus
extern "C" {
#endif

/* mode 0: never; 1: in every eligible phase; 2 (default): when it pays -- which the measurement recorded in EXPERIMENTS.md ("Headline
 * force loop: two feet per lane": B = 4096, n_col = 20, 2.40 -> 2.21 ms) resolves to "in every eligible phase".  Returns the old value. */
int bmpc_set_force_foot_pairs(int mode);
/* Telemetry: how many (wave, force phase) pairs ran that loop on the current device since the last reset (reset != 0: the count is
 * returned and set to 0).  A wave counts a phase only if both its problems were eligible.  A wave that holds a non-finite iterate -- a
 * diverged wave-mate's, dead or alive, its last knot's included -- is not eligible in that phase or any later one: it counts nothing from
 * there on, at every horizon (before the unit map was made once per solve such a wave could still count phases at horizons below 20
 * knots).  Outputs do not depend on which loop ran.  Waits for the device; -1 on error. */
long bmpc_force_foot_pair_phases(int reset);

#ifdef __cplusplus
}
#endif
#endif
