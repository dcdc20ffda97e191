"""Generates tests/golden/biped_walk_b4_it10.npz: seeded inputs of the synthetic biped (bunmpc_amd.problems.make_batch("biped_walk"),
n_eff = 2) and the outputs of the strict C restatement (oracle/biconvex_oracle.c) on them, in the format of make_golden.py's
centroidal fixtures.

NOT reference outputs (parity unpinned, as make_golden.py explains): the fixture freezes the oracle's behaviour on two-footed
problems, so that the GPU tests of the biped kernels have inputs / outputs that do not depend on building the oracle.

Run from the repo root:  python tests/golden/make_golden_biped.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from bunmpc_amd import problems  # noqa: E402
from oracle import oracle_c  # noqa: E402

CASES = [  # name, config, B, num_iters
    ("biped_walk_b4_it10", "biped_walk", 4, 10),
]


def fixture(config, B, iters):
    """the arrays of one fixture (what the CPU test compares with the committed file)"""
    b = problems.make_batch(config, B)
    r = oracle_c.solve_batch(b, num_iters=iters)
    return dict(config=config, num_iters=iters, m=b.m, rho=b.rho, mu=b.mu, cnt_plan=b.cnt_plan, dt=b.dt, x_init=b.x_init,
                X_nom=b.X_nom, X_ter=b.X_ter, W_X=b.W_X, W_X_ter=b.W_X_ter, W_F=b.W_F, bounds=b.bounds,
                X=r["X"], F=r["F"], P=r["P"], L_x=r["L_x"], L_f=r["L_f"], stats=r["stats"])


def main():
    out_dir = os.path.dirname(os.path.abspath(__file__))
    for name, config, B, iters in CASES:
        f = fixture(config, B, iters)
        np.savez_compressed(os.path.join(out_dir, name + ".npz"), **f)
        print(name, "stats", f["stats"].tolist())


if __name__ == "__main__":
    main()
