"""CPU restatement of the centroidal solve with a NON-diagonal Q (test infrastructure, like oracle/oracle_np.py, which it extends):
function::ProblemData with the whole matrix in its gradient and objective difference, problem.cpp:31-56 formula by formula.
oracle_np's Fista, soc_projection, build_A_x, build_A_f and ADMM loop are used as they are: biconvex_solve constructs `Problem` by
its module-level name, which is swapped for the call."""
import numpy as np
import scipy.sparse as sp

from oracle import oracle_np


class BlockProblem(oracle_np.Problem):
    """ProblemData with a general symmetric Q, held sparse (the reference's Eigen::SparseMatrix) or dense: two accumulation orders"""
    sparse = True

    def __init__(self, Q, q, lb=None, ub=None):
        super().__init__(None, q, lb, ub)
        self.Q = sp.csr_matrix(Q) if self.sparse else np.asarray(Q, dtype=np.float64)

    def set_data(self, A, b, P, rho):      # problem.cpp:31-45: ATA = 2 (Q + rho A'A), ATbPk = 2 rho A'(-b + P) + q
        self.A, self.rho = A, rho
        AtA = A.T @ A
        self.ATA = 2.0 * (self.Q + rho * AtA) if self.sparse else sp.csr_matrix(2.0 * (self.Q + rho * AtA.toarray()))
        self.bPk = -b + P
        self.ATbPk = 2.0 * rho * (A.T @ self.bPk) + self.q

    def obj_diff(self, y1, y0):             # problem.cpp:47-56: (y1 + y0)'Q (y1 - y0) + q'(y1 - y0) + rho (|A y1 + bPk|^2 - |A y0 + bPk|^2)
        d = y1 - y0
        return (y1 + y0) @ (self.Q @ d) + self.q @ d + self.rho * (
            np.sum((self.A @ y1 + self.bPk) ** 2) - np.sum((self.A @ y0 + self.bPk) ** 2))


class DenseBlockProblem(BlockProblem):
    sparse = False


def biconvex_solve(cnt_plan, dt, m, x_init, Qx, qx, Qf, lbx, ubx, X, F, P, sparse=True, **kw):
    """oracle_np.biconvex_solve with Qx (nx, nx) and Qf (nf, nf) dense square matrices"""
    orig = oracle_np.Problem
    oracle_np.Problem = BlockProblem if sparse else DenseBlockProblem
    try:
        return oracle_np.biconvex_solve(cnt_plan, dt, m, x_init, np.asarray(Qx, float), qx, np.asarray(Qf, float), lbx, ubx, X, F, P, **kw)
    finally:
        oracle_np.Problem = orig


def solve_problem(b, i, raw, blk, iters, warm=None, L_x=2.25e6, L_f=506.25, sparse=True):
    """problem i of batch b with the raw bounds of `raw` and the block costs of `blk` (problems.block_costs), cold or from warm = (X, F, P)"""
    from bunmpc_amd import problems
    X0, F0, P0 = b.warm_start() if warm is None else warm
    return biconvex_solve(b.cnt_plan[i], b.dt[i], b.m, b.x_init[i], problems.block_diag_matrix(blk["Qx_blk"][i]), blk["qx"][i],
                          problems.block_diag_matrix(blk["Qf_blk"][i]), raw["lbx"][i], raw["ubx"][i], X0[i], F0[i], P0[i],
                          sparse=sparse, L_x=L_x, L_f=L_f, rho=b.rho, mu=b.mu, num_iters=iters)
