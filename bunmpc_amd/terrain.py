"""Terrain height maps (numpy, no GPU): a regular grid of heights with bilinear interpolation, the object the reference's
harness takes as `height_map` (duck-typed: `getHeight(x, y)`, abstract_cyclic_gen.py:333-337, 370-374), plus the unit surface
normal the Euclidean friction cones need (`getNormal`).

The arithmetic below is the contract: csrc/plan_gen.hip repeats it operation for operation (separate multiplies and adds, no
contraction), and the tests compare the two bit for bit.  Node (iy, ix) of Z sits at (x0 + ix cell, y0 + iy cell):
    u = (x - x0) / cell, v = (y - y0) / cell, clamped to [0, nx - 1] / [0, ny - 1]   (outside the map: the border's height)
    ix = min(int(floor(u)), nx - 2), a = u - ix; iy, b likewise
    d0 = z10 - z00, d1 = z11 - z01                      (z<ix offset><iy offset>: z10 is one node further in x)
    h0 = z00 + a d0, h1 = z01 + a d1, h = h0 + b (h1 - h0)
    gx = (d0 + b (d1 - d0)) / cell, gy = (h1 - h0) / cell
    r = sqrt((gx gx + gy gy) + 1), n = (-gx / r, -gy / r, 1 / r)
The clamp comes before the conversion to an integer (and ignores NaN: fmax / fmin), so every index is in range for any x, y.
"""
import numpy as np

MAX_NODES = 4096      # per axis, as the device entry points (include/bunmpc.h: bmpc_terrain_t)


class HeightMap:
    """Z (ny, nx): one terrain; Z (B, ny, nx): one terrain per problem of a batch."""

    def __init__(self, x0, y0, cell, Z):
        Z = np.array(Z, dtype=np.float64, order="C")      # (a copy: the map does not change under its user)
        if Z.ndim not in (2, 3):
            raise ValueError("HeightMap: Z must be (ny, nx) or (B, ny, nx), got shape %s" % (Z.shape,))
        ny, nx = Z.shape[-2:]
        if not (2 <= nx <= MAX_NODES and 2 <= ny <= MAX_NODES):
            raise ValueError("HeightMap: nx and ny must be in [2, %d], got nx = %d, ny = %d" % (MAX_NODES, nx, ny))
        x0, y0, cell = float(x0), float(y0), float(cell)
        if not (np.isfinite(cell) and cell > 0.0):
            raise ValueError("HeightMap: cell must be finite and > 0, got %r" % (cell,))
        if not (np.isfinite(x0) and np.isfinite(y0)):
            raise ValueError("HeightMap: x0 and y0 must be finite, got %r, %r" % (x0, y0))
        if not np.all(np.isfinite(Z)):
            raise ValueError("HeightMap: heights must be finite")
        self.x0, self.y0, self.cell, self.Z = x0, y0, cell, Z
        self.nx, self.ny = nx, ny
        self.per_problem = Z.ndim == 3
        self.B = Z.shape[0] if self.per_problem else None

    # ---- builders ----------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_function(cls, f, x0=-1.0, y0=-1.0, cell=0.02, nx=128, ny=128):
        """Z[iy, ix] = f(x, y) at the nodes (f vectorised over arrays)"""
        x = x0 + np.arange(nx) * cell
        y = y0 + np.arange(ny) * cell
        X, Y = np.meshgrid(x, y)
        return cls(x0, y0, cell, np.broadcast_to(np.asarray(f(X, Y), dtype=np.float64), (ny, nx)))

    @classmethod
    def plane(cls, roll, pitch, z0=0.0, **grid):
        """The plane through (0, 0, z0) with normal R_y(pitch) R_x(roll) e_z (problems.plane_normals' convention), radians"""
        n = np.array([np.sin(pitch) * np.cos(roll), -np.sin(roll), np.cos(pitch) * np.cos(roll)])
        return cls.from_function(lambda x, y: z0 - (n[0] * x + n[1] * y) / n[2], **grid)

    @classmethod
    def stairs(cls, rise, run, x_start=0.0, z0=0.0, **grid):
        """Steps of height `rise` every `run` metres along x from x_start on (flat before it); between two nodes either side of an
        edge the bilinear surface is a ramp one cell long"""
        return cls.from_function(lambda x, y: z0 + rise * np.maximum(np.floor((x - x_start) / run + 1e-9) + 1.0, 0.0), **grid)

    # ---- evaluation --------------------------------------------------------------------------------------------------------------
    def _cell(self, x, y, problem):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        u = np.fmin(np.fmax((x - self.x0) / self.cell, 0.0), float(self.nx - 1))
        v = np.fmin(np.fmax((y - self.y0) / self.cell, 0.0), float(self.ny - 1))
        ix = np.minimum(np.floor(u).astype(np.int64), self.nx - 2)
        iy = np.minimum(np.floor(v).astype(np.int64), self.ny - 2)
        a, b = u - ix, v - iy
        if self.per_problem:
            if problem is None:      # the leading axis of x is the problem axis
                if x.ndim == 0 or x.shape[0] != self.B:
                    raise ValueError("HeightMap of %d terrains: x needs a leading axis of that length, or problem=" % self.B)
                problem = np.arange(self.B).reshape((self.B,) + (1,) * (x.ndim - 1))
            p = np.asarray(problem, dtype=np.int64)
            if np.any(p < 0) or np.any(p >= self.B):
                raise ValueError("HeightMap: problem index outside [0, %d)" % self.B)
            Z = lambda jy, jx: self.Z[p, jy, jx]      # noqa: E731
        else:
            Z = lambda jy, jx: self.Z[jy, jx]         # noqa: E731
        return a, b, Z(iy, ix), Z(iy, ix + 1), Z(iy + 1, ix), Z(iy + 1, ix + 1)

    def _eval(self, x, y, problem):
        a, b, z00, z10, z01, z11 = self._cell(x, y, problem)
        d0, d1 = z10 - z00, z11 - z01
        h0 = z00 + a * d0
        h1 = z01 + a * d1
        dh = h1 - h0
        h = h0 + b * dh
        gx = (d0 + b * (d1 - d0)) / self.cell
        gy = dh / self.cell
        return h, gx, gy

    def getHeight(self, x, y, problem=None):
        """bilinear height at (x, y); arrays of one shape.  problem: index of the terrain, per point, for a (B, ny, nx) map (default:
        the leading axis of x)"""
        return self._eval(x, y, problem)[0]

    def getNormal(self, x, y, problem=None):
        """unit normal of the bilinear surface at (x, y): shape of x + (3,)"""
        _, gx, gy = self._eval(x, y, problem)
        r = np.sqrt((gx * gx + gy * gy) + 1.0)
        return np.stack([-gx / r, -gy / r, 1.0 / r], axis=-1)
