"""Writes tests/golden/lie_ref.npz: the SE(3) primitives of bunmpc_amd/csrc/rbd_device.h (and of oracle/rbd_np.py) at their edges, evaluated
from their definitions with mpmath at 60 digits -- no series cut-over, no float64 anywhere between input and output -- and rounded once.
Needs mpmath; the tests that read the file do not.        python tests/golden/make_golden_lie.py

Per op (tests/lie_ref.py: OPS) the file holds <op>_in [n][in], <op>_ref [n][ref], <op>_unit, and for the rows whose axis sign is free
<op>_alt_rows (their indices) and <op>_alt (the reference with the other sign).

The unit of a row is what any float64 routine is allowed there:
    unit = 2^-52 max|ref row| + max_j sum_i |f_j(x + ulp(x_i) e_i) - f_j(x)|
(one rounding of the largest output, plus what the last bit of each input moves the outputs by, evaluated in mp; where the axis sign
is free, see below, the move is measured to the nearer of the two signs, so that a branch flip never counts as a move).  For the three
elementary ops it is ulp(ref) per output; sincos adds |k| |pi/2 - (c1 + c2)|, k = rint(2 x / pi), c1 and c2 the two literals of
sincos_fast's Cody-Waite reduction: the reduction's own residual, the price of stopping at two pieces (domain |x| <= 1e5).

Definitions.  exp: Rodrigues' closed forms; a coefficient that cancels (1 - cos t, t - sin t, ...) is evaluated with 8 more digits per
decimal digit that t lies below 1, so the closed form serves down to the smallest subnormal; t = 0 takes the limit.  log: the angle
2 atan2(|v|, w) of the normalised relative quaternion (v, w), w >= 0, along v.  Jacobians: the closed forms of jexp3, jlog3, Barfoot's
Q and [[A, -A Q A], [0, A]], in mp.  selfcheck() holds the closed forms of jexp6 and of the Jacobian of log6 to the power series
sum (-ad)^n / (n+1)! and its inverse, which share nothing with them.

Where the relative quaternion's w is 0 -- to within 2^-50, the rounding its four products of float64 inputs already carry -- the rotation
is by pi and the sign of the axis is free: alt holds the other one, and a routine may return either.

Rows are edges, not a cloud: see ANGLES and CUTS."""
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import lie_ref  # noqa: E402

DPS = 60
PI = float(np.pi)
# rotation angles; PI - 0 is the double below pi
ANGLES = [0.0, 1e-300, 1e-12, 1e-9, 1e-8, 1e-6, 1e-4, 1e-3, 1.5e-3, 3e-3, 1e-2, 1.01e-2, 3e-2, 0.1, 0.5, 1.0, 2.0, 3.0] + \
         [PI - d for d in (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 3e-6, 1e-6, 1e-7, 1e-9, 0.0)]
# the angles at which a routine changes formula (rbd_device.h): t2 = 1e-6 (abc, log3, state_integrate_q; th * th = 1e-6 in state_diff_q),
# t2 = 1e-4 (jlog3, beta_of), t2 = 1e-8 (state_integrate), n2 = sin^2(t/2) = 1e-16 (state_diff_q), t2 = 0.25 (q_left), cos t = -0.5 (log3);
# each with the double either side
CUTS = [float(np.sqrt(1e-6)), float(np.sqrt(1e-4)), float(np.sqrt(1e-8)), 2e-8, 0.5, 2.0 * PI / 3.0]
MAGNITUDES = [1e-3, 0.3, 3.0]          # translations and rho
NORMS = [1.0, 0.99, 2.0]               # quaternions as given: unit, as linear interpolation leaves them, and far off
SINCOS_C1, SINCOS_C2 = 1.57079632673412561417e+00, 6.07710050650619224932e-11      # the literals of sincos_fast
ALIGNED = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1)]
QUAT_ALIGNED = [(0, 0, 0, 1), (1, 0, 0, 0), (0, 0, 0, -1), (0, 1, 0, 0), (0, 0, 1, 0)]


# ------------------------------------------------------------------------------------------------ mp: the definitions ---
def _sk(v):
    return [[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]


def _mm(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def _mv(A, x):
    return [sum(A[i][k] * x[k] for k in range(len(x))) for i in range(len(A))]


def _T(A):
    return [list(r) for r in zip(*A)]


def _lin(*terms):
    """sum of c * M over (c, M)"""
    n, m = len(terms[0][1]), len(terms[0][1][0])
    return [[sum(c * M[i][j] for c, M in terms) for j in range(m)] for i in range(n)]


def _eye(n=3):
    return [[mp.mpf(i == j) for j in range(n)] for i in range(n)]


def _flat(A):
    return [x for r in A for x in r]


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _coef(t2, closed, limit):
    """closed(t) with the digits its cancellations need; limit at t = 0"""
    if t2 == 0:
        return [mp.mpf(x) for x in limit]
    lost = max(0, -int(mp.floor(mp.log10(t2) / 2)))
    with mp.workdps(DPS + 8 * lost + 10):
        return closed(mp.sqrt(t2))


def _abc(t2):
    return _coef(t2, lambda t: [mp.sin(t) / t, (1 - mp.cos(t)) / t ** 2, (t - mp.sin(t)) / t ** 3], [1, mp.mpf(1) / 2, mp.mpf(1) / 6])


def _alpha_diag(t2):
    return _coef(t2, lambda t: [1 / t ** 2 - mp.sin(t) / (2 * t * (1 - mp.cos(t))), t * mp.sin(t) / (2 * (1 - mp.cos(t)))], [mp.mpf(1) / 12, 1])


def _c123(t2):
    return _coef(t2, lambda t: [(t - mp.sin(t)) / t ** 3, (t ** 2 + 2 * mp.cos(t) - 2) / (2 * t ** 4), (2 * t - 3 * mp.sin(t) + t * mp.cos(t)) / (2 * t ** 5)],
                 [mp.mpf(1) / 6, mp.mpf(1) / 24, mp.mpf(1) / 120])


def _exp6(v, w):
    a, b, c = _abc(_dot(w, w))
    K = _sk(w)
    K2 = _mm(K, K)
    return _lin((1, _eye()), (a, K), (b, K2)), _mv(_lin((1, _eye()), (b, K), (c, K2)), v)


def _jexp3(w):
    _, b, c = _abc(_dot(w, w))
    K = _sk(w)
    return _lin((1, _eye()), (-b, K), (c, _mm(K, K)))


def _jlog3(w):
    alpha, diag = _alpha_diag(_dot(w, w))
    return _lin((alpha, [[x * y for y in w] for x in w]), (diag, _eye()), (mp.mpf(1) / 2, _sk(w)))


def _q_left(rho, phi):
    c1, c2, c3 = _c123(_dot(phi, phi))
    P, R = _sk(phi), _sk(rho)
    PR, RP = _mm(P, R), _mm(R, P)
    PRP = _mm(PR, P)
    return _lin((mp.mpf(1) / 2, R), (c1, PR), (c1, RP), (c1, PRP), (c2, _mm(P, PR)), (c2, _mm(RP, P)), (-3 * c2, PRP), (c3, _mm(PRP, P)), (c3, _mm(P, PRP)))


def _blocks(A, B):
    """[[A, B], [0, A]]"""
    Z = [[mp.mpf(0)] * 3 for _ in range(3)]
    return [A[i] + B[i] for i in range(3)] + [Z[i] + A[i] for i in range(3)]


def _jexp6(nu):
    return _blocks(_jexp3(nu[3:]), _q_left([-x for x in nu[:3]], [-x for x in nu[3:]]))


def _jlog6(nu):
    A = _jlog3(nu[3:])
    AQA = _mm(_mm(A, _q_left([-x for x in nu[:3]], [-x for x in nu[3:]])), A)
    return _blocks(A, [[-x for x in r] for r in AQA])


def _unit_quat(q):
    n = mp.sqrt(_dot(q, q))
    return [x / n for x in q]


def _qmul(a, b):      # xyzw
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
            a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def _quat_R(q):      # of a unit quaternion
    x, y, z, w = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def _quat_log(r):
    """(log of the unit quaternion r as a rotation vector, whether the axis sign is free)"""
    if r[3] < 0:
        r = [-x for x in r]
    n = mp.sqrt(_dot(r[:3], r[:3]))
    if n == 0:
        return [mp.mpf(0)] * 3, False
    th = 2 * mp.atan2(n, r[3])
    return [th * x / n for x in r[:3]], r[3] <= mp.mpf(2) ** -50


def _log6_with(w, pr):
    alpha, _ = _alpha_diag(_dot(w, w))
    K = _sk(w)
    return _mv(_lin((1, _eye()), (-mp.mpf(1) / 2, K), (alpha, _mm(K, K))), pr) + list(w)


# f(op)(x) -> (outputs, the outputs with the other axis sign or None); x: the row's inputs as mp numbers
def _f_exp6(x):
    R, p = _exp6(x[:3], x[3:])
    return _flat(R) + p, None


def _f_log3_q(x):
    w, free = _quat_log(_unit_quat(x))
    return w, [-c for c in w] if free else None


def _f_diff(x):
    p0, q0, p1, q1 = x[0:3], _unit_quat(x[3:7]), x[7:10], _unit_quat(x[10:14])
    w, free = _quat_log(_qmul([-q0[0], -q0[1], -q0[2], q0[3]], q1))
    pr = _mv(_T(_quat_R(q0)), [p1[i] - p0[i] for i in range(3)])
    out = []
    for ww in (w, [-c for c in w]) if free else (w,):
        nu = _log6_with(ww, pr)
        out.append(nu + _flat(_jlog6(nu)))
    return out[0], out[1] if free else None


def _f_integrate(x):
    p, q, v, w = x[0:3], _unit_quat(x[3:7]), x[7:10], x[10:13]
    _, dp = _exp6(v, w)
    t = mp.sqrt(_dot(w, w))
    s = mp.sin(t / 2) / t if t != 0 else mp.mpf(1) / 2
    r = _unit_quat(_qmul(q, [s * w[0], s * w[1], s * w[2], mp.cos(t / 2)]))
    return [a + b for a, b in zip(p, _mv(_quat_R(q), dp))] + r, None


F = {
    "sincos": lambda x: ([mp.sin(x[0]), mp.cos(x[0])], None),
    "rcp_rsqrt": lambda x: ([1 / x[0], 1 / mp.sqrt(x[0])], None),
    "atan2_pos": lambda x: ([mp.atan2(x[0], x[1])], None),
    "exp6": _f_exp6,
    "jexp3": lambda x: (_flat(_jexp3(x)), None),
    "jlog3": lambda x: (_flat(_jlog3(x)), None),
    "q_left": lambda x: (_flat(_q_left(x[:3], x[3:])), None),
    "jexp6": lambda x: (_flat(_jexp6(x)), None),
    "log3_q": _f_log3_q,
    "diff": _f_diff,
    "integrate": _f_integrate,
}
ELEMENTARY = ("sincos", "rcp_rsqrt", "atan2_pos")


def reference(op, row):
    """(ref, alt, unit) of one row of float64 inputs, as float64 arrays"""
    with mp.workdps(DPS):
        x = [mp.mpf(float(v)) for v in row]
        ref, alt = F[op](x)
        out = np.array([float(v) for v in ref])
        out_alt = out if alt is None else np.array([float(v) for v in alt])
        if op in ELEMENTARY:
            unit = np.spacing(np.abs(out))
            if op == "sincos":
                k = mp.nint(2 * x[0] / mp.pi)
                unit = unit + float(abs(k) * abs(mp.pi / 2 - (mp.mpf(SINCOS_C1) + mp.mpf(SINCOS_C2))))
            return out, out_alt, unit
        moved = [mp.mpf(0)] * len(ref)
        for i in range(len(x)):
            xp = list(x)
            xp[i] = x[i] + mp.mpf(float(np.spacing(abs(float(row[i])))))
            # where the sign is free the last bit of an input may tip w across 0 and with it the branch: the move is to the nearer sign
            steps = [[abs(a - b) for a, b in zip(rp, ref)] for rp in F[op](xp) if rp is not None]
            moved = [m + s for m, s in zip(moved, min(steps, key=max))]
        unit = mp.mpf(2) ** -52 * max(abs(v) for v in ref) + max(moved)
        return out, out_alt, np.array([float(unit)])


def selfcheck():
    """the closed forms of jexp6 and of the Jacobian of log6 against sum_n (-ad)^n / (n+1)! and its inverse"""
    rng = np.random.default_rng(11)
    with mp.workdps(DPS):
        for t in (1e-9, 1e-3, 0.3, 3.0, PI):
            nu = [mp.mpf(float(c)) for c in np.concatenate([rng.standard_normal(3), t * _axis(rng)])]
            Kw, Kv = _sk(nu[3:]), _sk(nu[:3])
            ad = [Kw[i] + Kv[i] for i in range(3)] + [[mp.mpf(0)] * 3 + Kw[i] for i in range(3)]
            J, term = _eye(6), _eye(6)
            for n in range(1, 200):
                term = [[-c / (n + 1) for c in r] for r in _mm(term, ad)]
                J = _lin((1, J), (1, term))
                if max(abs(c) for c in _flat(term)) < mp.mpf(10) ** -(DPS - 5):
                    break
            assert max(abs(a - b) for a, b in zip(_flat(J), _flat(_jexp6(nu)))) < mp.mpf(10) ** -(DPS - 12), t
            assert max(abs(a - b) for a, b in zip(_flat(_mm(_jlog6(nu), J)), _flat(_eye(6)))) < mp.mpf(10) ** -(DPS - 12), t


# ---------------------------------------------------------------------------------------------------------- the rows ---
def _axis(rng):
    a = rng.standard_normal(3)
    return a / np.linalg.norm(a)


def rotations():
    """[(angle, unit axis, axis-aligned?)]: every angle of ANGLES about an aligned axis and a random one; every cut and the doubles
    either side of it about an aligned axis and a random one"""
    rng = np.random.default_rng(2026)
    rows, k = [], 0
    for t in ANGLES:
        rows.append((t, np.array(ALIGNED[k % 6], float), True))
        rows.append((t, _axis(rng), False))
        k += 1
    for c in CUTS:
        for t in (np.nextafter(c, 0.0), c, np.nextafter(c, 4.0)):
            rows.append((float(t), np.array(ALIGNED[k % 6], float), True))
            rows.append((float(t), _axis(rng), False))
            k += 1
    return rows


def _quat_of(t, a):
    return np.concatenate([np.sin(0.5 * t) * a, [np.cos(0.5 * t)]])


def _qmul_np(a, b):
    return np.array(_qmul(list(a), list(b)), float)


def inputs():
    """{op: [n][in] float64}"""
    rng = np.random.default_rng(355)
    rot = rotations()
    w = np.array([t * a for t, a, _ in rot])
    lin = np.array([MAGNITUDES[i % 3] * _axis(rng) for i in range(len(rot))])
    out = {"exp6": np.hstack([lin, w]), "jexp3": w, "jlog3": w, "q_left": np.hstack([lin, w]), "jexp6": np.hstack([lin, w])}

    # quaternions: of every rotation at the three norms in turn; both signs; rotations by exactly pi (w = 0)
    quats = [NORMS[i % 3] * _quat_of(t, a) for i, (t, a, _) in enumerate(rot)]
    quats += [-NORMS[i % 3] * _quat_of(t, _axis(rng)) for i, t in enumerate((1e-9, 1e-3, 1.0, 3.0, PI - 1e-7))]
    pis = [np.array(a + (0.0,)) for a in ALIGNED[:4]] + [np.concatenate([_axis(rng), [0.0]]) for _ in range(4)]
    quats += [NORMS[i % 3] * q for i, q in enumerate(pis)]
    out["log3_q"] = np.array(quats)

    # two placements: q1 = q0 (x) the rotation (q0 aligned where the rotation is, so that tiny angles survive the product), then q1 = -q0,
    # the relative w just either side of 0, and rotations by exactly pi
    def q0_of(i, aligned):
        return np.array(QUAT_ALIGNED[i % 5], float) if aligned else _unit(rng.standard_normal(4))

    def _unit(q):
        return q / np.linalg.norm(q)

    pairs = []
    for i, (t, a, aligned) in enumerate(rot):
        q0 = q0_of(i, aligned)
        pairs.append((NORMS[i % 3] * q0, NORMS[(i // 3) % 3] * _qmul_np(q0, _quat_of(t, a))))
    for i in range(4):
        q0 = q0_of(i, i < 2)
        pairs.append((NORMS[i % 3] * q0, -NORMS[i % 3] * q0))
    for i, e in enumerate((1e-9, -1e-9, 1e-12, -1e-12, 1e-9, -1e-9, 1e-12, -1e-12)):
        q0 = q0_of(i, i < 4)
        pairs.append((q0, NORMS[i % 3] * _qmul_np(q0, np.concatenate([np.sqrt(1.0 - e * e) * (np.array(ALIGNED[i], float) if i < 4 else _axis(rng)), [e]]))))
    pairs += [(NORMS[i % 3] * np.array([0.0, 0.0, 0.0, 1.0]), NORMS[(i + 1) % 3] * q) for i, q in enumerate(pis[:6])]
    p0 = rng.standard_normal((len(pairs), 3))
    p1 = p0 + np.array([MAGNITUDES[i % 3] * _axis(rng) for i in range(len(pairs))])
    out["diff"] = np.hstack([p0, np.array([a for a, _ in pairs]), p1, np.array([b for _, b in pairs])])

    q = np.array([NORMS[i % 3] * q0_of(i, aligned) for i, (_, _, aligned) in enumerate(rot)])
    out["integrate"] = np.hstack([rng.standard_normal((len(rot), 3)), q, lin, w])

    # sincos: zeros and tiny arguments, the doubles nearest k pi/2 and their neighbours, log-uniform magnitudes 1e-8 .. 1e5 of both signs
    x = [0.0, -0.0, 1e-300, -1e-300, 1e-20, -1e-20]
    with mp.workdps(DPS):
        for k in list(range(1, 9)) + [1000, 63661]:
            for s in (1, -1):
                c = float(s * k * mp.pi / 2)
                x += [float(np.nextafter(c, -np.inf)), c, float(np.nextafter(c, np.inf))]
    x += list(10.0 ** rng.uniform(-8, 5, 120) * np.where(rng.random(120) < 0.5, -1.0, 1.0))
    out["sincos"] = np.array(x)[:, None]

    a = [2.0 ** k for k in range(-500, 501, 50)] + [0.5, 2.0, 4.0, 1.0, float(np.nextafter(1.0, 0.0)), float(np.nextafter(1.0, 2.0))]
    a += list(2.0 ** rng.uniform(-500, 500, 80))
    out["rcp_rsqrt"] = np.array(a)[:, None]

    # atan2_pos (y, x >= 0, not both 0): the axes, the diagonal, t = y / x either side of tan(pi/8), (n, w) on the unit circle, small ratios
    t8 = float(np.sqrt(2.0) - 1.0)
    yx = [(0.0, 1.0), (0.0, 1e-30), (1.0, 0.0), (1e30, 0.0), (1.0, 1.0), (1e-8, 1e-8), (3.7, 3.7)]
    for t in (float(np.nextafter(t8, 0.0)), t8, float(np.nextafter(t8, 1.0))):
        yx += [(t, 1.0), (1.0, t), (3.0 * t, 3.0)]
    for n in 10.0 ** np.linspace(-8, 0, 41):
        yx.append((float(n), float(np.sqrt(max(0.0, 1.0 - n * n)))))
    for k in range(1, 31):
        s = float(rng.uniform(0.5, 2.0))
        yx += [(s * 10.0 ** -k, s), (s, s * 10.0 ** -k)]
    yx += [tuple(r) for r in rng.uniform(0.0, 1.0, (40, 2))]
    out["atan2_pos"] = np.array(yx)
    return out


def main():
    selfcheck()
    arrays = {}
    for op, rows in inputs().items():
        assert rows.shape[1] == lie_ref.OPS[op][1] and len(rows) <= 512, op
        ref, alt, unit = zip(*(reference(op, r) for r in rows))
        free = [i for i in range(len(rows)) if not np.array_equal(ref[i], alt[i])]
        arrays.update({op + "_in": rows, op + "_ref": np.array(ref), op + "_unit": np.array(unit), op + "_alt_rows": np.array(free, np.int32),
                       op + "_alt": np.array([alt[i] for i in free]).reshape(len(free), lie_ref.OPS[op][3])})
        assert arrays[op + "_ref"].shape == (len(rows), lie_ref.OPS[op][3]), op
        print("%-10s %3d rows, %d with a free axis sign" % (op, len(rows), len(free)))
    np.savez_compressed(lie_ref.FIXTURE, **arrays)
    print(lie_ref.FIXTURE, os.path.getsize(lie_ref.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
