"""fp64 truth of the Lie-group operators of csrc/lie_ops.hip / sk_gs_amd/lietorch.py (a plain helper module, numpy only).

What it states, independently of the code under test:

* the forward maps ``exp`` / ``log`` of SO3 (unit quaternion xyzw) and SE3 (embedding (t, q), tangent (tau, phi)), and the row-vector
  gradients documented at the top of lie_ops.hip: ``da = dX J_l(a)`` for exp, ``dX = da J_l^-1(log X)`` for log, with the SE3 blocks
  ``[[J, Q], [0, J]]`` and ``[[J^-1, -J^-1 Q J^-1], [0, J^-1]]``; gradients of group elements are left-tangent rows in the first K of
  their N slots, the rest zero;
* the other operators (inv, mul, adj, adjT, act, act4, vec / InitFromVec) through 3x3 rotation matrices.

The five scalar coefficients of J, J^-1 and Q

    A = (1 - cos t) / t^2      B = (t - sin t) / t^3      C = (t^2 + 2 cos t - 2) / (2 t^4)
    D = (2 t - 3 sin t + t cos t) / (2 t^5)               E = (1 - t cot(t / 2) / 2) / t^2

are evaluated by their Taylor series below ``CROSSOVER`` and by the closed form above it: the closed forms cancel (in fp64 they are off by
1e-9 relative at t = 1e-6, D by far more), so neither they nor the fp64 torch bodies can serve as the truth at small angles.  At the
crossover (t = 2) the closed forms lose at most two digits and the series (14 terms for A..D, 24 for E whose radius of convergence is
2 pi) are converged to the last bit; tests/test_lie_truth_cpu.py checks all five against mpmath to 1e-14 relative from 1e-12 to pi.

Branch convention of ``log``: the kernel's, ``phi = 2 atan(n / w) / n * v`` with n = |v| -- NOT atan2.  A quaternion with w < 0 gives the
rotation vector of angle 2 atan(n / w) in (-pi, 0) about v, i.e. q and -q give the same rotation vector; the value jumps from +pi to -pi
across w = 0, and w = 0 itself takes the kernel's side (-pi).  The input quaternion is normalised first, as the constructors do.
"""
from fractions import Fraction
from math import factorial

import numpy as np

CROSSOVER = 2.0


def _bernoulli(n_max):
    B = [Fraction(0)] * (n_max + 1)
    B[0] = Fraction(1)
    for m in range(1, n_max + 1):
        B[m] = -sum(Fraction(factorial(m + 1), factorial(k) * factorial(m + 1 - k)) * B[k] for k in range(m)) / (m + 1)
    return B


_NT = 14
_BERN = _bernoulli(48)
# coefficients of the series in t^2, lowest order first
SERIES = {
    'A': [float(Fraction((-1) ** k, factorial(2 * k + 2))) for k in range(_NT)],
    'B': [float(Fraction((-1) ** k, factorial(2 * k + 3))) for k in range(_NT)],
    'C': [float(Fraction((-1) ** k, factorial(2 * k + 4))) for k in range(_NT)],
    'D': [float(Fraction((-1) ** k * (k + 1), factorial(2 * k + 5))) for k in range(_NT)],
    'E': [float(abs(_BERN[2 * n]) / factorial(2 * n)) for n in range(1, 25)],   # (t/2) cot(t/2) = 1 - sum |B_2n| t^2n / (2n)!
}


def _closed(name, t):
    s, c = np.sin(t), np.cos(t)
    if name == 'A':
        return (1.0 - c) / t ** 2
    if name == 'B':
        return (t - s) / t ** 3
    if name == 'C':
        return (t * t + 2.0 * c - 2.0) / (2.0 * t ** 4)
    if name == 'D':
        return (2.0 * t - 3.0 * s + t * c) / (2.0 * t ** 5)
    return (1.0 - 0.5 * t * np.cos(0.5 * t) / np.sin(0.5 * t)) / t ** 2


def coefficient(name, theta):
    """one of the five coefficients at the angles ``theta`` (any shape, fp64)"""
    theta = np.asarray(theta, np.float64)
    t2 = theta * theta
    ser = np.zeros_like(theta)
    for c in reversed(SERIES[name]):
        ser = ser * t2 + c
    small = theta < CROSSOVER
    return np.where(small, ser, _closed(name, np.where(small, CROSSOVER, theta)))


# ------------------------------------------------------------------------------------------------ small batched helpers
def hat(v):
    v = np.asarray(v, np.float64)
    z = np.zeros_like(v[..., 0])
    return np.stack([z, -v[..., 2], v[..., 1], v[..., 2], z, -v[..., 0], -v[..., 1], v[..., 0], z], -1).reshape(*v.shape[:-1], 3, 3)


def _row(g, M):
    return np.einsum('...i,...ij->...j', g, M)


def _col(M, a):
    return np.einsum('...ij,...j->...i', M, a)


def _pad(g, n):
    return np.concatenate([g, np.zeros(g.shape[:-1] + (n - g.shape[-1],))], -1)


def qnormalize(q):
    q = np.asarray(q, np.float64)
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def qmul(a, b):
    av, aw, bv, bw = a[..., :3], a[..., 3:], b[..., :3], b[..., 3:]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), aw * bw - (av * bv).sum(-1, keepdims=True)], -1)


def qconj(q):
    return np.concatenate([-q[..., :3], q[..., 3:]], -1)


def qmat(q):
    """rotation matrix of a unit quaternion xyzw:  R = I + 2 w hat(v) + 2 hat(v)^2"""
    V = hat(q[..., :3])
    return np.eye(3) + 2.0 * q[..., 3, None, None] * V + 2.0 * V @ V


# ------------------------------------------------------------------------------------------------ exp / log and their Jacobians
def _theta(phi):
    return np.sqrt((phi * phi).sum(-1))


def so3_exp(phi):
    phi = np.asarray(phi, np.float64)
    th = _theta(phi)
    t2 = th * th
    small = th < 1e-2                                                     # sin(t/2)/t: series (next term 4e-28) below, closed form above
    imag = np.where(small, 0.5 - t2 / 48.0 + t2 * t2 / 3840.0 - t2 ** 3 / 645120.0, np.sin(0.5 * th) / np.where(small, 1.0, th))
    return np.concatenate([imag[..., None] * phi, np.cos(0.5 * th)[..., None]], -1)


def so3_log(q):
    q = qnormalize(q)
    v, w = q[..., :3], q[..., 3]
    n = np.sqrt((v * v).sum(-1))
    r = n / np.where(w == 0, 1.0, w)
    small = np.abs(r) < 1e-3                                               # 2 atan(n/w)/n = (2/w) (1 - r^2/3 + r^4/5 - r^6/7 ...)
    ser = 2.0 / np.where(w == 0, 1.0, w) * (1.0 - r ** 2 / 3.0 + r ** 4 / 5.0 - r ** 6 / 7.0)
    gen = 2.0 * np.arctan(r) / np.where(n == 0, 1.0, n)
    f = np.where(w == 0, -np.pi / np.where(n == 0, 1.0, n), np.where(small, ser, gen))
    return f[..., None] * v


def so3_left_jacobian(phi):
    phi = np.asarray(phi, np.float64)
    th, P = _theta(phi)[..., None, None], hat(phi)
    return np.eye(3) + coefficient('A', th) * P + coefficient('B', th) * (P @ P)


def so3_left_jacobian_inverse(phi):
    phi = np.asarray(phi, np.float64)
    th, P = _theta(phi)[..., None, None], hat(phi)
    return np.eye(3) - 0.5 * P + coefficient('E', th) * (P @ P)


def se3_Q(tau, phi):
    tau, phi = np.asarray(tau, np.float64), np.asarray(phi, np.float64)
    th, T, P = _theta(phi)[..., None, None], hat(tau), hat(phi)
    PT, TP = P @ T, T @ P
    PTP = PT @ P
    return (0.5 * T + coefficient('B', th) * (PT + TP + PTP) + coefficient('C', th) * (P @ PT + TP @ P - 3.0 * PTP)
            + coefficient('D', th) * (PTP @ P + P @ PTP))


def se3_exp(a):
    a = np.asarray(a, np.float64)
    return np.concatenate([_col(so3_left_jacobian(a[..., 3:]), a[..., :3]), so3_exp(a[..., 3:])], -1)


def se3_log(X):
    X = np.asarray(X, np.float64)
    phi = so3_log(X[..., 3:7])
    return np.concatenate([_col(so3_left_jacobian_inverse(phi), X[..., :3]), phi], -1)


def _blocks(a, b, c, d):
    return np.concatenate([np.concatenate([a, b], -1), np.concatenate([c, d], -1)], -2)


def se3_left_jacobian(a):
    a = np.asarray(a, np.float64)
    J = so3_left_jacobian(a[..., 3:])
    return _blocks(J, se3_Q(a[..., :3], a[..., 3:]), np.zeros_like(J), J)


def se3_left_jacobian_inverse(a):
    a = np.asarray(a, np.float64)
    Ji = so3_left_jacobian_inverse(a[..., 3:])
    return _blocks(Ji, -Ji @ se3_Q(a[..., :3], a[..., 3:]) @ Ji, np.zeros_like(Ji), Ji)


# ------------------------------------------------------------------------------------------------ the two groups
class SO3:
    name, K, N = 'SO3', 3, 4
    exp, log = staticmethod(so3_exp), staticmethod(so3_log)
    left_jacobian, left_jacobian_inverse = staticmethod(so3_left_jacobian), staticmethod(so3_left_jacobian_inverse)

    @staticmethod
    def canon(X):
        return qnormalize(X)

    @staticmethod
    def inv(X):
        return qconj(qnormalize(X))

    @staticmethod
    def mul(X, Y):
        return qmul(qnormalize(X), qnormalize(Y))

    @staticmethod
    def Adj(X):
        return qmat(qnormalize(X))

    @staticmethod
    def adj(a):
        return hat(a)

    @staticmethod
    def matrix4(X):
        M = np.zeros(X.shape[:-1] + (4, 4))
        M[..., :3, :3] = qmat(qnormalize(X))
        M[..., 3, 3] = 1.0
        return M

    @staticmethod
    def act_jacobian(y, y3=None):
        return hat(-y)

    @staticmethod
    def projector(X):
        """the N x K block of lietorch's orthogonal_projector: rows 0..2 = (w I - hat(v)) / 2, row 3 = -v / 2"""
        q = qnormalize(X)
        return np.concatenate([0.5 * (q[..., 3, None, None] * np.eye(3) - hat(q[..., :3])), -0.5 * q[..., None, :3]], -2)

    @staticmethod
    def projector_pinv(X):
        """K x N: J_q^T J_q = I / 4 for a unit quaternion, so pinv(J_q) = 4 J_q^T (the Moore-Penrose conditions: test_lie_truth_cpu.py)"""
        return 4.0 * np.swapaxes(SO3.projector(X), -1, -2)


class SE3:
    name, K, N = 'SE3', 6, 7
    exp, log = staticmethod(se3_exp), staticmethod(se3_log)
    left_jacobian, left_jacobian_inverse = staticmethod(se3_left_jacobian), staticmethod(se3_left_jacobian_inverse)

    @staticmethod
    def canon(X):
        X = np.asarray(X, np.float64)
        return np.concatenate([X[..., :3], qnormalize(X[..., 3:7])], -1)

    @staticmethod
    def inv(X):
        X = SE3.canon(X)
        qi = qconj(X[..., 3:])
        return np.concatenate([-_col(qmat(qi), X[..., :3]), qi], -1)

    @staticmethod
    def mul(X, Y):
        X, Y = SE3.canon(X), SE3.canon(Y)
        return np.concatenate([X[..., :3] + _col(qmat(X[..., 3:]), Y[..., :3]), qmul(X[..., 3:], Y[..., 3:])], -1)

    @staticmethod
    def Adj(X):
        X = SE3.canon(X)
        R = qmat(X[..., 3:])
        return _blocks(R, hat(X[..., :3]) @ R, np.zeros_like(R), R)

    @staticmethod
    def adj(a):
        T, P = hat(a[..., :3]), hat(a[..., 3:])
        return _blocks(P, T, np.zeros_like(P), P)

    @staticmethod
    def matrix4(X):
        X = SE3.canon(X)
        M = np.zeros(X.shape[:-1] + (4, 4))
        M[..., :3, :3] = qmat(X[..., 3:])
        M[..., :3, 3] = X[..., :3]
        M[..., 3, 3] = 1.0
        return M

    @staticmethod
    def act_jacobian(y, y3=None):
        I = np.broadcast_to(np.eye(3), y.shape[:-1] + (3, 3)) * (1.0 if y3 is None else y3[..., None, None])
        return np.concatenate([I, hat(-y)], -1)

    @staticmethod
    def projector(X):
        """[[I, hat(-t)], [0, J_q]]  (N x K)"""
        X = SE3.canon(X)
        Jq = SO3.projector(X[..., 3:])
        top = np.concatenate([np.broadcast_to(np.eye(3), Jq.shape[:-2] + (3, 3)), hat(-X[..., :3])], -1)
        return np.concatenate([top, np.concatenate([np.zeros_like(Jq), Jq], -1)], -2)

    @staticmethod
    def projector_pinv(X):
        """[[I, -4 hat(-t) J_q^T], [0, 4 J_q^T]]  (K x N).  numpy's SVD-based pinv loses |t|^2 eps on this matrix (1e-10 at |t| = 100),
        hence the block form; test_lie_truth_cpu.py checks the four Moore-Penrose conditions on it"""
        X = SE3.canon(X)
        Pq = SO3.projector_pinv(X[..., 3:])
        top = np.concatenate([np.broadcast_to(np.eye(3), Pq.shape[:-2] + (3, 3)), -hat(-X[..., :3]) @ Pq], -1)
        return np.concatenate([top, np.concatenate([np.zeros(Pq.shape[:-2] + (3, 3)), Pq], -1)], -2)


GROUPS = {'SO3': SO3, 'SE3': SE3}


def operator(G, name, x, y=None, cot=None):
    """(value, dX, dY) of operator ``name`` of group ``G`` at the rows x (and y) for the cotangent rows ``cot``; gradients of group
    arguments are tangent rows padded to N.  ``act4`` multiplies the translation by the point's fourth coordinate; ``vec`` is the identity
    forward with ``cot J`` backward; ``InitFromVec`` the identity forward with ``cot[:K] pinv(J)`` backward (N wide, not a tangent row)."""
    x = np.asarray(x, np.float64)
    y = None if y is None else np.asarray(y, np.float64)
    K, N = G.K, G.N
    if name == 'exp':
        return G.exp(x), _row(cot[..., :K], G.left_jacobian(x)), None
    if name == 'log':
        a = G.log(x)
        return a, _pad(_row(cot, G.left_jacobian_inverse(a)), N), None
    if name == 'inv':
        Xi = G.inv(x)
        return Xi, _pad(-_row(cot[..., :K], G.Adj(Xi)), N), None
    if name == 'mul':
        return G.mul(x, y), _pad(cot[..., :K], N), _pad(_row(cot[..., :K], G.Adj(x)), N)
    if name == 'adj':
        A = G.Adj(x)
        b = _col(A, y)
        return b, _pad(-_row(cot, G.adj(b)), N), _row(cot, A)
    if name == 'adjT':
        A = G.Adj(x)
        Adb = _col(A, cot)
        return _row(y, A), _pad(-_row(y, G.adj(Adb)), N), Adb
    if name == 'act':
        M = G.matrix4(x)
        out = _col(M[..., :3, :3], y) + M[..., :3, 3]
        return out, _pad(_row(cot, G.act_jacobian(out)), N), _row(cot, M[..., :3, :3])
    if name == 'InitFromVec':
        return x, _row(cot[..., :K], G.projector_pinv(x)), None
    if name == 'act4':
        M = G.matrix4(x)
        out = _col(M, y)
        return out, _pad(_row(cot[..., :3], G.act_jacobian(out[..., :3], out[..., 3])), N), _row(cot, M)
    if name == 'vec':
        return x, _pad(_row(cot, G.projector(x)), N), None
    raise KeyError(name)


def row_error(got, want, cot=None):
    """per-row error: max |got - want| over the row, divided by max(|want row|_inf, 1) for values (``cot`` None) and by
    max(|want row|_inf, |cotangent row|_inf) for gradients"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max(-1)
    scale = np.maximum(scale, 1.0) if cot is None else np.maximum(scale, np.abs(np.asarray(cot, np.float64)).max(-1))
    return np.abs(got - want).max(-1) / np.maximum(scale, 1e-300)


def align_quaternion_sign(got, want):
    """q and -q are the same rotation: flips whole quaternions (the last four columns) of ``got`` onto ``want``'s side"""
    got = np.array(got, np.float64)
    s = np.where((got[..., -4:] * want[..., -4:]).sum(-1, keepdims=True) < 0, -1.0, 1.0)
    got[..., -4:] *= s
    return got
