"""The fp64 truth of the Lie operators (tests/lie_truth.py) checked against things that do not share its formulas: mpmath at 120 digits
for the five coefficients, J J^-1 = I, and a central finite difference of exp through 4x4 matrices for the left-tangent convention."""
import mpmath
import numpy as np
import pytest

import lie_truth as T


def _mp_coefficient(name, t):
    s, c = mpmath.sin(t), mpmath.cos(t)
    return {'A': lambda: (1 - c) / t ** 2, 'B': lambda: (t - s) / t ** 3, 'C': lambda: (t * t + 2 * c - 2) / (2 * t ** 4),
            'D': lambda: (2 * t - 3 * s + t * c) / (2 * t ** 5), 'E': lambda: (1 - t * mpmath.cot(t / 2) / 2) / t ** 2}[name]()


@pytest.mark.parametrize('name', 'ABCDE')
def test_coefficients_against_mpmath(name):
    """1e-14 relative on a log grid from 1e-12 to pi, both sides of the crossover included.  The closed form in mpmath loses
    ~5 log10(1/theta) digits to cancellation (D at 1e-12: 60), hence 120 digits of working precision."""
    grid = np.concatenate([np.logspace(-12, np.log10(np.pi), 400), [np.nextafter(T.CROSSOVER, 0), T.CROSSOVER, np.nextafter(T.CROSSOVER, 4), np.pi]])
    got = T.coefficient(name, grid)
    with mpmath.workprec(400):
        want = [_mp_coefficient(name, mpmath.mpf(float(t))) for t in grid]
        rel = max(abs((mpmath.mpf(float(g)) - w) / w) for g, w in zip(got, want))
    assert rel <= 1e-14, (name, float(rel))


def _tangents(n, K, seed, theta_lo=-9.0, theta_hi=np.log10(np.pi - 1e-3)):
    g = np.random.default_rng(seed)
    a = g.standard_normal((n, K))
    d = g.standard_normal((n, 3))
    a[:, -3:] = d / np.linalg.norm(d, axis=-1, keepdims=True) * 10.0 ** g.uniform(theta_lo, theta_hi, (n, 1))
    return a


def test_jacobian_times_its_inverse_is_the_identity():
    a = _tangents(4000, 6, 0)
    a[:, :3] *= 10.0 ** np.random.default_rng(1).uniform(-3, 2, (4000, 1))
    e3 = np.abs(T.so3_left_jacobian(a[:, 3:]) @ T.so3_left_jacobian_inverse(a[:, 3:]) - np.eye(3)).max()
    assert e3 <= 1e-13, e3
    P = T.se3_left_jacobian(a) @ T.se3_left_jacobian_inverse(a) - np.eye(6)
    scale = np.maximum(1.0, np.linalg.norm(a[:, :3], axis=-1))[:, None, None]          # the Q block carries |tau|
    assert np.abs(P / scale).max() <= 1e-13, np.abs(P / scale).max()


def test_exp_and_log_are_inverse_maps():
    for G in (T.SO3, T.SE3):
        a = _tangents(4000, G.K, 2)
        back = G.log(G.exp(a))
        assert np.abs(back - a).max() <= 1e-13 * max(1.0, np.abs(a).max()), G.name
        X = G.exp(a)
        X[:, -4:] *= -1.3                                                   # -q, un-normalised: the same rotation vector (branch convention)
        assert np.abs(G.log(X) - a).max() <= 1e-13 * max(1.0, np.abs(a).max()), G.name
    q = np.array([[0.6, 0.0, 0.8, 0.0], [0.6, 0.0, 0.8, 1e-9], [0.6, 0.0, 0.8, -1e-9]])
    n = np.linalg.norm(T.so3_log(q), axis=-1)
    assert np.allclose(n, np.pi, atol=1e-8) and np.allclose(T.so3_log(q)[[0, 2]], -T.so3_log(q)[[1, 1]], atol=1e-8)   # w = 0 sides with w < 0


@pytest.mark.parametrize('group', ['SO3', 'SE3'])
def test_left_jacobian_against_a_finite_difference_of_exp(group):
    """M = exp(a + h e_i) exp(a - h e_i)^-1 = exp(D) as 4x4 matrices with D = 2 h hat(J_l e_i) + O(h^3), and (M - M^-1) / 2 = D + O(h^3):
    column i of J_l read off the matrices, with no use of log or of the Jacobian's formulas.  Moderate angles (0.1 .. 2.5): the truncation is h^2 |J'''| ~ 1e-10."""
    G = T.GROUPS[group]
    a = _tangents(200, G.K, 3, theta_lo=-1.0, theta_hi=np.log10(2.5))
    J = G.left_jacobian(a)
    h = 1e-5
    for i in range(G.K):
        e = np.zeros(G.K)
        e[i] = h
        M = G.matrix4(G.exp(a + e)) @ np.linalg.inv(G.matrix4(G.exp(a - e)))
        W = (M - np.linalg.inv(M)) / 2.0                                   # sinh of the generator: no second-order term
        rot = np.stack([W[:, 2, 1], W[:, 0, 2], W[:, 1, 0]], -1) / (2 * h)
        col = rot if group == 'SO3' else np.concatenate([W[:, :3, 3] / (2 * h), rot], -1)
        assert np.abs(col - J[:, :, i]).max() <= 2e-9, (group, i, np.abs(col - J[:, :, i]).max())


@pytest.mark.parametrize('group', ['SO3', 'SE3'])
def test_log_gradient_is_the_inverse_of_the_exp_gradient(group):
    G = T.GROUPS[group]
    a = _tangents(500, G.K, 4)
    cot = np.random.default_rng(5).standard_normal((500, G.K))
    _, dX, _ = T.operator(G, 'log', G.exp(a), cot=cot)
    assert np.abs(dX[:, G.K:]).max() == 0
    _, da, _ = T.operator(G, 'exp', a, cot=dX)
    assert np.abs(da - cot).max() <= 1e-12 * max(1.0, np.abs(a).max())


@pytest.mark.parametrize('group', ['SO3', 'SE3'])
def test_projector_pseudo_inverse_meets_the_moore_penrose_conditions(group):
    G = T.GROUPS[group]
    X = G.exp(_tangents(300, G.K, 6))
    X[:, -4:] *= 1.2
    if group == 'SE3':
        X[:, :3] *= 10.0 ** np.random.default_rng(7).uniform(-3, 2, (300, 1))
    J, P = G.projector(X), G.projector_pinv(X)
    sym = lambda M: np.abs(M - np.swapaxes(M, -1, -2)).max()  # noqa: E731
    s = max(1.0, np.abs(X[:, :-4]).max()) ** 2 if group == 'SE3' else 1.0
    assert np.abs(P @ J - np.eye(G.K)).max() <= 1e-13 * s and np.abs(J @ P @ J - J).max() <= 1e-13 * s
    assert sym(P @ J) <= 1e-13 * s and sym(J @ P) <= 1e-13 * s and np.abs(P @ J @ P - P).max() <= 1e-13 * s
