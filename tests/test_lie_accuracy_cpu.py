"""The pure-torch bodies of sk_gs_amd/lietorch.py (the CPU path; csrc/lie_ops.hip repeats them term for term) against the fp64 truth of
tests/lie_truth.py, per row, in every angle band from 1e-9 to pi (tests/lie_cases.py has the rows, the metric and the bounds).

fp32: the bounds of the GPU test, 3e-6 on values and 2e-5 on gradients.  fp64: the same bounds scaled by the ratio of the unit
roundoffs, 2^-53 / 2^-24 -- the formulas are the same, so their error is the same number of ulps -- plus 1e-14 for the first term the
series leave out (largest for J^-1's coefficient at the crossover: |B_18| / 18! = 8.6e-15), which does not shrink with the precision.
The other such term are the rows around w = 0 of log: below |w| = 1e-6 so3_log returns +-pi / n for 2 atan(n / w) / n, an approximation
that is off by 2 |w| / n <= 2e-6 absolute (6e-7 of pi) in any precision; those rows keep the fp32 bounds in fp64 too.

This is where the crossover of the series and their length are justified.  With lietorch's closed forms above theta^2 = 0.1 (five
terms below) every band met the bounds at |tau| = 1, but at |tau| = 1e2 the band 0.1 .. 1 did not: the closed forms of the t^-4 and
t^-5 coefficients of Q are still 2e-6 off at theta = 0.5, 5e-5 of a gradient row whose cotangent is nearly parallel to tau (worst
rows of 4 x 3000 per band, log backward: 1.4e-5, one draw at 2.5e-5).  With the crossover at theta^2 = 1 the same rows give 4.5e-6, the
level of every other band (the cross product ga x tau in fp32), and theta^2 = 4 gains nothing more.  Eight terms: the first one left
out is < 1e-14 of the leading one at the crossover, so the fp64 path is exact to its own precision as well.
"""
import numpy as np
import pytest
import torch

import lie_cases as C
import lie_truth as T

FP64_SCALE = 2.0 ** -29
SERIES_REST = 1e-14


def _lietorch():
    from sk_gs_amd import lietorch as L
    return L


@pytest.mark.parametrize('dtype', ['fp32', 'fp64'])
@pytest.mark.parametrize('op', C.OPERATORS_ALL_BANDS + C.OPERATORS_NEAR_IDENTITY)
@pytest.mark.parametrize('group', ['SO3', 'SE3'])
def test_torch_bodies_against_the_truth(group, op, dtype):
    L = _lietorch()
    x, y, cot, labels, scales = C.make_case(T.GROUPS[group], op, L.SERIES_THETA2, n_per=400 if op in C.OPERATORS_ALL_BANDS else 200)
    got = C.run_standin(L, group, op, x, y, cot, 'cpu', torch.float32 if dtype == 'fp32' else torch.float64)
    err = C.errors(group, op, x, y, cot, got)
    if dtype == 'fp64':
        for k, e in err.items():                                            # in units of the fp32 bounds (module docstring)
            err[k] = e / np.where(labels == C.AT_PI, 1.0, FP64_SCALE + SERIES_REST / (C.VALUE_BOUND if k == 'value' else C.GRAD_BOUND))
    rows, text = C.table(group, op, err, labels, scales)
    print(text)
    assert not C.failures(rows), (group, op, dtype, C.failures(rows))


def test_series_meet_the_closed_forms_at_the_crossover():
    """both sides of SERIES_THETA2, in fp32: the series' truncation and the closed forms' cancellation are each far inside the bound"""
    L = _lietorch()
    d = torch.tensor([0.36, -0.48, 0.8])
    tau = torch.tensor([0.6, 0.0, -0.8])
    for th, series in ((L.SERIES_THETA2 ** 0.5 * (1 - 1e-5), True), (L.SERIES_THETA2 ** 0.5 * (1 + 1e-5), False)):
        phi = d * th
        assert bool(phi.square().sum() < L.SERIES_THETA2) == series
        p64 = phi.double().numpy()
        for got, want in ((L._so3_left_jacobian(phi), T.so3_left_jacobian(p64)), (L._so3_left_jacobian_inverse(phi), T.so3_left_jacobian_inverse(p64)),
                          (L._se3_calcQ(tau, phi), T.se3_Q(tau.double().numpy(), p64))):
            assert np.abs(got.double().numpy() - want).max() <= 1e-6


def test_kernel_and_torch_bodies_carry_the_same_series():
    """csrc/lie_ops.hip states its coefficients as literals; they are the numbers lietorch.py computes, to the last bit of fp32"""
    import os
    import re
    L = _lietorch()
    src = open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), 'csrc', 'lie_ops.hip')).read()
    assert float(re.search(r'SERIES_THETA2 = ([0-9.]+)f;', src).group(1)) == L.SERIES_THETA2
    assert int(re.search(r'SERIES_TERMS = (\d+);', src).group(1)) == L.SERIES_TERMS
    for name in 'ABCDE':
        body = re.search(r'SERIES_%s\[SERIES_TERMS\] = \{(.*?)\};' % name, src, re.S).group(1)
        lits = [np.float32(float(a) / float(b)) for a, b in re.findall(r'SKGS_F\((-?[0-9.]+), ([0-9.]+)\)', body)]
        assert lits == [np.float32(c) for c in getattr(L, '_SERIES_' + name)], name
