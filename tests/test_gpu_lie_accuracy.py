"""csrc/lie_ops.hip (skgs_lie_forward / skgs_lie_backward, reached through sk_gs_amd.lietorch on the device) against the fp64 truth of
tests/lie_truth.py, per row, in every angle regime: exp and log over all bands from 1e-9 to pi (exp to 6.0) plus the exact rows (0, 1e-6,
the series' crossover, the at-pi branches of log), the other operators near the identity (theta <= 1e-2; O(1) angles are
test_hip_group_operators_against_the_torch_bodies' part), SE3 at |tau| = 1e-3, 1 and 1e2, launches of 1, 63, 64, 65 and 1000 rows.
tests/lie_cases.py has the rows, the metric and the bounds (3e-6 values, 2e-5 gradients, per row, no row dropped).

Every case prints its table of worst per-row errors per band (`[lie-accuracy] ...`); LAB_NOTEBOOK.md keeps the tables measured with
lietorch's closed forms down to 1e-6 (where the bands from 1e-6 to 1 fail) and with the series below theta^2 = 1.
"""
import pytest
import torch

import lie_cases as C
import lie_truth as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('op', C.OPERATORS_ALL_BANDS + C.OPERATORS_NEAR_IDENTITY)
@pytest.mark.parametrize('group', ['SO3', 'SE3'])
def test_hip_group_operators_against_the_truth(group, op):
    from sk_gs_amd import lietorch as L
    n_per = {'SO3': 300, 'SE3': 100}[group] if op in C.OPERATORS_ALL_BANDS else {'SO3': 450, 'SE3': 150}[group]
    x, y, cot, labels, scales = C.make_case(T.GROUPS[group], op, L.SERIES_THETA2, n_per)
    before = dict(L.hip_op_calls)
    got = C.run_standin(L, group, op, x, y, cot, 'cuda', torch.float32)
    n = len(C.launches(len(x)))
    assert L.hip_op_calls['backward'] == before['backward'] + n                         # the HIP launches ran, one per direction
    assert L.hip_op_calls['forward'] == before['forward'] + (0 if op in ('vec', 'InitFromVec') else n)
    err = C.errors(group, op, x, y, cot, got)
    rows, text = C.table(group, op, err, labels, scales)
    print(text)
    assert not C.failures(rows), (group, op, C.failures(rows))
