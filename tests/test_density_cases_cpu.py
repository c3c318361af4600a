"""The cases of tests/density_cases.py are what they claim to be (no GPU): float32 and float64 agree on every flag -- the condition that
lets tests/test_gpu_density_control.py demand exact row lists with no row excluded -- the restated masks are the torch expressions of
sk_gs_amd/densify.py and the reference's prune lines, and the planted ties are there."""
import numpy as np
import pytest
import torch

import density_cases as dc

CASES = dc.case_list()


@pytest.mark.parametrize('case', CASES, ids=dc.case_id)
def test_float32_and_float64_take_the_same_side_everywhere(case):
    c = dc.make_case(*case)
    for with_radii in (True, False):
        m64, m32 = dc.masks_of(c, np.float64, with_radii), dc.masks_of(c, np.float32, with_radii)
        for name, a, b in zip(('clone', 'split', 'drop'), m64, m32):
            assert a.shape == (c['P'],) and np.array_equal(a, b), (name, with_radii, np.nonzero(a != b)[0][:8])
    clone, split, drop = dc.masks_of(c)
    # ... and they are what the generator meant every row to be
    assert np.array_equal(clone, c['sel'] & ~c['big']) and np.array_equal(split, c['sel'] & c['big'])
    assert np.array_equal(~drop, c['keep']) and np.array_equal(~dc.masks_of(c, with_radii=False)[2], c['keep_opacity_only'])
    assert not (clone & split).any()
    # the margin itself, in float64: whatever passes through exp or the sigmoid stays MARGIN away from its threshold
    s = np.exp(c['log_scale'].astype(np.float64)).max(1) if c['P'] else np.zeros(0)
    o = 1 / (1 + np.exp(-c['opacity'].astype(np.float64).reshape(-1)))
    for v, thr in ((s, dc.SCENE_EXTENT), (s, dc.WORLD_LIMIT), (o, dc.MIN_OPACITY)):
        assert (np.abs(v / np.float64(thr) - 1) >= 0.99 * dc.MARGIN).all()
    rows, counts = dc.expected_select(clone, split, c['N'])
    assert rows.size == counts[0] + counts[1] + c['N'] * counts[2] <= (2 + c['N']) * c['P'] and counts[0] + counts[2] == c['P']
    if c['pattern'] == 'all_split' and c['P']:
        assert counts[0] == 0 and counts[2] == c['P']            # the empty group in front of a full one
    if c['pattern'] == 'tiles_ge_256' and c['P'] > dc.SCAN_BLOCK * dc.TILE:
        assert counts[1] + counts[2] == c['P'] - dc.SCAN_BLOCK * dc.TILE > 2 * dc.TILE   # three tiles in the scan's second pass


@pytest.mark.parametrize('case', [c for c in CASES if c[0] == 4101], ids=dc.case_id)
def test_restated_masks_are_the_torch_expressions(case):
    """the mask lines of densify.py::densify_and_clone / densify_and_split (with densify()'s NaN -> 0 in front) and the reference's prune
    (networks/gaussian_splatting.py:646-650) on CPU tensors"""
    c = dc.make_case(*case)
    accum, denom, scaling_, opacity, radii = (torch.from_numpy(c[k]) for k in ('accum', 'denom', 'log_scale', 'opacity', 'max_radii'))
    thr, extent = float(dc.MAX_GRAD), float(dc.SCENE_EXTENT)
    grads = accum / denom
    grads[grads.isnan()] = 0.0
    clone = (torch.norm(grads, dim=-1) >= thr) & (torch.exp(scaling_).amax(dim=1) <= extent)
    padded = torch.zeros((c['P'],))
    padded[:grads.shape[0]] = grads.squeeze()
    scaling = torch.exp(scaling_)
    split = (padded >= thr) & (scaling.amax(dim=1) > extent)
    drop_o = (torch.sigmoid(opacity) < float(dc.MIN_OPACITY)).squeeze()
    drop = torch.logical_or(torch.logical_or(drop_o, radii > float(dc.MAX_SCREEN)), torch.gt(scaling.amax(dim=1), float(dc.WORLD_LIMIT)))
    want = dc.masks_of(c)
    assert np.array_equal(clone.numpy(), want[0]) and np.array_equal(split.numpy(), want[1])
    assert np.array_equal(drop.numpy(), want[2]) and np.array_equal(drop_o.numpy(), dc.masks_of(c, with_radii=False)[2])
    # the two-call route's row list (clone appends, split then keeps the unselected originals AND the clones) is the one gather's
    P, N = c['P'], c['N']
    after_clone = np.concatenate([np.arange(P), np.nonzero(want[0])[0]])
    sel2 = np.concatenate([want[1], np.zeros(int(want[0].sum()), bool)])     # a fresh clone carries a zero gradient
    two_calls = np.concatenate([after_clone[~sel2], np.tile(after_clone[sel2], N)])
    assert np.array_equal(two_calls, dc.expected_select(want[0], want[1], N)[0])


def test_planted_ties_are_present_and_decide_as_stated():
    total = {k: 0 for k in dc.TIE_KINDS}
    for case in CASES:
        c = dc.make_case(*case)
        clone, split, drop = dc.masks_of(c)
        chosen = clone | split
        acc, den = c['accum'].reshape(-1), c['denom'].reshape(-1)
        t = c['ties']
        assert chosen[t['at']].all() and (acc[t['at']] == dc.MAX_GRAD * den[t['at']]).all() and np.isin(den[t['at']], (1, 2, 4)).all()
        assert not chosen[t['below']].any() and (np.nextafter(acc[t['below']], np.float32(1)) == dc.MAX_GRAD * den[t['below']]).all()
        assert not chosen[t['nan']].any() and (den[t['nan']] == 0).all() and (acc[t['nan']] == 0).all()
        assert chosen[t['inf']].all() and (den[t['inf']] == 0).all() and (acc[t['inf']] > 0).all()
        assert (acc[t['negative']] < 0).all() and not split[t['negative']].any()
        assert np.array_equal(clone[t['negative']], ~c['big'][t['negative']])
        assert (c['max_radii'][t['radius']] == dc.MAX_SCREEN).all() and np.array_equal(drop[t['radius']], ~c['keep'][t['radius']])
        total['radius'] += int((~drop[t['radius']]).sum())       # on the threshold and kept: nothing else drops these
        for k in dc.TIE_KINDS[:-1]:
            total[k] += t[k].size
        if c['P'] >= 2047 and c['pattern'].startswith('random_0.5'):
            assert all(t[k].size > 0 for k in dc.TIE_KINDS), case
    assert all(v > 0 for v in total.values()), total
    assert {c[0] for c in CASES} == set(dc.SIZES) and {c[2] for c in CASES} == {1, 2, 3}
    assert {c[1] for c in CASES if c[0] == 4101} == {c[1] for c in CASES if c[0] == 530_001} == set(dc.PATTERNS)


def test_split_children_truth_is_a_rotation_about_the_parent():
    """the fp64 truth of the children: |x - mu| = |normals * exp(ls)| (R is orthogonal whatever |q| is), R(0) = I"""
    N, d = 3, dc.split_children_inputs(257)
    xyz, ls = dc.split_children_truth(d['normals'], d['xyz'], d['log_scale'], d['rot'], N)
    v = d['normals'].astype(np.float64) * np.exp(d['log_scale'].astype(np.float64))
    off = xyz - d['xyz']
    assert np.allclose(np.linalg.norm(off, axis=1), np.linalg.norm(v, axis=1), rtol=1e-12, atol=1e-14)  # (mu <= 3 cancels)
    zero = ~d['rot'].any(1)
    assert zero.sum() >= 2 and np.array_equal(off[zero], (d['xyz'].astype(np.float64) + v - d['xyz'])[zero])
    assert np.allclose(ls, d['log_scale'] - np.log(0.8 * N), rtol=0, atol=1e-12)
    assert np.linalg.norm(d['rot'], axis=1)[~zero].min() < 0.02 and np.linalg.norm(d['rot'], axis=1).max() > 50
