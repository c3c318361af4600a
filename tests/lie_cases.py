"""Rows, launches and the per-row verdict shared by tests/test_lie_accuracy_cpu.py and tests/test_gpu_lie_accuracy.py (a plain helper).

Rows.  ``theta`` is drawn log-uniformly inside each decade from 1e-9 up to pi - 1e-3 (exp: one more band up to 6.0), directions uniformly
on the sphere; SE3 rows repeat every band at |tau| (|t| for group elements) = 1e-3, 1 and 1e2.  Exact rows are appended: theta = 0,
float32(1e-6) and the crossover of the series (``SERIES_THETA2`` of sk_gs_amd/lietorch.py) each with its nextafter on both sides, along an
axis and along a random direction; for log, quaternions whose |w| sits just below / just above 1e-6 on both sides of 0 (the at-pi
branches of so3_log) and quaternions with w < 0.  Group elements are the truth's exp of such tangents rounded to fp32, their quaternion
scaled by 0.7 .. 1.3 (the constructors normalise) -- the at-pi rows excepted, whose |w| is the point.  All inputs are fp32 numbers; the
truth is evaluated at exactly those numbers in fp64.

Launches.  The rows of a case are cut into launches of B = 1, 63, 64, 65, 1000, 1, 63 ... rows (the lane tail of a
one-lane-per-element kernel), every launch forward and backward.

Verdict.  Per row (lie_truth.row_error), the worst row of every band asserted against VALUE_BOUND / GRAD_BOUND -- the bounds
test_hip_group_operators_against_the_torch_bodies holds at O(1) angles, here per row in every band.  No row is dropped or masked; the one
canonicalisation is the sign of a whole quaternion for exp, inv and mul.
"""
import numpy as np

import lie_truth as T

VALUE_BOUND, GRAD_BOUND = 3e-6, 2e-5
BATCHES = (1, 63, 64, 65, 1000)
SCALES = (1e-3, 1.0, 1e2)
_EDGES = [10.0 ** e for e in range(-9, 1)] + [np.pi - 1e-3]
ANGLE_BANDS = list(zip(_EDGES[:-1], _EDGES[1:]))                              # 1e-9..1e-8, ..., 1e-1..1, 1..pi-1e-3
EXP_BAND = (np.pi - 1e-3, 6.0)
NEAR_IDENTITY_BANDS = [b for b in ANGLE_BANDS if b[1] <= 1e-2 * (1 + 1e-12)]
OPERATORS_ALL_BANDS = ('exp', 'log')
OPERATORS_NEAR_IDENTITY = ('inv', 'mul', 'adj', 'adjT', 'act', 'act4', 'vec', 'InitFromVec')
SIGN_FREE = ('exp', 'inv', 'mul')
AT_PI = 'at-pi / w<0'


def band_name(b):
    return f'{b[0]:.3g}..{b[1]:.3g}'


def _directions(g, n):
    d = g.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _with_scales(G, g, phi, label):
    """tangent rows (tau, phi) for every |tau| of SCALES (SO3: phi alone); returns rows, band labels, scales"""
    if G.K == 3:
        return phi, [label] * len(phi), np.ones(len(phi))
    rows = [np.concatenate([s * _directions(g, len(phi)), phi], -1) for s in SCALES]
    return np.concatenate(rows), [label] * (len(phi) * len(SCALES)), np.repeat(SCALES, len(phi))


def tangent_rows(G, bands, n_per, crossover_theta2, seed=0):
    """fp32 tangent rows over ``bands`` plus the exact rows; returns (a [R, K] float32, labels [R], scales [R])"""
    g = np.random.default_rng(seed)
    parts = []
    for b in bands:
        theta = 10.0 ** g.uniform(np.log10(b[0]), np.log10(b[1]), (n_per, 1))
        parts.append(_with_scales(G, g, _directions(g, n_per) * theta, band_name(b)))
    one = np.float32(1)
    exact = [np.float32(0)]
    for c in (np.float32(1e-6), np.sqrt(np.float32(crossover_theta2))):
        exact += [np.nextafter(c, np.float32(0)), c, np.nextafter(c, one)]
    exact = [t for t in exact if t <= bands[-1][1]]
    th = np.array(exact, np.float64)[:, None]
    phi = np.concatenate([th * np.array([[1.0, 0, 0]]), th * np.array([[0, 0, -1.0]]), th * _directions(g, len(th))])
    parts.append(_with_scales(G, g, phi, 'exact'))
    a = np.concatenate([p[0] for p in parts]).astype(np.float32)
    return a, np.array(sum((p[1] for p in parts), [])), np.concatenate([p[2] for p in parts])


def group_rows(G, bands, n_per, crossover_theta2, seed=0, at_pi=False):
    """fp32 group elements: exp of tangent_rows rounded to fp32 with the quaternion scaled by 0.7 .. 1.3; ``at_pi`` appends the rows of
    so3_log's branches around w = 0 and rows with w < 0"""
    a, labels, scales = tangent_rows(G, bands, n_per, crossover_theta2, seed)
    g = np.random.default_rng(seed + 1000)
    X = G.exp(a.astype(np.float64)).astype(np.float32)
    X[:, -4:] *= g.uniform(0.7, 1.3, (len(X), 1)).astype(np.float32)
    if at_pi:
        e = np.float32(1e-6)
        ws = [np.float32(0.9e-6), np.nextafter(e, np.float32(0)), e, np.nextafter(e, np.float32(1)), np.float32(1.1e-6)]
        ws = np.array(ws + [-w for w in ws] + [-1e-3, -0.1, -0.5, -0.9, -0.999, -0.9999999, -1.0], np.float64)
        ws = np.repeat(ws, 4)
        q = np.concatenate([_directions(g, len(ws)) * np.sqrt(1.0 - ws * ws)[:, None], ws[:, None]], -1)
        if G.K == 3:
            X2, s2 = q, np.ones(len(q))
        else:
            X2 = np.concatenate([np.concatenate([s * _directions(g, len(q)), q], -1) for s in SCALES])
            s2 = np.repeat(SCALES, len(q))
        X = np.concatenate([X, X2.astype(np.float32)])
        labels, scales = np.concatenate([labels, [AT_PI] * len(X2)]), np.concatenate([scales, s2])
    return X, labels, scales


def launches(n):
    """slices that cut n rows into launches of BATCHES rows, cyclically"""
    out, i, k = [], 0, 0
    while i < n:
        b = min(BATCHES[k % len(BATCHES)], n - i)
        out.append(slice(i, i + b))
        i, k = i + b, k + 1
    return out


def make_case(G, op, crossover_theta2, n_per, seed=0):
    """(x, y, cot, labels, scales) of operator ``op``: fp32 arrays"""
    g = np.random.default_rng(seed + 7)
    K, N = G.K, G.N
    if op == 'exp':
        x, labels, scales = tangent_rows(G, ANGLE_BANDS + [EXP_BAND], n_per, crossover_theta2, seed)
    elif op == 'log':
        x, labels, scales = group_rows(G, ANGLE_BANDS, n_per, crossover_theta2, seed, at_pi=True)
    else:
        x, labels, scales = group_rows(G, NEAR_IDENTITY_BANDS, n_per, crossover_theta2, seed)
    R = len(x)
    y = None
    if op == 'mul':                                                        # near the identity as well, other rows' transforms
        y = group_rows(G, NEAR_IDENTITY_BANDS, n_per, crossover_theta2, seed + 1)[0][g.permutation(R)]
    elif op in ('adj', 'adjT'):
        y = g.standard_normal((R, K))
    elif op == 'act':
        y = g.standard_normal((R, 3))
    elif op == 'act4':
        y = g.standard_normal((R, 4))
    width = {'exp': N, 'inv': N, 'mul': N, 'vec': N, 'InitFromVec': N, 'log': K, 'adj': K, 'adjT': K, 'act': 3, 'act4': 4}[op]
    cot = g.standard_normal((R, width))
    f32 = lambda t: None if t is None else np.ascontiguousarray(t, np.float32)  # noqa: E731
    return f32(x), f32(y), f32(cot), labels, scales


def run_standin(L, group, op, x, y, cot, device, dtype):
    """operator ``op`` through the stand-in's public interface (sk_gs_amd.lietorch: the HIP launches for fp32 rows on a HIP device, the
    torch bodies otherwise), one forward and one backward per launch of ``launches``; returns (value, dX, dY) as fp64 numpy arrays"""
    import torch
    G = {'SO3': L.SO3, 'SE3': L.SE3}[group]
    f = {'exp': lambda a, b: G.exp(a).data, 'log': lambda a, b: G(a).log(), 'inv': lambda a, b: G(a).inv().data,
         'mul': lambda a, b: (G(a) * G(b)).data, 'adj': lambda a, b: G(a).adj(b), 'adjT': lambda a, b: G(a).adjT(b),
         'act': lambda a, b: G(a).act(b), 'act4': lambda a, b: G(a).act(b), 'vec': lambda a, b: G(a).vec(),
         'InitFromVec': lambda a, b: G.InitFromVec(a).data}[op]
    conv = lambda t, s: torch.from_numpy(t[s]).to(device=device, dtype=dtype)  # noqa: E731
    outs, dxs, dys = [], [], []
    for s in launches(len(x)):
        a = conv(x, s).requires_grad_()
        b = None if y is None else conv(y, s).requires_grad_()
        out = f(a, b)
        (out * conv(cot, s)).sum().backward()
        outs.append(out.detach().cpu().double().numpy())
        dxs.append(a.grad.cpu().double().numpy())
        dys.append(None if b is None else b.grad.cpu().double().numpy())
    return np.concatenate(outs), np.concatenate(dxs), None if y is None else np.concatenate(dys)


def errors(group, op, x, y, cot, got):
    """per-row errors of ``got`` = (value, dX, dY) against the truth at the fp32 inputs: {'value' | 'dX' | 'dY': [R]}"""
    G = T.GROUPS[group]
    c64 = cot.astype(np.float64)
    want = T.operator(G, op, x.astype(np.float64), None if y is None else y.astype(np.float64), c64)
    value = T.align_quaternion_sign(got[0], want[0]) if op in SIGN_FREE else got[0]
    err = {'value': T.row_error(value, want[0]), 'dX': T.row_error(got[1], want[1], c64)}
    if want[2] is not None:
        err['dY'] = T.row_error(got[2], want[2], c64)
    return err


def table(group, op, err, labels, scales):
    """[(band, what, worst per-row error, |tau| of that row)] in the order the bands were generated, and its printable form"""
    rows = []
    for band in dict.fromkeys(labels.tolist()):
        m = labels == band
        for what, e in err.items():
            i = int(np.argmax(np.where(m, e, -1.0)))
            rows.append((band, what, float(e[i]), float(scales[i])))
    text = '\n'.join(f'[lie-accuracy] {group:3s} {op:15s} {band:18s} {what:5s} {e:9.2e}  (|tau| {s:g})' for band, what, e, s in rows)
    return rows, text


def failures(rows):
    return [(band, what, e, s) for band, what, e, s in rows if not e <= (VALUE_BOUND if what == 'value' else GRAD_BOUND)]
