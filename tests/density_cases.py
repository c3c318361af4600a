"""Decisions, row lists and seeded cases of adaptive density control, shared by tests/test_density_cases_cpu.py and
tests/test_gpu_density_control.py (a plain helper: numpy only, no GPU, no reference checkout).

Restatement.  The masks of ``densify_and_clone`` / ``densify_and_split`` / ``prune`` (networks/gaussian_splatting.py:589-650) written
out once more, evaluated in ``dtype`` (float64: the truth; float32: the arithmetic the kernels use) at exactly the float32 inputs:
    g      = accum / denom,  NaN -> 0                                                   (:639-640)
    clone  = |g| >= t  and  max exp(log_scale) <= extent                                (:627-631)
    split  =  g  >= t  and  max exp(log_scale) >  extent                                (:595-599)
    drop   = sigmoid(o) < min_opacity  [or  max_radii > max_screen_size  or  max exp(log_scale) > world_limit]   (:646-650)
and the row lists the one-gather formulation promises (sk_gs_amd/densify.py):
    select: rows = nonzero(~split) ++ nonzero(clone) ++ nonzero(split) x N (whole blocks),  counts = [n_keep, n_clone, n_split]
    prune:  rows = nonzero(~drop),  counts = [n_keep]

Cases.  ``make_case(P, pattern, N)`` first decides what every Gaussian IS (selected by the gradient or not, large or small, kept by
prune or dropped and why) and then draws numbers that realise it with room to spare: everything that passes through exp, the sigmoid or
an inexact division sits at least ``MARGIN`` (relative) from its threshold, so float32 and float64 take the same side and EVERY row can be
compared, none left out.  Ties are planted only where float32 is exact, and never change what a row is:
    'at'       accum = t * denom with denom in {1, 2, 4}: the quotient is t exactly -> selected                       (>=, not >)
    'below'    accum = the float32 just below that                                   -> not selected
    'nan'      denom = 0, accum = 0: NaN -> 0                                        -> not selected
    'inf'      denom = 0, accum > 0: +inf                                            -> selected
    'negative' accum < 0 with |g| well over t: cloned when small (the norm), NOT split when large (the signed value)
    'radius'   max_radii == max_screen_size exactly                                  -> not pruned                    (>, not >=)
The thresholds themselves are float32 numbers (t = 2^-12 is exact in every format).

Patterns say which Gaussians the gradient selects (and which ones prune keeps): 'random_0.5', 'random_0.01', 'none', 'all_clone',
'all_split' (counts[0] == 0: an empty group in front of a full one), 'tile_last' / 'tile_first' (one Gaussian per compaction tile of
2048, in its last / first slot), 'tiles_ge_256' (only tiles the scan reaches in its second pass), 'very_last'.
"""
import functools

import numpy as np

TILE = 2048            # Gaussians per compaction tile (csrc/densify.hip: CTILE)
SCAN_BLOCK = 256       # tiles per pass of the one-workgroup scan (TILE_T)
MARGIN = 1e-3

MAX_GRAD = np.float32(2.0 ** -12)
EXTENT = 5.0                                   # scene extent: densify compares with 0.01 x, prune's world limit is 0.1 x
SCENE_EXTENT = np.float32(0.01 * EXTENT)
WORLD_LIMIT = np.float32(0.1 * EXTENT)
MIN_OPACITY = np.float32(0.05)
MAX_SCREEN = np.float32(20.0)

SIZES = (0, 1, 7, 2047, 2048, 2049, 4101, 100_003, 524_288, 530_001)
PATTERNS = ('random_0.5', 'random_0.01', 'none', 'all_clone', 'all_split', 'tile_last', 'tile_first', 'tiles_ge_256', 'very_last')
TIE_KINDS = ('at', 'below', 'nan', 'inf', 'negative', 'radius')


# ------------------------------------------------------------------------------------------------------ restatement
def _max_scale(log_scale, dtype):
    return np.exp(np.asarray(log_scale, np.float32).reshape(-1, 3).astype(dtype)).max(1)


def clone_split_masks(accum, denom, log_scale, max_grad, scene_extent, dtype=np.float64):
    """(clone, split) of densify(); every operand converted to ``dtype`` first"""
    a, d = np.asarray(accum, np.float32).reshape(-1).astype(dtype), np.asarray(denom, np.float32).reshape(-1).astype(dtype)
    with np.errstate(divide='ignore', invalid='ignore'):
        g = a / d
    g[np.isnan(g)] = 0
    big = _max_scale(log_scale, dtype) > dtype(scene_extent)
    return (np.abs(g) >= dtype(max_grad)) & ~big, (g >= dtype(max_grad)) & big


def prune_mask(opacity_logit, max_radii, log_scale, min_opacity, max_screen_size, world_limit, dtype=np.float64):
    """the Gaussians prune() drops; ``max_radii`` None: the opacity test alone (the reference's max_screen_size = 0)"""
    o = np.asarray(opacity_logit, np.float32).reshape(-1).astype(dtype)
    drop = dtype(1) / (dtype(1) + np.exp(-o)) < dtype(min_opacity)
    if max_radii is not None:
        drop = drop | (np.asarray(max_radii, np.float32).astype(dtype) > dtype(max_screen_size))
        drop = drop | (_max_scale(log_scale, dtype) > dtype(world_limit))
    return drop


def expected_select(clone, split, N):
    rows = np.concatenate([np.nonzero(~split)[0], np.nonzero(clone)[0], np.tile(np.nonzero(split)[0], N)]).astype(np.int64)
    return rows, np.array([(~split).sum(), clone.sum(), split.sum()], np.int32)


def expected_prune(drop):
    rows = np.nonzero(~drop)[0].astype(np.int64)
    return rows, np.array([rows.size], np.int32)


# ------------------------------------------------------------------------------------------------------------ cases
def pattern_mask(P, pattern, g):
    i = np.arange(P)
    if pattern.startswith('random_'):
        return g.random(P) < float(pattern.split('_')[1])
    return {'none': np.zeros(P, bool), 'all_clone': np.ones(P, bool), 'all_split': np.ones(P, bool),
            'tile_last': (i % TILE == TILE - 1) | (i == P - 1), 'tile_first': i % TILE == 0,
            'tiles_ge_256': i >= SCAN_BLOCK * TILE, 'very_last': i == P - 1}[pattern]


def _between(g, n, lo, hi):
    return g.uniform(lo, hi, n)


@functools.lru_cache(maxsize=None)
def make_case(P, pattern, N, seed=0):
    """dict of float32 inputs (accum [P,1], denom [P,1], log_scale [P,3], opacity [P,1], max_radii [P]), the intent masks
    (sel, big, keep), ``ties`` (kind -> row indices) and the sizes.  Treat it as read-only: it is shared between tests."""
    g = np.random.default_rng([seed, P, PATTERNS.index(pattern), N])
    pat = pattern_mask(P, pattern, g)                     # the gradient selects these rows; prune (with radii) keeps these rows
    # ---- what a row is
    reason = g.integers(1, 8, P)                          # bit 0: transparent, bit 1: fills the screen, bit 2: too large for the world
    reason[pat] = 0
    huge = (reason & 4) != 0
    big = {'all_clone': np.zeros(P, bool), 'all_split': np.ones(P, bool)}.get(pattern, g.random(P) < 0.5) | huge
    sel = pat
    kind = g.integers(0, 12, P)                           # how the row realises it: 0 / 1 / 2 = the exact ways, else with a margin
    t = np.float64(MAX_GRAD)
    # ---- gradient statistics
    denom = g.integers(1, 6, P).astype(np.float64)
    ratio = np.where(sel, _between(g, P, 1 + MARGIN, 3.0), _between(g, P, 0.0, 1 - MARGIN))
    accum = (ratio * t * denom).astype(np.float32)
    denom = denom.astype(np.float32)
    pow2 = np.float32(2.0) ** g.integers(0, 3, P).astype(np.float32)
    ties = {}
    for name, rows, acc, den in (
            ('at', sel & (kind == 0), MAX_GRAD * pow2, pow2),
            ('inf', sel & (kind == 1), accum, np.zeros(P, np.float32)),
            ('negative', (kind == 2) & ((sel & ~big) | (~sel & big)), -np.float32(t * 2.5) * denom, denom),
            ('below', ~sel & (kind == 0), np.nextafter(MAX_GRAD * pow2, np.float32(0)), pow2),
            ('nan', ~sel & (kind == 1), np.zeros(P, np.float32), np.zeros(P, np.float32))):
        accum, denom = np.where(rows, acc, accum).astype(np.float32), np.where(rows, den, denom).astype(np.float32)
        ties[name] = np.nonzero(rows)[0]
    # ---- scales: small < SCENE_EXTENT < large < WORLD_LIMIT < huge, each with MARGIN to spare
    e, w = np.float64(SCENE_EXTENT), np.float64(WORLD_LIMIT)
    assert 4.0 * e < (1 - MARGIN) * w
    top = np.where(huge, w * _between(g, P, 1 + MARGIN, 3.0),
                   np.where(big, e * _between(g, P, 1 + MARGIN, 4.0), e * _between(g, P, 0.05, 1 - MARGIN)))
    log_scale = np.log(top)[:, None] - g.uniform(0.0, 2.0, (P, 3))
    log_scale[np.arange(P), g.integers(0, 3, P)] = np.log(top)
    # ---- opacity and screen radius
    drop_o, drop_r = (reason & 1) != 0, (reason & 2) != 0
    sig = np.float64(MIN_OPACITY) * np.where(drop_o, _between(g, P, 0.02, 1 - MARGIN), _between(g, P, 1 + MARGIN, 19.0))
    opacity = np.log(sig / (1 - sig))
    max_radii = np.float64(MAX_SCREEN) * np.where(drop_r, _between(g, P, 1 + MARGIN, 3.0), _between(g, P, 0.0, 1 - MARGIN))
    on_radius = ~drop_r & (g.integers(0, 12, P) == 0)
    max_radii = np.where(on_radius, np.float64(MAX_SCREEN), max_radii)
    ties['radius'] = np.nonzero(on_radius)[0]
    return dict(P=P, N=N, pattern=pattern, sel=sel, big=big, keep=pat, keep_opacity_only=~drop_o, ties=ties,
                accum=np.ascontiguousarray(accum.reshape(P, 1)), denom=np.ascontiguousarray(denom.reshape(P, 1)),
                log_scale=np.ascontiguousarray(log_scale.astype(np.float32)),
                opacity=np.ascontiguousarray(opacity.astype(np.float32).reshape(P, 1)),
                max_radii=np.ascontiguousarray(max_radii.astype(np.float32)))


def case_list():
    """(P, pattern, N): every size at 'random_0.5' with N = 2, every pattern at 4101 and at 530 001 with N cycling through 1, 2, 3, and
    the two patterns with the most splits at the N they miss that way"""
    cases = [(P, 'random_0.5', 2) for P in SIZES]
    for P in (4101, 530_001):
        cases += [(P, pat, (1, 2, 3)[i % 3]) for i, pat in enumerate(PATTERNS)]
        cases += [(P, 'random_0.5', 3), (P, 'all_split', 3), (P, 'all_split', 1)]
    assert len(set(cases)) == len(cases)
    return cases


def case_id(c):
    return f'{c[0]}-{c[1]}-N{c[2]}'


def masks_of(case, dtype=np.float64, with_radii=True):
    """(clone, split, drop) of a case in ``dtype``"""
    clone, split = clone_split_masks(case['accum'], case['denom'], case['log_scale'], MAX_GRAD, SCENE_EXTENT, dtype)
    drop = prune_mask(case['opacity'], case['max_radii'] if with_radii else None, case['log_scale'], MIN_OPACITY, MAX_SCREEN,
                      WORLD_LIMIT, dtype)
    return clone, split, drop


# --------------------------------------------------------------------------------------------- split children: truth
def split_children_inputs(n, seed=0):
    """float32 inputs of skgs_split_children: normals, xyz, log_scale in [-12, 3], quaternions of norm 1e-2 .. 1e2 and a few all-zero"""
    g = np.random.default_rng([seed, n, 77])
    q = g.standard_normal((n, 4))
    q *= (10.0 ** g.uniform(-2, 2, (n, 1))) / np.linalg.norm(q, axis=1, keepdims=True)
    q[g.random(n) < 0.05] = 0.0
    if n >= 2:
        q[n - 1] = 0.0
    f = lambda a: np.ascontiguousarray(a.astype(np.float32))  # noqa: E731
    return dict(normals=f(g.standard_normal((n, 3))), xyz=f(g.uniform(-3, 3, (n, 3))), log_scale=f(g.uniform(-12, 3, (n, 3))), rot=f(q))


def split_children_truth(normals, xyz, log_scale, rot, N):
    """fp64 at the float32 inputs: mu + R(q / max(|q|, 1e-12)) (normals * exp(ls)),  log(exp(ls) / (0.8 N))
    (gaussian_splatting.py:601-611; xyzw quaternion, my_ext/ops_3d/quaternion.py:162-172; F.normalize's eps makes R(0) = I)"""
    nrm, mu, ls, q = (np.asarray(a, np.float32).astype(np.float64) for a in (normals, xyz, log_scale, rot))
    q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)
    x, y, z, w = q.T
    R = np.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
                  2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x,
                  2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, 1 - 2 * x * x - 2 * y * y], -1).reshape(-1, 3, 3)
    s = np.exp(ls)
    return mu + np.einsum('nij,nj->ni', R, nrm * s), np.log(s / (0.8 * N))


def split_bound(torch_value, truth, factor):
    """max-norm bound of a tensor: ``factor`` x the error of the float32 torch lines against the same truth, at least 4 ulp of the
    tensor's largest magnitude; returns (bound, torch error)"""
    ref_err = float(np.abs(np.asarray(torch_value, np.float64) - truth).max()) if truth.size else 0.0
    floor = 4 * float(np.spacing(np.float32(np.abs(truth).max()))) if truth.size else 0.0
    return max(factor * ref_err, floor), ref_err
