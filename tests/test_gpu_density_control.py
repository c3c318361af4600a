"""Density control's kernels (csrc/densify.hip) through the C ABI, as sk_gs_amd/densify.py and FusedAdam.gather_rows call it, against
the plain restatement of tests/density_cases.py: the row list of skgs_densify_select / skgs_prune_select row for row, skgs_gather_rows
against plain indexing, skgs_split_children against its fp64 value, densify() against densify_and_clone + densify_and_split -- and
that no launch writes outside what it was given (sentinels behind every output)."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import density_cases as dc
from helpers import REF_ERR_FACTOR, rel_err, to_np

pytestmark = pytest.mark.gpu

CASES = dc.case_list()
ROW_SENTINEL = -0x5a5a5a5a5a5a5a5b
BYTE_SENTINEL = 0xa5
INT_SENTINEL = 0x5a5a5a5a
GUARD = 64


def _lib():
    from sk_gs_amd import _C
    lib = _C.load_library()
    lib.skgs_select_workspace_bytes.restype = C.c_size_t
    return lib, _C


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)


def _dev(a):
    return torch.from_numpy(a).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _first_difference(got, want):
    bad = np.nonzero(got != want)[0]
    return f'{bad.size} rows differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}' if bad.size else ''


def _select_buffers(lib, P, n_rows, n_counts):
    ws_bytes = int(lib.skgs_select_workspace_bytes(C.c_int32(P)))
    rows = torch.full((n_rows + GUARD,), ROW_SENTINEL, dtype=torch.int64, device='cuda')
    ws = torch.full((ws_bytes + GUARD,), BYTE_SENTINEL, dtype=torch.uint8, device='cuda')
    counts = torch.full((n_counts + GUARD,), -1, dtype=torch.int32, device='cuda')
    return rows, ws, counts, ws_bytes


def _check_select_outputs(P, rows, ws, counts, ws_bytes, want_rows, want_counts):
    torch.cuda.synchronize()
    got_counts, got, ws_h = to_np(counts), to_np(rows), to_np(ws)
    assert np.array_equal(got_counts[:want_counts.size], want_counts), (got_counts[:want_counts.size], want_counts)
    assert (got_counts[want_counts.size:] == -1).all(), 'counts written behind the group sizes'
    n_out = want_rows.size
    assert np.array_equal(got[:n_out], want_rows), _first_difference(got[:n_out], want_rows)
    assert (got[n_out:] == ROW_SENTINEL).all(), f'rows written from n_out = {n_out} on: {np.nonzero(got[n_out:] != ROW_SENTINEL)[0][:8]}'
    assert (ws_h[ws_bytes:] == BYTE_SENTINEL).all(), 'workspace written beyond skgs_select_workspace_bytes(P)'
    # inside the workspace: P flag bytes, then the tile counters from the next multiple of 16 -- the bytes between are nobody's
    assert (ws_h[P:(P + 15) & ~15] == BYTE_SENTINEL).all(), 'the padding between the flags and the tile counters was written'
    assert ws_bytes >= ((P + 15) & ~15) + (P + dc.TILE - 1) // dc.TILE * 16


@pytest.mark.parametrize('case', CASES, ids=dc.case_id)
def test_densify_select_row_list_is_the_restatement(case):
    """counts and rows[:n_out] of skgs_densify_select, every row; rows from n_out on, the guard behind the workspace and the guard behind
    counts untouched.  P = 0: zero counts, rows untouched."""
    c = dc.make_case(*case)
    P, N = c['P'], c['N']
    lib, _C = _lib()
    clone, split, _ = dc.masks_of(c)
    want_rows, want_counts = dc.expected_select(clone, split, N)
    rows, ws, counts, ws_bytes = _select_buffers(lib, P, (2 + N) * P, 3)
    acc, den, ls = _dev(c['accum']), _dev(c['denom']), _dev(c['log_scale'])
    _C._check(lib.skgs_densify_select(C.c_int32(P), _p(acc), _p(den), _p(ls), C.c_float(float(dc.MAX_GRAD)),
                                      C.c_float(float(dc.SCENE_EXTENT)), C.c_int32(N), _p(rows), _p(counts), _p(ws), _C._stream()))
    _check_select_outputs(P, rows, ws, counts, ws_bytes, want_rows, want_counts)
    if P == 0:
        assert want_rows.size == 0 and not want_counts.any()


@pytest.mark.parametrize('with_radii', [True, False], ids=['radii', 'opacity_only'])
@pytest.mark.parametrize('case', CASES, ids=dc.case_id)
def test_prune_select_row_list_is_the_restatement(case, with_radii):
    """skgs_prune_select with max_radii2D set (the pattern itself survives: one Gaussian per tile, only tiles >= 256, ...) and NULL (the
    opacity test alone)"""
    c = dc.make_case(*case)
    P = c['P']
    lib, _C = _lib()
    want_rows, want_counts = dc.expected_prune(dc.masks_of(c, with_radii=with_radii)[2])
    rows, ws, counts, ws_bytes = _select_buffers(lib, P, P, 1)
    op, ls, radii = _dev(c['opacity']), _dev(c['log_scale']), _dev(c['max_radii']) if with_radii else None
    _C._check(lib.skgs_prune_select(C.c_int32(P), _p(op), _p(radii), _p(ls), C.c_float(float(dc.MIN_OPACITY)),
                                    C.c_float(float(dc.MAX_SCREEN)), C.c_float(float(dc.WORLD_LIMIT)), _p(rows), _p(counts), _p(ws),
                                    _C._stream()))
    _check_select_outputs(P, rows, ws, counts, ws_bytes, want_rows, want_counts)
    if with_radii:
        assert np.array_equal(want_rows, np.nonzero(c['keep'])[0])


# ------------------------------------------------------------------------------------------------------------ gather
WIDTHS = (1, 3, 4, 45, 48)


def _descriptor_table(pairs):
    blob = bytearray()
    for src, dst, width, fresh in pairs:
        blob += struct.pack('<QQii', src.data_ptr(), dst.data_ptr(), width, fresh)
    return torch.frombuffer(blob, dtype=torch.uint8).cuda()


@pytest.mark.parametrize('source', ['more_rows', 'fewer_rows'])
@pytest.mark.parametrize('keep', ['none', 'third', 'all'])
@pytest.mark.parametrize('n_out', [1, 1000, 200_003])
def test_gather_rows_is_plain_indexing(n_out, keep, source):
    """ONE launch over ten tensors (row widths 1, 3, 4, 45, 48, each with fresh_is_zero 0 and 1), duplicates in ``rows``, against
    ``src[rows]`` with the rows from n_keep on zeroed where asked, bit for bit; a guard row behind every destination.  At 200 003 rows
    the width-48 tensors have 9.6 M elements: more than the 8192 x 1024 one sweep of the capped grid covers."""
    lib, _C = _lib()
    n_keep = {'none': 0, 'third': n_out // 3, 'all': n_out}[keep]
    n_src = 2 * n_out + 5 if source == 'more_rows' else max(1, n_out // 2)
    g = torch.Generator(device='cuda').manual_seed(n_out * 7 + n_keep)
    rows = torch.randint(0, n_src, (n_out,), device='cuda', generator=g)
    rows[::5] = int(rows[0])                                               # duplicates whatever the source size
    rows[-1] = n_src - 1                                                   # the last source row is reachable
    if n_out > 1:
        assert int(torch.unique(rows).numel()) < n_out
    pairs = []
    for width in WIDTHS:
        for fresh in (0, 1):
            src = torch.randn((n_src, width), device='cuda', generator=g)
            dst = torch.full((n_out + 1, width), INT_SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)
            pairs.append((src, dst, width, fresh))
    assert n_out < 200_000 or n_out * max(WIDTHS) > 8192 * 1024
    table = _descriptor_table(pairs)
    _C._check(lib.skgs_gather_rows(C.c_int32(len(pairs)), _p(table), C.c_int64(n_out), C.c_int64(n_keep), _p(rows),
                                   C.c_int32(max(WIDTHS)), _C._stream()))
    torch.cuda.synchronize()
    for src, dst, width, fresh in pairs:
        want = src[rows]
        if fresh:
            want[n_keep:] = 0.0
        assert torch.equal(_bits(dst[:n_out]), _bits(want)), (width, fresh)
        assert bool((_bits(dst[n_out:]) == INT_SENTINEL).all()), f'guard row of width {width} written'


def test_gather_rows_early_returns_and_bad_sizes():
    lib, _C = _lib()
    src = torch.randn(5, 3, device='cuda')
    dst = torch.full((5, 3), INT_SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)
    rows = torch.arange(5, device='cuda')
    table = _descriptor_table([(src, dst, 3, 0)])
    st = _C._stream()
    _C._check(lib.skgs_gather_rows(C.c_int32(0), C.c_void_p(None), C.c_int64(5), C.c_int64(5), C.c_void_p(None), C.c_int32(3), st))
    _C._check(lib.skgs_gather_rows(C.c_int32(1), _p(table), C.c_int64(0), C.c_int64(0), _p(rows), C.c_int32(3), st))
    torch.cuda.synchronize()
    assert bool((_bits(dst) == INT_SENTINEL).all())
    for n_out, n_keep, width in ((5, 6, 3), (-1, 0, 3), (5, -1, 3), (5, 5, 0)):
        with pytest.raises(_C.SkgsError):
            _C._check(lib.skgs_gather_rows(C.c_int32(1), _p(table), C.c_int64(n_out), C.c_int64(n_keep), _p(rows), C.c_int32(width), st))
    torch.cuda.synchronize()
    assert bool((_bits(dst) == INT_SENTINEL).all())


# ---------------------------------------------------------------------------------------------------- split children
def _torch_split_lines(normals, xyz, log_scale, rot, N):
    """the float32 lines of densify.py::densify_and_split for rows that are all selected, the normal draws given"""
    from sk_gs_amd import densify
    scaling = torch.exp(log_scale)
    samples = normals * scaling                                       # torch.normal(mean=0, std=stds) = stds * standard normal
    rots = densify.quaternion_to_R(rot)
    return densify._rotate(rots, samples) + xyz, torch.log(scaling / (0.8 * N))


@pytest.mark.parametrize('N', [1, 2, 3, 10])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 5000])
def test_split_children_against_fp64(n, N):
    """skgs_split_children against mu + R(q / |q|) (normals * exp(ls)) and log(exp(ls) / (0.8 N)) in fp64 at the float32 inputs.
    Bound per tensor: REF_ERR_FACTOR (2: two fp32 evaluations of one expression) x the max-norm error of the float32 torch lines of
    densify_and_split against the same fp64 value, at least 4 ulp of the tensor's largest magnitude -- computed here from torch, never
    from the kernel.  Rows from n on, and rot, stay bit-identical.

    Measured on the MI355X (kernel error, torch restatement error; absolute, max-norm), the worst of the 20 cases per tensor:
      xyz        1.27e-5 against 1.02e-5 (n = 5000, N = 1; bound 2.04e-5); the largest kernel error is 1.31e-5 (n = 5000, N = 10), torch's too
      log_scale  1.88e-6 against 9.27e-7 (N = 1, every n >= 255; bound = the 4 ulp floor, 3.81e-6: |log_scale| reaches 12, one ulp is 9.5e-7);
                 N = 2, 3, 10: 1.41e-6 ... 1.44e-6 on both sides"""
    lib, _C = _lib()
    extra = 3
    d = dc.split_children_inputs(n + extra, seed=N)
    t = {k: _dev(v) for k, v in d.items()}
    before = {k: v.clone() for k, v in t.items()}
    want_xyz, want_ls = dc.split_children_truth(d['normals'][:n], d['xyz'][:n], d['log_scale'][:n], d['rot'][:n], N)
    ref_xyz, ref_ls = _torch_split_lines(*(before[k][:n] for k in ('normals', 'xyz', 'log_scale', 'rot')), N)
    _C._check(lib.skgs_split_children(C.c_int32(n), C.c_int32(N), _p(t['normals']), _p(t['xyz']), _p(t['log_scale']), _p(t['rot']),
                                      _C._stream()))
    torch.cuda.synchronize()
    for name, got, ref, want in (('xyz', t['xyz'], ref_xyz, want_xyz), ('log_scale', t['log_scale'], ref_ls, want_ls)):
        bound, ref_err = dc.split_bound(to_np(ref), want, REF_ERR_FACTOR)
        err = float(np.abs(to_np(got[:n]).astype(np.float64) - want).max())
        print(f'[split_children] n={n} N={N} {name}: kernel error {err:.3e}, torch restatement error {ref_err:.3e}, bound {bound:.3e}')
        assert err <= bound, (name, err, ref_err, bound)
        assert torch.equal(_bits(got[n:]), _bits(before[name][n:])), f'{name}: rows from n on were written'
    assert torch.equal(_bits(t['rot']), _bits(before['rot'])) and torch.equal(_bits(t['normals']), _bits(before['normals']))


# ------------------------------------------------------------------------------------- densify() against the two calls
def _model_and_optimizer(case):
    from sk_gs_amd import densify
    from sk_gs_amd.model import SkinnedGaussians
    from sk_gs_amd.optim import FusedAdam
    P = case['P']
    model = SkinnedGaussians(P, 8, 4, num_frames=2, seed=5).cuda()
    names = densify._names(model)
    opt = FusedAdam([{'params': [getattr(model, a)], 'lr': 1e-3 * (i + 1), 'name': n} for i, (a, n) in enumerate(names.items())],
                    eps=1e-15)
    g = torch.Generator().manual_seed(11)
    for _ in range(2):
        for a in names:
            p = getattr(model, a)
            p.grad = torch.randn(p.shape, generator=g).cuda()
        opt.step()
    model._scaling.data.copy_(_dev(case['log_scale']))         # the sizes the case decided, the moments of the two steps
    stats = densify.DensifyStats(P, 'cuda')
    stats.xyz_gradient_accum, stats.denom = _dev(case['accum']), _dev(case['denom'])
    stats.max_radii2D = _dev(case['max_radii'])
    return model, opt, stats, names


def _state(model, opt, names):
    out = {}
    for a in names:
        p = getattr(model, a)
        out[a] = (p.detach().clone(), opt.state[p]['exp_avg'].clone(), opt.state[p]['exp_avg_sq'].clone())
    return out


def test_densify_is_clone_then_split_row_for_row():
    """densify.densify (one device-side selection, one gather) against densify_and_clone followed by densify_and_split (torch masks, two
    gathers) on identical models after two Adam steps: same P, every parameter and both moments bit-identical -- the children's _xyz
    (other random draws) and _scaling excepted, the latter held to the bound of test_split_children_against_fp64 -- and both equal to
    plain indexing of the state before with the restatement's row list.  Measured on the MI355X, children's _scaling: densify() 6.9e-7
    from the fp64 value, the torch route 4.5e-7, bound 1.9e-6 (the 4 ulp floor)."""
    from sk_gs_amd import densify
    case = dc.make_case(4101, 'random_0.5', 2)
    N, thr, extent = case['N'], float(dc.MAX_GRAD), dc.EXTENT
    assert np.float32(0.01 * extent) == dc.SCENE_EXTENT
    clone, split, _ = dc.masks_of(case)
    rows, (n_keep, n_clone, n_split) = dc.expected_select(clone, split, N)
    n_old = int(n_keep + n_clone)
    one, opt1, stats1, names = _model_and_optimizer(case)
    two, opt2, stats2, _ = _model_and_optimizer(case)
    before = _state(one, opt1, names)
    for a, s in _state(two, opt2, names).items():
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(s, before[a])), a
    densify.densify(one, opt1, stats1, max_grad=thr, extent=extent, generator=torch.Generator(device='cuda').manual_seed(3), N=N)
    grads = stats2.xyz_gradient_accum / stats2.denom
    grads[grads.isnan()] = 0.0
    densify.densify_and_clone(two, opt2, grads, thr, 0.01 * extent, stats2)
    assert two.P == case['P'] + n_clone
    densify.densify_and_split(two, opt2, grads, thr, 0.01 * extent, N=N, stats=stats2,
                              generator=torch.Generator(device='cuda').manual_seed(3))
    assert one.P == two.P == rows.size == case['P'] + n_clone + (N - 1) * n_split
    got1, got2 = _state(one, opt1, names), _state(two, opt2, names)
    idx = _dev(rows)
    for a in names:
        upto = n_old if a in ('_xyz', '_scaling') else rows.size
        for k, (x, y, b) in enumerate(zip(got1[a], got2[a], before[a])):
            assert x.shape == y.shape == (rows.size,) + tuple(b.shape[1:]), (a, k)
            full = k > 0 or upto == rows.size                   # the moments of every tensor are compared whole
            m = rows.size if full else upto
            assert torch.equal(_bits(x[:m]), _bits(y[:m])), (a, k)
            want = b[idx]
            if k > 0:
                want[int(n_keep):] = 0.0                        # clones and children start from zero moments
            assert torch.equal(_bits(x[:m]), _bits(want[:m])), (a, k)
    # the children: N blocks of the split rows; their scale against the fp64 value, held to the torch route's own error
    parents = np.nonzero(split)[0]
    want_ls = np.log(np.exp(np.tile(case['log_scale'][parents], (N, 1)).astype(np.float64)) / (0.8 * N))
    bound, ref_err = dc.split_bound(to_np(got2['_scaling'][0][n_old:]), want_ls, REF_ERR_FACTOR)
    err = float(np.abs(to_np(got1['_scaling'][0][n_old:]).astype(np.float64) - want_ls).max())
    print(f'[densify] children _scaling: kernel error {err:.3e}, torch route error {ref_err:.3e}, bound {bound:.3e}')
    assert n_split > 0 and err <= bound, (err, ref_err, bound)
    # ... and their position is a draw around the parent: |R^T (x - mu)| / sigma is a standard normal sample on both routes
    mu, sig = before['_xyz'][0][idx[n_old:]], torch.exp(before['_scaling'][0][idx[n_old:]])
    R = densify.quaternion_to_R(before['_rotation'][0][idx[n_old:]])
    for got in (got1, got2):
        zed = torch.bmm(R.transpose(1, 2), (got['_xyz'][0][n_old:] - mu)[..., None]).squeeze(-1) / sig
        assert float(zed.abs().max()) < 6.0 and 0.9 < float(zed.std()) < 1.1
    for stats in (stats1, stats2):
        assert stats.xyz_gradient_accum.shape == stats.denom.shape == (one.P, 1) and stats.max_radii2D.shape == (one.P,)
        assert not bool(stats.xyz_gradient_accum.any()) and not bool(stats.denom.any()) and not bool(stats.max_radii2D.any())


def test_prune_keeps_the_restatements_rows():
    """densify.prune on the same model: parameters, moments and statistics are plain indexing with nonzero(~drop)"""
    from sk_gs_amd import densify
    case = dc.make_case(4101, 'random_0.5', 2)
    model, opt, stats, names = _model_and_optimizer(case)
    model._opacity.data.copy_(_dev(case['opacity']))
    before, radii = _state(model, opt, names), stats.max_radii2D.clone()
    keep = _dev(dc.expected_prune(dc.masks_of(case)[2])[0])
    densify.prune(model, opt, stats, min_opacity=float(dc.MIN_OPACITY), extent=dc.EXTENT, max_screen_size=float(dc.MAX_SCREEN))
    assert model.P == keep.numel() and 0 < model.P < case['P']
    assert np.float32(0.1 * dc.EXTENT) == dc.WORLD_LIMIT
    for a, got in _state(model, opt, names).items():
        for x, b in zip(got, before[a]):
            assert torch.equal(_bits(x), _bits(b[keep])), a
    assert torch.equal(stats.max_radii2D, radii[keep]) and stats.denom.shape == (model.P, 1)


# -------------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize('P,mult', [(1, 3.0), (255, 0.5), (1061, 3.0), (1061, 1.0)])
def test_densify_stats_masked_update(P, mult):
    """skgs_densify_stats with grad_multiplier != 1, radii <= 0 (negative included) and P no multiple of the block: entries with
    radii <= 0 keep their bits in all three arrays, the others follow the float32 restatement in the kernel's order
    (acc + mult * sqrt(gx gx + gy gy), denom + 1, max(max_radii, radii)) to the 1e-6 of test_densify_stats_and_lbs_weights_kernels"""
    from sk_gs_amd import _C
    g = np.random.default_rng(P)
    radii = g.integers(-3, 30, P).astype(np.int32)
    radii[0] = 7
    if P > 2:
        radii[1], radii[P - 1] = -1, 0
    grad = g.standard_normal((P, 3)).astype(np.float32)
    acc, den = g.random((P, 1)).astype(np.float32), g.integers(0, 5, (P, 1)).astype(np.float32)
    mr = (g.random(P) * 40).astype(np.float32)
    a, d, m = _dev(acc), _dev(den), _dev(mr)
    _C.densify_stats(_dev(radii), _dev(grad), a, d, m, grad_multiplier=mult)
    torch.cuda.synchronize()
    on = radii > 0
    f = np.float32
    nrm = np.sqrt(grad[:, 0] * grad[:, 0] + grad[:, 1] * grad[:, 1], dtype=f)
    want_a = np.where(on, acc[:, 0] + (nrm if mult == 1.0 else f(mult) * nrm), acc[:, 0]).astype(f)
    want_d, want_m = np.where(on, den[:, 0] + f(1), den[:, 0]), np.where(on, np.maximum(mr, radii.astype(f)), mr)
    got_a, got_d, got_m = to_np(a)[:, 0], to_np(d)[:, 0], to_np(m)
    for got, old in ((got_a, acc[:, 0]), (got_d, den[:, 0]), (got_m, mr)):
        assert np.array_equal(got[~on].view(np.int32), old[~on].view(np.int32))
    assert 0 < on.sum() and (P < 3 or on.sum() < P)
    assert rel_err(got_a, want_a) <= 1e-6 and np.array_equal(got_d, want_d) and np.array_equal(got_m, want_m)
