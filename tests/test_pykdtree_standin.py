"""The ``pykdtree`` stand-in (sk_gs_amd/pykdtree.py) without a GPU: ``install_reference_hooks()`` plants it, ``KDTree.query`` follows
pykdtree's contract for what the reference uses, and its chunked CPU search agrees with a float64 brute force and (where scipy is
installed) with ``scipy.spatial.cKDTree``.  Then the reference's UNMODIFIED ``update_gs_knn`` (networks/sk_gs.py:1342-1355) on it and the
patched one's fall-through on CPU tensors, in a child process as tests/test_host_cpu.py does; skipped where the reference checkout is
absent.

Comparisons are tie-tolerant (duplicate points make equal distances, whose order is this package's rule, not pykdtree's): the sorted
distances agree to 1e-6 relative (fp32 rounding of a three-term sum of squares), every returned index reproduces its returned distance,
no index repeats in a row, and no unlisted point is closer than the last column."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REFERENCE = '/root/reference'
sys.path.insert(0, ROOT)


def _child(script, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, env=e, timeout=600)


# ------------------------------------------------------------------------------------------------ the hook
_HOOK = r"""
import sys
sys.dont_write_bytecode = True
sys.path.insert(0, {root!r})
import sk_gs_amd
hooked = sk_gs_amd.install_reference_hooks()
from pykdtree.kdtree import KDTree
import pykdtree, pykdtree.kdtree, sk_gs_amd.pykdtree as kd
assert KDTree is kd.KDTree and pykdtree.kdtree is kd and sys.modules['pykdtree.kdtree'] is kd and 'pykdtree.kdtree' in hooked
import numpy as np
d, i = KDTree(np.eye(3, dtype=np.float32)).query(np.eye(3, dtype=np.float32), k=2)
assert i.dtype == np.uint32 and i[:, 0].tolist() == [0, 1, 2] and np.allclose(d[:, 1], 2 ** 0.5)
assert sk_gs_amd.install_as_pykdtree() is kd            # idempotent
print('HOOK-OK')
"""

_HOOK_OFF = r"""
import sys
sys.dont_write_bytecode = True
sys.path.insert(0, {root!r})
import sk_gs_amd
hooked = sk_gs_amd.install_reference_hooks()
assert 'pykdtree' not in sys.modules and 'pykdtree.kdtree' not in sys.modules and 'pykdtree.kdtree' not in hooked, hooked
assert sk_gs_amd.install_as_pykdtree() is None
assert 'pytorch3d.ops' in sys.modules                   # the other stand-ins are untouched by the switch
print('OFF-OK')
"""


def test_install_reference_hooks_plants_the_stand_in():
    r = _child(_HOOK.format(root=ROOT))
    assert r.returncode == 0 and 'HOOK-OK' in r.stdout, r.stderr[-2000:]


def test_switch_leaves_sys_modules_alone():
    r = _child(_HOOK_OFF.format(root=ROOT), env={'SKGS_PYKDTREE': '0'})
    assert r.returncode == 0 and 'OFF-OK' in r.stdout, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ query against a brute force
def _cloud(kind, n, seed):
    rng = np.random.default_rng(seed * 7919 + n)
    if kind == 'uniform':
        p = rng.random((n, 3))
    elif kind == 'clustered':
        c = rng.normal(size=(5, 3))[rng.integers(0, 5, n)]
        p = c + 0.01 * rng.normal(size=(n, 3))
    elif kind == 'duplicates':
        p = rng.random((n, 3))
        rows = rng.permutation(n)[:max(n // 10, 1)] if n > 1 else np.zeros(0, np.int64)
        p[rows] = p[rng.integers(0, n, rows.size)]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p.astype(np.float32))


def _check_against_brute_force(data, q, k, dist, idx, want_sorted=None):
    """the tie-tolerant comparison of the module docstring; ``dist`` Euclidean [m,k], ``idx`` [m,k]"""
    n, m = data.shape[0], q.shape[0]
    kk = min(k, n)
    assert dist.shape == (m, k) and idx.shape == (m, k)
    assert np.all(idx[:, kk:] == n) and np.all(np.isinf(dist[:, kk:]))            # missing neighbours
    d64 = np.sqrt(((q[:, None, :].astype(np.float64) - data[None, :, :].astype(np.float64)) ** 2).sum(-1))   # [m,n]
    want = np.sort(d64, axis=1)[:, :kk] if want_sorted is None else want_sorted[:, :kk]
    got, ids = dist[:, :kk].astype(np.float64), idx[:, :kk].astype(np.int64)
    assert np.all(np.diff(got, axis=1) >= 0)                                       # ascending
    scale = np.maximum(want, 1e-30)
    # (exact duplicates give 0 = 0)
    assert np.all(np.abs(got - want) <= 1e-6 * scale), float(np.max(np.abs(got - want) / scale))
    assert np.all((ids >= 0) & (ids < n))
    assert np.all(np.abs(np.take_along_axis(d64, ids, axis=1) - got) <= 1e-6 * np.maximum(got, 1e-30))   # an index reproduces its distance
    srt = np.sort(ids, axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1])                                       # no index twice in a row
    if kk < n:                                                                     # no unlisted point is closer than the last column
        rest = d64.copy()
        np.put_along_axis(rest, ids, np.inf, axis=1)
        assert np.all(rest.min(axis=1) >= got[:, -1] * (1 - 1e-6))


@pytest.mark.parametrize('kind', ['uniform', 'clustered', 'duplicates'])
@pytest.mark.parametrize('n', [1, 5, 1000, 5000])
def test_query_against_a_float64_brute_force(kind, n):
    from sk_gs_amd.pykdtree import KDTree
    data = _cloud(kind, n, 1)
    tree = KDTree(data)
    m = min(n, 1500)                                  # (the float64 matrix of the check is m x n)
    for k in (1, 3, 21, 32):
        dist, idx = tree.query(data[:m], k=k)
        if k == 1:
            assert dist.shape == (m,) and idx.shape == (m,)
            dist, idx = dist[:, None], idx[:, None]
        _check_against_brute_force(data, data[:m], k, dist, idx)
        if n > 1 and kind != 'duplicates':
            assert np.all(dist[:, 0] == 0) and np.array_equal(idx[:, 0], np.arange(m))    # a point is its own nearest neighbour


@pytest.mark.parametrize('k', [1, 3, 21, 32])
def test_query_set_that_is_not_the_data(k):
    from sk_gs_amd.pykdtree import KDTree
    data, q = _cloud('clustered', 3000, 2), _cloud('uniform', 700, 3) * 2 - 0.5
    dist, idx = KDTree(data).query(q, k=k)
    if k == 1:
        dist, idx = dist[:, None], idx[:, None]
    _check_against_brute_force(data, q, k, dist, idx)


@pytest.mark.parametrize('kind', ['uniform', 'duplicates'])
def test_query_against_scipy(kind):
    spatial = pytest.importorskip('scipy.spatial')
    from sk_gs_amd.pykdtree import KDTree
    data, q = _cloud(kind, 4000, 4), _cloud('uniform', 800, 5)
    for k in (1, 21):
        want, _ = spatial.cKDTree(data.astype(np.float64)).query(q.astype(np.float64), k=k)
        dist, idx = KDTree(data).query(q, k=k)
        if k == 1:
            dist, idx, want = dist[:, None], idx[:, None], want[:, None]
        _check_against_brute_force(data, q, k, dist, idx, want_sorted=want)


def test_output_contract():
    from sk_gs_amd.pykdtree import KDTree
    data = _cloud('uniform', 50, 6)
    tree = KDTree(data, leafsize=10)
    assert tree.n == 50 and tree.ndim == 3 and tree.data_pts.dtype == np.float32
    d, i = tree.query(data, k=1)
    assert d.dtype == np.float32 and i.dtype == np.uint32 and d.shape == (50,) and i.shape == (50,)
    d, i = tree.query(data, k=4)
    assert d.dtype == np.float32 and i.dtype == np.uint32 and d.shape == (50, 4) and i.shape == (50, 4)
    d2, i2 = tree.query(data, k=4, sqr_dists=True)
    assert np.array_equal(i, i2) and np.array_equal(d, np.sqrt(d2)) and d2.dtype == np.float32
    # fewer points than columns: idx = n, dist = inf
    d, i = tree.query(data[:7], k=60)
    assert d.shape == (7, 60) and np.all(i[:, 50:] == 50) and np.all(np.isinf(d[:, 50:])) and np.all(i[:, :50] < 50)
    assert np.all(np.isfinite(d[:, :50]))
    # float64 data: float64 distances; other widths run too (the CPU route)
    d, i = KDTree(data.astype(np.float64)).query(data.astype(np.float64), k=3)
    assert d.dtype == np.float64 and i.dtype == np.uint32 and np.array_equal(i[:, 0], np.arange(50))
    d, i = KDTree(data[:, :2]).query(data[:5, :2], k=2)
    assert d.shape == (5, 2) and np.array_equal(i[:, 0], np.arange(5))
    # ties keep the lower index first (this package's rule)
    twin = np.zeros((4, 3), np.float32)
    d, i = KDTree(twin).query(twin, k=4)
    assert np.array_equal(i, np.tile(np.arange(4, dtype=np.uint32), (4, 1))) and np.all(d == 0)
    # what is not implemented says so; a mismatch of types or widths is refused as pykdtree refuses it
    for kw in (dict(eps=0.1), dict(distance_upper_bound=1.0), dict(mask=np.zeros(50, bool))):
        with pytest.raises(NotImplementedError, match='not implemented'):
            tree.query(data, k=2, **kw)
    with pytest.raises(TypeError):
        tree.query(data.astype(np.float64), k=2)
    with pytest.raises(ValueError):
        tree.query(data[:, :2], k=2)
    with pytest.raises(ValueError):
        tree.query(data, k=0)


# ------------------------------------------------------------------------------------------------ the reference's own method on it
_REF_SCRIPT = r"""
import sys, warnings
sys.dont_write_bytecode = True
sys.path[:0] = [{root!r}, {golden!r}, {ref!r}, {tests!r}]
import make_golden
make_golden.STUBS = make_golden.STUBS - {{'lietorch', 'pytorch3d', 'diff_gaussian_rasterization', 'pykdtree'}}
sys.meta_path.insert(0, make_golden._Finder())
import sk_gs_amd
sk_gs_amd.install_reference_hooks()
warnings.simplefilter('ignore')
import numpy as np, yaml, torch
from torch import nn
import networks.sk_gs as sk
from sk_gs_amd import reference_accel as ra, pykdtree as kd
import test_pykdtree_standin as T
S = sk.SkeletonGaussianSplatting
m = S(**yaml.safe_load(open({ref!r} + '/exps/default.yaml'))['arch_cfg'])
P = 3000
pts = torch.from_numpy(T._cloud('clustered', P, 9))
m._xyz = nn.Parameter(pts.clone())
assert m.gs_knn_num == 20 and m.gs_knn_index.shape[0] == 0 and tuple(m.gs_knn_update_interval) == (1000, 3000)

# (1) the UNMODIFIED method runs through the stand-in
orig = S.update_gs_knn
n0 = kd.calls['cpu']
m.update_gs_knn(force=True)
assert kd.calls['cpu'] == n0 + 1
assert m.gs_knn_index.dtype == torch.int64 and tuple(m.gs_knn_index.shape) == (P, 21)
assert m.gs_knn_dist.dtype == torch.float32 and tuple(m.gs_knn_dist.shape) == (P, 21)
T._check_against_brute_force(pts.numpy(), pts.numpy()[:1200], 21, m.gs_knn_dist.numpy()[:1200], m.gs_knn_index.numpy()[:1200])
table = m.gs_knn_index

# (2) the patched method on CPU tensors is the reference's own, with its gating: the flag, force, the row count, the interval
sk_gs_amd.accelerate_reference(adam=False)
assert S.update_gs_knn is ra.update_gs_knn and ra._table_originals['gs_knn'] is orig
r0 = ra.calls['gs_knn_reference']
m.update_gs_knn(force=True)                                    # the flag is still set: once per step
assert kd.calls['cpu'] == n0 + 1 and m.gs_knn_index is table and ra.calls['gs_knn_reference'] == r0 + 1
m._is_gs_knn_updated, m._step = False, 1
m.update_gs_knn()                                              # nothing due
assert kd.calls['cpu'] == n0 + 1 and m.gs_knn_index is table and m._is_gs_knn_updated
m._is_gs_knn_updated = False
m.update_gs_knn(force=True)
assert kd.calls['cpu'] == n0 + 2 and m.gs_knn_index is not table and torch.equal(m.gs_knn_index, table)
m._is_gs_knn_updated, m._step = False, 2000                    # the interval
m.update_gs_knn()
assert kd.calls['cpu'] == n0 + 3
m._is_gs_knn_updated, m._step = False, 4000                    # ... and past its end
m.update_gs_knn()
assert kd.calls['cpu'] == n0 + 3
m._is_gs_knn_updated = False                                   # the row count
m._xyz = nn.Parameter(pts[:2500].clone())
m.update_gs_knn()
assert kd.calls['cpu'] == n0 + 4 and tuple(m.gs_knn_index.shape) == (2500, 21)
assert ra.calls['gs_knn_fused'] == 0
# the restated interval rule against the reference's
from my_ext import utils
for step in (0, 1, 999, 1000, 1500, 2000, 3000, 3001, 4000):
    for iv in ((1000, 3000), (1000,), (500, 1000, 2000), (0, 10), (7, 21)):
        assert ra._interval_due(step, *iv) == utils.check_interval(step, *iv, force_end=False), (step, iv)
# the patched loss_weight_smooth keeps calling it
w = torch.softmax(torch.randn(2500, 5), -1)
m._is_gs_knn_updated = False
assert torch.equal(m.loss_weight_smooth(w), (w[:, None] - w[m.gs_knn_index]).abs().mean()) and m._is_gs_knn_updated

# (3) restore_reference() undoes the patch
ra.restore_reference()
assert S.update_gs_knn is orig and 'gs_knn' not in ra._table_originals
print('REF-OK')
"""


@pytest.mark.skipif(not os.path.isdir(_REFERENCE), reason='the reference checkout is not on this machine')
def test_reference_update_gs_knn_runs_on_the_stand_in():
    r = _child(_REF_SCRIPT.format(root=ROOT, golden=os.path.join(ROOT, 'tests', 'golden'), ref=_REFERENCE, tests=os.path.join(ROOT, 'tests')))
    assert r.returncode == 0 and 'REF-OK' in r.stdout, r.stderr[-3000:]
