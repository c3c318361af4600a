"""skgs_point_knn (csrc/point_knn.hip) -- exact K nearest neighbours among 3-D points -- against the chunked torch search of
sk_gs_amd/pytorch3d_ops.py (``_search_torch`` for the indices, a gather of ``_pairwise`` for the squared distances) on the same device:
indices and squared distances BIT-exact, whatever the Z-order, the boxes and the pruning did.  Then the three layers on top: the patched
``update_gs_knn`` (reference_accel.py) on a stand-in model with the reference's attribute names, ``knn_points``' new route, and the
``pykdtree`` stand-in's device route against its CPU route."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ clouds and the reference
def cloud(kind, n, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + n)
    if kind == 'uniform':
        p = torch.rand(n, 3, generator=g)
    elif kind == 'surface':     # thin shells around a few centres: what a trained scene's Gaussians look like
        c = torch.randn(6, 3, generator=g)[torch.randint(0, 6, (n,), generator=g)]
        d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
        p = c + d * (0.3 + 0.002 * torch.randn(n, 1, generator=g))
    elif kind == 'duplicates':  # 10 % exact copies of other rows (clones are exact duplicates of their parents)
        p = torch.rand(n, 3, generator=g)
        rows = torch.randperm(n, generator=g)[:max(n // 10, 1)]
        p[rows] = p[torch.randint(0, n, (rows.numel(),), generator=g)]
    elif kind == 'equal':
        p = torch.full((n, 3), 0.37)
    elif kind == 'line':
        p = torch.zeros(n, 3)
        p[:, 1] = torch.rand(n, generator=g)
        p[:, 2] = 2.0
    elif kind == 'plane':
        p = torch.rand(n, 3, generator=g)
        p[:, 0] = -1.5
    else:
        raise ValueError(kind)
    return (p * scale).float().contiguous().to(DEV)


def reference(q, data, K):
    """(idx [m,K] int64, dist2 [m,K]) by ``_search_torch`` + a gather of ``_pairwise``; columns beyond n_data: -1 / inf"""
    from sk_gs_amd.pytorch3d_ops import _pairwise, _search_torch
    n, m, k = data.shape[0], q.shape[0], min(K, data.shape[0])
    idx = torch.full((m, K), -1, dtype=torch.int64, device=q.device)
    d2 = torch.full((m, K), float('inf'), dtype=torch.float32, device=q.device)
    if m and k:
        found = _search_torch(q, data, K, 2)[:, :k]
        idx[:, :k] = found
        chunk = max(1, (1 << 24) // n)
        for a in range(0, m, chunk):
            d2[a:a + chunk, :k] = _pairwise(q[a:a + chunk], data, 2).gather(1, found[a:a + chunk])
    return idx, d2


def check(data, q, K):
    from sk_gs_amd import _C
    idx, d2, d1 = _C.point_knn(data, q, K=K, want='both')
    want_i, want_d = reference(data if q is None else q, data, K)
    bad = int((idx != want_i).sum())
    print(f'n_data {data.shape[0]} n_query {idx.shape[0]} K {K}: index mismatches {bad}, '
          f'distance bit mismatches {int((d2.view(torch.int32) != want_d.view(torch.int32)).sum())}')
    assert idx.dtype == torch.int64 and idx.shape == want_i.shape and bad == 0
    assert torch.equal(d2.view(torch.int32), want_d.view(torch.int32))
    assert torch.equal(d1.view(torch.int32), torch.sqrt(d2).view(torch.int32))
    return idx, d2, d1


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize('kind', ['uniform', 'surface', 'duplicates'])
def test_self_query_20k_is_bit_exact(kind):
    data = cloud(kind, 20_000)
    idx, d2, _ = check(data, None, 21)
    assert bool((d2[:, 0] == 0).all())                      # a point is its own neighbour ...
    assert bool((idx == torch.arange(20_000, device=DEV)[:, None]).any(dim=1).all())   # ... somewhere in its row


def test_queries_that_are_not_the_data():
    data = cloud('surface', 7000, seed=1)
    q = cloud('uniform', 3001, seed=2) * 2.0 - 1.0           # partly outside the data's box
    check(data, q, 21)
    check(cloud('uniform', 900, seed=3), cloud('uniform', 5000, seed=4), 8)


@pytest.mark.parametrize('K', [1, 3, 16, 21, 32])
def test_every_list_size(K):
    check(cloud('uniform', 6000, seed=K), None, K)


@pytest.mark.parametrize('P', [1, 63, 257, 1025])
def test_partial_blocks(P):
    data = cloud('uniform', P, seed=5)
    for K in (1, 21):
        check(data, None, K)
    check(data, cloud('uniform', 130, seed=6), 5)


def test_more_columns_than_points():
    data = cloud('uniform', 5, seed=7)
    idx, d2, d1 = check(data, None, 21)
    assert bool((idx[:, 5:] == -1).all()) and bool(torch.isinf(d2[:, 5:]).all()) and bool(torch.isinf(d1[:, 5:]).all())
    assert bool((idx[:, :5] >= 0).all())


@pytest.mark.parametrize('kind', ['equal', 'line', 'plane'])
def test_degenerate_clouds(kind):
    check(cloud(kind, 3000, seed=8), None, 21)


@pytest.mark.parametrize('scale', [1e-3, 1e3])
def test_coordinate_scale(scale):
    check(cloud('surface', 6000, seed=9, scale=scale), None, 21)


def _abi():
    from sk_gs_amd import _C
    lib = _C.load_library()
    lib.skgs_point_knn_workspace_bytes.restype = C.c_size_t
    return _C, lib


def _call(lib, _C, data, K, idx, d2, d1, ws, ws_bytes, q=None):
    p = lambda t: C.c_void_p(None if t is None else t.data_ptr())  # noqa: E731
    m = data.shape[0] if q is None else q.shape[0]
    return lib.skgs_point_knn(C.c_int32(data.shape[0]), p(data), C.c_int32(m), p(q), C.c_int32(K), p(idx), p(d2), p(d1), p(ws),
                              C.c_size_t(ws_bytes), _C._stream())


def test_either_output_may_be_null_and_calls_repeat_bit_for_bit():
    _C, lib = _abi()
    n, K = 5000, 21
    data = cloud('duplicates', n, seed=10)
    nbytes = int(lib.skgs_point_knn_workspace_bytes(C.c_int32(n), C.c_int32(n)))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    want_i, want_d = reference(data, data, K)
    runs = []
    for has_d2, has_d1 in ((True, True), (True, False), (False, True), (False, False), (True, True)):
        idx = torch.full((n, K), -7, dtype=torch.int64, device=DEV)
        d2 = torch.full((n, K), -7.0, device=DEV) if has_d2 else None
        d1 = torch.full((n, K), -7.0, device=DEV) if has_d1 else None
        ws.random_(0, 255)                                   # the scratch carries nothing from call to call
        assert _call(lib, _C, data, K, idx, d2, d1, ws, nbytes) == 0
        assert torch.equal(idx, want_i)
        if has_d2:
            assert torch.equal(d2.view(torch.int32), want_d.view(torch.int32))
        if has_d1:
            assert torch.equal(d1.view(torch.int32), torch.sqrt(want_d).view(torch.int32))
        runs.append((idx, d2, d1))
    assert torch.equal(runs[0][0], runs[-1][0]) and torch.equal(runs[0][1].view(torch.int32), runs[-1][1].view(torch.int32))
    assert torch.equal(runs[0][2].view(torch.int32), runs[-1][2].view(torch.int32))


def test_bad_arguments_are_refused_with_an_error_code():
    _C, lib = _abi()
    n = 2000
    data = cloud('uniform', n, seed=11)
    nbytes = int(lib.skgs_point_knn_workspace_bytes(C.c_int32(n), C.c_int32(n)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    idx = torch.full((n, 33), -7, dtype=torch.int64, device=DEV)
    d2 = torch.empty((n, 33), device=DEV)
    lib.skgs_last_error.restype = C.c_char_p
    assert _call(lib, _C, data, 33, idx, d2, None, ws, nbytes) != 0 and b'K' in lib.skgs_last_error()
    assert _call(lib, _C, data, 0, idx, d2, None, ws, nbytes) != 0
    assert _call(lib, _C, data, 21, idx, d2, None, ws, nbytes - 1) != 0 and b'workspace' in lib.skgs_last_error()
    assert _call(lib, _C, data, 21, idx, d2, None, None, 0) != 0
    assert _call(lib, _C, data, 21, None, d2, None, ws, nbytes) != 0
    torch.cuda.synchronize()
    assert bool((idx == -7).all())                           # nothing ran
    # an empty cloud or an empty query set: nothing to do, no error
    empty = torch.empty((0, 3), device=DEV)
    assert _call(lib, _C, empty, 21, idx, d2, None, None, 0) == 0
    assert _call(lib, _C, data, 21, idx, d2, None, None, 0, q=empty) == 0
    torch.cuda.synchronize()
    assert bool((idx == -7).all())
    with pytest.raises(_C.SkgsError):
        _C.point_knn(data, None, K=33)


_BIG = r"""
import sys
sys.path.insert(0, {root!r})
import torch
sys.path.insert(0, {tests!r})
import test_gpu_point_knn as t
from sk_gs_amd import _C
P, K = 500_000, 21
data = t.cloud('surface', P, seed=12)
idx, d2 = _C.point_knn(data, None, K=K)
torch.cuda.synchronize()
rows = torch.randperm(P, generator=torch.Generator().manual_seed(0))[:2000].to(t.DEV)
want_i, want_d = t.reference(data[rows].contiguous(), data, K)
assert torch.equal(idx[rows], want_i), int((idx[rows] != want_i).sum())
assert torch.equal(d2[rows].view(torch.int32), want_d.view(torch.int32))
print('big ok')
"""


def test_half_a_million_points():
    """BASELINE config #4's size, in a child process under its own time limit; 2 000 sampled rows against the brute force"""
    r = subprocess.run([sys.executable, '-c', _BIG.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))], capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0 and 'big ok' in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


# ------------------------------------------------------------------------------------------------ update_gs_knn
class TableModel:
    """what ``update_gs_knn`` / ``loss_weight_smooth`` read and write on the reference's model (networks/sk_gs.py:433-437, 1342-1359, 1518)"""

    def __init__(self, points, gs_knn_num=20, interval=(1000, 3000)):
        from sk_gs_amd import reference_accel as ra
        self.points = points
        self.gs_knn_num, self.gs_knn_update_interval = gs_knn_num, interval
        self.gs_knn_index = torch.empty(0, gs_knn_num, dtype=torch.long, device=points.device)
        self.gs_knn_dist = torch.empty(0, gs_knn_num, dtype=torch.float, device=points.device)
        self._is_gs_knn_updated, self._step = False, 1
        self._ra = ra

    def update_gs_knn(self, force=False):
        return self._ra.update_gs_knn(self, force)


def test_patched_update_gs_knn_builds_the_table_without_a_host_sync():
    from sk_gs_amd import reference_accel as ra
    P = 12_000
    m = TableModel(cloud('surface', P, seed=13))
    m.update_gs_knn()                                        # (the first call sizes the cached scratch)
    first = m.gs_knn_index
    m._is_gs_knn_updated = False
    before = ra.calls['gs_knn_fused']
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        m.update_gs_knn(force=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert ra.calls['gs_knn_fused'] == before + 1
    want_i, want_d = reference(m.points, m.points, 21)
    assert m.gs_knn_index.dtype == torch.int64 and m.gs_knn_index.shape == (P, 21) and m.gs_knn_index.is_contiguous()
    assert m.gs_knn_dist.dtype == torch.float32 and m.gs_knn_dist.shape == (P, 21)
    assert torch.equal(m.gs_knn_index, want_i) and torch.equal(m.gs_knn_index, first)
    assert torch.equal(m.gs_knn_dist.view(torch.int32), torch.sqrt(want_d).view(torch.int32))     # Euclidean, as pykdtree's

    # the table feeds loss_weight_smooth's fast path: the torch expression's value
    w = torch.softmax(torch.randn(P, 5, generator=torch.Generator().manual_seed(1)), -1).to(DEV).requires_grad_()
    m._is_gs_knn_updated = False
    fused0 = ra.calls['weight_reg_fused']
    got = ra.loss_weight_smooth(m, w)
    want = (w[:, None] - w[m.gs_knn_index]).abs().mean()
    assert ra.calls['weight_reg_fused'] == fused0 + 1
    print('loss_weight_smooth', float(got.detach()), float(want.detach()))
    assert abs(float(got.detach()) - float(want.detach())) <= 2e-6 * abs(float(want.detach())) + 1e-9     # (the bound of the kernel's own test: another sum order)
    assert ra.calls['gs_knn_fused'] == before + 1 and m.gs_knn_index.shape == (P, 21)   # nothing was due: no rebuild


def test_patched_update_gs_knn_gating():
    from sk_gs_amd import reference_accel as ra
    m = TableModel(cloud('uniform', 3000, seed=14))
    n0 = ra.calls['gs_knn_fused']
    m.update_gs_knn()                                        # the row count differs from the empty table: built
    assert ra.calls['gs_knn_fused'] == n0 + 1 and m.gs_knn_index.shape == (3000, 21) and m._is_gs_knn_updated
    table = m.gs_knn_index
    m.update_gs_knn(force=True)                              # the flag: at most once per step, even when forced
    assert ra.calls['gs_knn_fused'] == n0 + 1 and m.gs_knn_index is table
    m._is_gs_knn_updated = False                             # (what the reference's step does, sk_gs.py:1518)
    m.update_gs_knn()                                        # nothing is due at step 1
    assert ra.calls['gs_knn_fused'] == n0 + 1 and m.gs_knn_index is table and m._is_gs_knn_updated
    m._is_gs_knn_updated, m._step = False, 2000              # the interval (every 1000 steps up to 3000)
    m.update_gs_knn()
    assert ra.calls['gs_knn_fused'] == n0 + 2 and m.gs_knn_index is not table
    table = m.gs_knn_index
    m._is_gs_knn_updated, m._step = False, 4000              # ... and not beyond its end
    m.update_gs_knn()
    assert ra.calls['gs_knn_fused'] == n0 + 2 and m.gs_knn_index is table
    m._is_gs_knn_updated = False                             # a densify / prune event changed the number of Gaussians
    m.points = cloud('uniform', 3500, seed=15)
    m.update_gs_knn()
    assert ra.calls['gs_knn_fused'] == n0 + 3 and m.gs_knn_index.shape == (3500, 21)
    want_i, _ = reference(m.points, m.points, 21)
    assert torch.equal(m.gs_knn_index, want_i)
    m._is_gs_knn_updated = False
    m.update_gs_knn(force=True)
    assert ra.calls['gs_knn_fused'] == n0 + 4


# ------------------------------------------------------------------------------------------------ knn_points
@pytest.mark.parametrize('K', [21, 8])
def test_knn_points_takes_the_new_route(K):
    from sk_gs_amd import pytorch3d_ops as p3d
    g = torch.Generator().manual_seed(K)
    p1, p2 = torch.rand(3000, 3, generator=g), torch.rand(5000, 3, generator=g)
    c = torch.randn(3000, K, generator=g).to(DEV)
    a, b = p1.to(DEV).requires_grad_(), p2.to(DEV).requires_grad_()
    before = dict(p3d.hip_calls)
    r = p3d.knn_points(a[None], b[None], K=K)
    assert p3d.hip_calls['point_knn'] == before['point_knn'] + 1
    assert p3d.hip_calls['knn_bones'] == before['knn_bones'] and p3d.hip_calls['sp_search'] == before['sp_search']
    (r.dists[0] * c).sum().backward()
    # the torch path on the same device (explicit lengths keep a call off the kernels)
    a0, b0 = p1.to(DEV).requires_grad_(), p2.to(DEV).requires_grad_()
    full1, full2 = torch.tensor([3000], device=DEV), torch.tensor([5000], device=DEV)
    r0 = p3d.knn_points(a0[None], b0[None], full1, full2, K=K)
    assert p3d.hip_calls['point_knn'] == before['point_knn'] + 1
    (r0.dists[0] * c).sum().backward()
    assert r.idx.dtype == torch.int64 and r.idx.shape == (1, 3000, K) and r.knn is None
    assert torch.equal(torch.as_tensor(r.idx).as_subclass(torch.Tensor), r0.idx)
    print('knn_points dists: max |difference| to the torch path', float((r.dists - r0.dists).abs().max()))
    want_i, want_d = reference(a.detach(), b.detach(), K)
    assert torch.equal(r.dists[0].detach().view(torch.int32), want_d.view(torch.int32))
    # the torch path forms the same three squares and adds them with torch's reduction, whose order is not `_pairwise`'s left to right:
    # two rounded additions of non-negative terms on either side, each within 2^-24 of its partial sum <= d, so the two results
    # are within 4 * 2^-24 * d of each other (observed: one unit in the last place on a few entries); the kernel's own bits are held
    # by the line above, against the order the C ABI states
    assert bool(((r.dists - r0.dists).abs() <= 4 * 2.0 ** -24 * r0.dists).all())
    for got, want in ((a.grad, a0.grad), (b.grad, b0.grad)):
        err = float((got - want).abs().max()) / float(want.abs().max())
        print('knn_points gradient error / max', err)
        assert err <= 1e-5


def test_knn_points_small_tables_keep_their_kernels():
    from sk_gs_amd import pytorch3d_ops as p3d
    g = torch.Generator().manual_seed(3)
    a, b = torch.rand(3000, 3, generator=g).to(DEV), torch.rand(512, 3, generator=g).to(DEV)
    before = dict(p3d.hip_calls)
    p3d.knn_points(a[None], b[None], K=5)
    assert p3d.hip_calls['sp_search'] == before['sp_search'] + 1 and p3d.hip_calls['point_knn'] == before['point_knn']


# ------------------------------------------------------------------------------------------------ the pykdtree stand-in
def test_pykdtree_stand_in_device_route_equals_its_cpu_route(monkeypatch):
    from sk_gs_amd import pykdtree as kd
    pts = cloud('duplicates', 4000, seed=16).cpu().numpy()
    q = cloud('uniform', 1500, seed=17).cpu().numpy()
    tree = kd.KDTree(pts)
    before = dict(kd.calls)
    on_dev = [tree.query(pts, k=21), tree.query(q, k=3), tree.query(q, k=1, sqr_dists=True)]
    assert kd.calls['hip'] == before['hip'] + 3 and kd.calls['cpu'] == before['cpu']
    monkeypatch.setenv('SKGS_PYKDTREE_DEVICE', '0')
    on_cpu = [tree.query(pts, k=21), tree.query(q, k=3), tree.query(q, k=1, sqr_dists=True)]
    assert kd.calls['cpu'] == before['cpu'] + 3
    for (d_a, i_a), (d_b, i_b) in zip(on_dev, on_cpu):
        assert d_a.dtype == np.float32 and i_a.dtype == np.uint32 and d_a.shape == d_b.shape and i_a.shape == i_b.shape
        assert np.array_equal(i_a, i_b) and np.array_equal(d_a.view(np.uint32), d_b.view(np.uint32))


def test_pykdtree_stand_in_overlapping_views_are_not_a_self_query(monkeypatch):
    """two contiguous views of one array with equal shapes that share memory but not their rows: a real query, not the data's own"""
    from sk_gs_amd import pykdtree as kd
    base = cloud('uniform', 3001, seed=18).cpu().numpy()
    data, q = base[:-1], base[1:]
    assert data.shape == q.shape and np.shares_memory(data, q) and data.flags.c_contiguous and q.flags.c_contiguous
    tree = kd.KDTree(data)
    assert tree.data_pts.ctypes.data == data.ctypes.data          # (no copy was made: the views still overlap inside the tree)
    d_a, i_a = tree.query(q, k=4)
    monkeypatch.setenv('SKGS_PYKDTREE_DEVICE', '0')
    d_b, i_b = tree.query(q, k=4)
    assert np.array_equal(i_a, i_b) and np.array_equal(d_a.view(np.uint32), d_b.view(np.uint32))
    assert np.array_equal(i_a[:-1, 0], np.arange(1, 3000))        # row r of q is row r + 1 of the data
