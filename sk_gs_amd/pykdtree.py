"""Stand-in for ``pykdtree`` (storpipfugl/pykdtree, un-pinned in the reference's requirements) -- what the reference imports from it,
so that the UNMODIFIED ``networks/sk_gs.py`` runs on a machine without that package::

    import sk_gs_amd
    sk_gs_amd.install_as_pykdtree()          # sys.modules['pykdtree'], ['pykdtree.kdtree'];  `from pykdtree.kdtree import KDTree`

Call site: ``update_gs_knn`` (networks/sk_gs.py:1349-1352): ``KDTree(points).query(points, k=gs_knn_num + 1)`` over all Gaussians -- the
21-column neighbour table ``loss_weight_smooth`` reads in every ``sp`` iteration, rebuilt whenever the number of Gaussians changed.

Semantics restated from pykdtree's published interface: ``KDTree(data_pts [n,d], leafsize=16)``;
``query(query_pts [m,d], k=1, eps=0, distance_upper_bound=None, sqr_dists=False, mask=None) -> (dist, idx)`` with ``dist`` in the
data's dtype (Euclidean, squared with ``sqr_dists``), ``idx`` uint32, both ``[m]`` for k = 1 and ``[m,k]`` otherwise, ascending; a row with
fewer than k neighbours is padded with ``idx = n``, ``dist = inf``.  The search here is EXACT (``eps = 0``); approximate search, a
distance bound and a mask are not implemented and raise.  Equal distances keep the lower index first (this package's rule).

3-column float32 data on a machine with a HIP device is one upload, ONE ``skgs_point_knn`` call (csrc/point_knn.hip) and one
download; everything else -- other widths, float64, a machine without a GPU -- is a chunked brute force on the CPU with the same
arithmetic (per-coordinate squares summed left to right in the data's dtype) and the same tie order, so both routes return the same
table.  ``SKGS_PYKDTREE_DEVICE=0`` keeps the CPU route.
"""
from __future__ import annotations

import os

import numpy as np

__all__ = ['KDTree']

calls = {'hip': 0, 'cpu': 0}  # counters (tests)


def _hip_device():
    if os.environ.get('SKGS_PYKDTREE_DEVICE', '1') == '0':
        return None
    try:
        import torch
        if torch.cuda.is_available() and getattr(torch.version, 'hip', None):
            return torch.device('cuda', torch.cuda.current_device())
    except Exception:  # noqa: BLE001  (no torch, no driver: the CPU route)
        pass
    return None


def _brute_force(data: np.ndarray, queries: np.ndarray, k: int):
    """(dist2 [m,k], idx [m,k] int64) of the k nearest rows of ``data``: squared distances accumulated over the coordinates in index
    order in the data's dtype, rows ascending by (distance, index); ``k <= n``"""
    n, m = data.shape[0], queries.shape[0]
    dist2 = np.empty((m, k), dtype=data.dtype)
    idx = np.empty((m, k), dtype=np.int64)
    chunk = max(1, (1 << 22) // max(n, 1))
    col = np.arange(n, dtype=np.uint64)[None, :]
    for a in range(0, m, chunk):
        q = queries[a:a + chunk]
        d = None
        for c in range(data.shape[1]):
            diff = q[:, None, c] - data[None, :, c]
            term = diff * diff
            d = term if d is None else d + term
        if data.dtype == np.float32:
            # the bit pattern of a non-negative float orders like the float: (distance bits, index) in one integer key, all distinct
            key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | col
            if k < n:
                key = np.partition(key, k - 1, axis=1)[:, :k]
            key = np.sort(key, axis=1)
            idx[a:a + chunk] = (key & np.uint64(0xffffffff)).astype(np.int64)
            dist2[a:a + chunk] = (key >> np.uint64(32)).astype(np.uint32).view(np.float32)
        else:
            order = np.argsort(d, axis=1, kind='stable')[:, :k]
            idx[a:a + chunk] = order
            dist2[a:a + chunk] = np.take_along_axis(d, order, axis=1)
    return dist2, idx


class KDTree:
    """``pykdtree.kdtree.KDTree`` as the reference uses it (no tree is built: the device search orders the points itself)."""

    def __init__(self, data_pts, leafsize: int = 16):
        data = np.asarray(data_pts)
        if data.ndim == 1:
            data = data[:, None]
        if data.ndim != 2:
            raise ValueError('data_pts must be a 2-d array [n_points, n_dims]')
        if data.dtype not in (np.float32, np.float64):
            data = data.astype(np.float64)
        if leafsize < 1:
            raise ValueError('leafsize must be greater than zero')
        self.data_pts = np.ascontiguousarray(data)
        self.data = self.data_pts.ravel()
        self.n, self.ndim = self.data_pts.shape
        self.leafsize = int(leafsize)

    def query(self, query_pts, k: int = 1, eps: float = 0, distance_upper_bound=None, sqr_dists: bool = False, mask=None):
        if eps != 0:
            raise NotImplementedError('sk_gs_amd.pykdtree: approximate search (eps != 0) is not implemented; the search is exact')
        if distance_upper_bound is not None:
            raise NotImplementedError('sk_gs_amd.pykdtree: distance_upper_bound is not implemented')
        if mask is not None:
            raise NotImplementedError('sk_gs_amd.pykdtree: mask is not implemented')
        k = int(k)
        if k < 1:
            raise ValueError('Number of neighbours must be greater than zero')
        q = np.asarray(query_pts)
        if q.ndim == 1:
            q = q[:, None]
        if q.ndim != 2 or q.shape[1] != self.ndim:
            raise ValueError('Data and query points must have same dimensions')
        if q.dtype != self.data_pts.dtype:
            raise TypeError('Type mismatch. query points must be of type %s' % self.data_pts.dtype.name)
        q = np.ascontiguousarray(q)
        m, kk = q.shape[0], min(k, self.n)
        dist = np.full((m, k), np.inf, dtype=self.data_pts.dtype)
        idx = np.full((m, k), self.n, dtype=np.uint32)
        if m > 0 and kk > 0:
            dev = _hip_device() if (self.ndim == 3 and self.data_pts.dtype == np.float32 and kk <= 32) else None
            if dev is not None:
                import torch
                from sk_gs_amd import _C
                d_data = torch.from_numpy(self.data_pts).to(dev)
                same = q.shape == self.data_pts.shape and q.strides == self.data_pts.strides and q.ctypes.data == self.data_pts.ctypes.data
                d_q = None if same else torch.from_numpy(q).to(dev)     # (the very same rows: a self query, one upload)
                i_dev, d_dev = _C.point_knn(d_data, d_q, K=kk, want='dist2')
                both = torch.cat([i_dev.to(torch.float64), d_dev.to(torch.float64)], dim=1).cpu().numpy()  # (one download; both exact in fp64)
                idx[:, :kk] = both[:, :kk].astype(np.uint32)
                dist[:, :kk] = both[:, kk:].astype(np.float32)
                calls['hip'] += 1
            else:
                d2, ix = _brute_force(self.data_pts, q, kk)
                idx[:, :kk] = ix.astype(np.uint32)
                dist[:, :kk] = d2
                calls['cpu'] += 1
            if not sqr_dists:
                dist[:, :kk] = np.sqrt(dist[:, :kk])
        if k == 1:
            return dist[:, 0], idx[:, 0]
        return dist, idx
