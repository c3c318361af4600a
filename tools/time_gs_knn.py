#!/usr/bin/env python3
"""Times one rebuild of the Gaussians' neighbour table (networks/sk_gs.py:1342-1355 `update_gs_knn`: P x P, K = gs_knn_num + 1 = 21).

    python tools/time_gs_knn.py [--out FILE] [--iters N] [--sizes 20000,100000,300000,500000]
    python tools/time_gs_knn.py --only 100000 --iters 5          # the call alone, for a kernel trace

For every size, on a uniform and on a clustered (thin shells) cloud:
  new      skgs_point_knn (csrc/point_knn.hip) through sk_gs_amd._C.point_knn, indices + Euclidean distances: HIP events around N calls
           after a warm-up; `sort` (box, Morton codes, radix sort), `build` (Z-ordered copy, one box per 64 points) and `search` from the
           library's own per-phase events (a second set of calls: the events sit between the launches)
  torch    the device alternative before this kernel: knn_points' chunked torch path (`_search_torch`: a [chunk, P] distance matrix and a
           stable sort per chunk), on all rows up to --torch-full-below points, else on --torch-rows rows and scaled to P (marked ~)
  host     the reference's route: positions to the host, KDTree(points).query(points, k=21), table back to the device -- through the real
           pykdtree where it is importable, else "not available"; scipy's cKDTree (16 workers) is timed the same way for scale
  inverse  sk_gs_amd.weight_reg.inverse_lists of the new table (torch argsort + bincount; what loss_weight_smooth's backward walks)
The yardstick: one rebuild per 100 iterations of stage sp (0.824 ms each) should cost at most 5 % of them: 4.1 ms."""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sk_gs_amd import _C, weight_reg  # noqa: E402
from sk_gs_amd.pytorch3d_ops import _search_torch  # noqa: E402

DEV = torch.device('cuda:0')
K = 21
PHASES = ('point_knn_sort', 'point_knn_build', 'point_knn_search')


def cloud(kind, n):
    g = torch.Generator().manual_seed(n)
    if kind == 'uniform':
        p = torch.rand(n, 3, generator=g)
    else:
        c = torch.randn(8, 3, generator=g)[torch.randint(0, 8, (n,), generator=g)]
        d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
        p = c + d * (0.3 + 0.002 * torch.randn(n, 1, generator=g))
    return p.float().contiguous().to(DEV)


def events_ms(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def host_route(tree_cls, pts, **query_kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = pts.detach().cpu().numpy()
    dist, idx = tree_cls(host).query(host, k=K, **query_kw)
    i_dev = torch.from_numpy(idx.astype(np.int32)).to(DEV, torch.int64)
    d_dev = torch.from_numpy(np.asarray(dist, dtype=np.float32)).to(DEV)
    torch.cuda.synchronize()
    del i_dev, d_dev
    return (time.perf_counter() - t0) * 1e3


def optional(module, name):
    try:
        return getattr(importlib.import_module(module), name)
    except Exception:  # noqa: BLE001
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--sizes', default='20000,100000,300000,500000')
    ap.add_argument('--only', type=int, default=0, help='just the new call at this size on the uniform cloud (for a kernel trace)')
    ap.add_argument('--torch-full-below', type=int, default=150_000)
    ap.add_argument('--torch-rows', type=int, default=512)
    ap.add_argument('--host-below', type=int, default=600_000)
    args = ap.parse_args()
    if args.only:
        pts = cloud('uniform', args.only)
        print(f'point_knn P={args.only} K={K}: {events_ms(lambda: _C.point_knn(pts, None, K=K, want="dist"), args.iters):.3f} ms')
        return
    real_kd = None if 'sk_gs_amd' in getattr(sys.modules.get('pykdtree'), '__version__', '') else optional('pykdtree.kdtree', 'KDTree')
    scipy_kd = optional('scipy.spatial', 'cKDTree')
    target = 0.05 * 100 * 0.824
    lines = [f'# one rebuild of the Gaussians\' neighbour table, K = {K}, self query; ms; mean of {args.iters} calls after warm-up (HIP events) -- {torch.cuda.get_device_name(0)}',
             f'# target: 5 % of 100 stage-sp iterations of 0.824 ms = {target:.2f} ms per rebuild',
             '# new = skgs_point_knn (sort / build / search: the library\'s per-phase events, a second set of calls); torch = knn_points\' chunked torch path',
             '# (~: timed on a sample of rows, scaled to P); host = device -> host copy + KD-tree + upload, wall clock; inverse = weight_reg.inverse_lists',
             f'# pykdtree: {"installed" if real_kd else "not available"}; scipy cKDTree (16 workers): {"installed" if scipy_kd else "not available"}',
             f'{"P":>7} {"cloud":>9} {"new":>8} {"sort":>7} {"build":>7} {"search":>8} {"torch":>11} {"pykdtree":>13} {"scipy":>9} {"inverse":>8} {"new/target":>10}']
    for P in [int(s) for s in args.sizes.split(',')]:
        for kind in ('uniform', 'clustered'):
            pts = cloud(kind, P)
            call = lambda: _C.point_knn(pts, None, K=K, want='dist')  # noqa: E731
            t_new = events_ms(call, args.iters)
            _C.profile_enable(list(PHASES))
            _C.profile_collect()
            for _ in range(args.iters):
                call()
            got = _C.profile_collect()
            _C.profile_enable([])
            ph = [got.get(n, (float('nan'), 1))[0] / args.iters for n in PHASES]
            if P < args.torch_full_below:
                t_torch, mark = events_ms(lambda: _search_torch(pts, pts, K, 2), 1, warm=0), ' '
            else:
                rows = pts[:args.torch_rows].contiguous()
                t_torch, mark = events_ms(lambda: _search_torch(rows, pts, K, 2), 1, warm=1) * P / rows.shape[0], '~'
            t_kd = f'{host_route(real_kd, pts):13.1f}' if (real_kd and P < args.host_below) else f'{"not available":>13}'
            t_sp = f'{host_route(scipy_kd, pts, workers=16):9.1f}' if (scipy_kd and P < args.host_below) else f'{"-":>9}'
            idx, _ = call()
            t_inv = events_ms(lambda: weight_reg.inverse_lists(idx.clone()), 3, warm=1)
            lines.append(f'{P:7d} {kind:>9} {t_new:8.3f} {ph[0]:7.3f} {ph[1]:7.3f} {ph[2]:8.3f} {mark}{t_torch:10.1f} {t_kd} {t_sp} {t_inv:8.3f} {t_new / target:9.2f}x')
            print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text)
    print(text)


if __name__ == '__main__':
    main()
