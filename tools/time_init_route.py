"""Stages init_fix / init: one iteration of the reference's loop (render + image terms + backward + the patched Adam.step) on the fused
route against the fallback (the reference's own sequence, restated in torch: init_stage, forward, the operator-path rasterizer, 0.8 L1 +
0.2 SSIM), both in one process, HIP events after warm-up; and the cost of one route rebuild (construction + the two graph captures), which
the densification of these stages triggers every 100 iterations.

    python tools/time_init_route.py [--P 3000 20000 100000] [--iters 50] [--warmup 10]
"""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F
import torch.optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAUSSIANS = ('_xyz', '_features_dc', '_features_rest', '_scaling', '_rotation', '_opacity')


class _InitModel:
    training, use_official_gaussians_render, convert_SHs_python, compute_cov3D, max_sh_degree = True, True, False, False, 3

    def __init__(self, p, net):
        for k in GAUSSIANS:
            setattr(self, k, p[k])
        self.sp_deform_net = net
        self._active_sh_degree = torch.tensor(3, dtype=torch.int, device=p['_xyz'].device)

    def get_now_stage(self, stage=None):
        return 'init' if stage is None else stage


def setup(P, W, H):
    from benchlib import options, reference_loop
    args = options.build_parser().parse_args(['--reference-loop', 'fused', '--config', '9', '--views', '3', '--stage', 'sp',
                                              '--superpoints', '128', '--knn', '4'])
    s = reference_loop.setup(args, {9: dict(name=f'init-{P}', P=P, M=12, K=4, W=W, H=H)})
    s.model = _InitModel(s.p, s.net)

    def outputs(v, stage):
        p = s.p
        d_xyz = s.net.reference_forward(p['_xyz'].detach(), s.times[v])['d_xyz']
        zero = d_xyz.new_tensor(0)
        if stage == 'init_fix':
            d_xyz = d_xyz.detach()
        scales = p['_scaling'].mean(dim=(0, 1), keepdim=True).expand_as(p['_scaling'])
        return dict(points=p['_xyz'] + d_xyz, scales=torch.exp(scales) + zero, rotations=F.normalize(p['_rotation'] + zero),
                    opacity=torch.sigmoid(p['_opacity']))
    s.outputs = outputs
    return s


def iteration(s, i, stage, route):
    v = i % 3
    if route:
        out = s.rf.render(s.model, t=s.times[v], info=s.infos[v], background=s.bg, time_id=s.time_ids[v], stage=stage)
        loss = sum(s.model_loss(out, s.targets_hwc[v]).values())
    else:
        loss = s.loss_of(s.render(v, s.outputs(v, stage)), s.targets[v])
    loss.backward()
    s.opt.step()
    s.opt.zero_grad(set_to_none=True)


def time_ms(fn, iters, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(warmup + i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--P', type=int, nargs='+', default=[3000, 20000, 100000])
    ap.add_argument('--W', type=int, default=800)
    ap.add_argument('--H', type=int, default=800)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rebuilds', type=int, default=5)
    ap.add_argument('--route-only', action='store_true', help='(profiling) time the route alone')
    a = ap.parse_args()
    from sk_gs_amd import reference_fused as rf
    print(f'# stages init_fix / init, {a.W}x{a.H}, one iteration = render + image terms + backward + Adam.step + zero_grad; '
          f'HIP events over {a.iters} iterations after {a.warmup}')
    print(f'{"stage":>9} {"P":>7} {"route ms":>9} {"fallback ms":>11} {"speed-up":>8} {"rebuild ms":>10}')
    for stage in ('init_fix', 'init'):
        for P in a.P:
            s = setup(P, a.W, a.H)
            fall = None if a.route_only else time_ms(lambda i: iteration(s, i, stage, False), a.iters, a.warmup)
            fused = time_ms(lambda i: iteration(s, i, stage, True), a.iters, a.warmup)
            assert rf.calls['render_reference'] == 0, rf.why_not
            route = rf.route_of_model(s.model, stage)
            rebuild = []
            for _ in range(a.rebuilds):     # what a replaced Parameter costs: a new route and its two captures
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = rf.FusedReferenceRoute(s.model, route.W, route.H, 3, 1.0, stage)
                r._capture()
                torch.cuda.synchronize()
                rebuild.append(1e3 * (time.perf_counter() - t0))
                del r
            rb = sorted(rebuild)[len(rebuild) // 2]
            print(f'{stage:>9} {P:>7} {fused:9.3f} ' + (f'{fall:11.3f} {fall / fused:8.2f}' if fall else f'{"-":>11} {"-":>8}') + f' {rb:10.1f}',
                  flush=True)
            s.ra.restore_reference()
            if 'adam' in s.ra._originals:
                torch.optim.Adam.step = s.ra._originals.pop('adam')
            for k in list(s.ra._originals):
                s.ra._originals.pop(k)
            for k in rf.calls:
                rf.calls[k] = 0


if __name__ == '__main__':
    main()
