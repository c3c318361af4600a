"""Stage sp_fix: one iteration of the reference's loop (render + image terms + backward + the patched Adam.step + zero_grad) on the
fused route in stage sp_fix, on the same route in stage sp, and on the sp_fix fallback (the reference's sp_fix sequence, restated in torch
with the per-method fast paths: calc_LBS_weight, DeformNetwork.forward, the skinning with d_xyz / d_rotation / d_scaling detached as
sk_gs.py:1174-1178 does, the operator-path rasterizer, 0.8 L1 + 0.2 SSIM), all three on the same scene in one process, HIP events after
warm-up.

    python tools/time_sp_fix_route.py [--P 20000 100000] [--lbs W weighted_kernel] [--iters 30] [--warmup 10]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F
import torch.optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def setup(P, W, H, M, K, lbs):
    from benchlib import options, reference_loop
    args = options.build_parser().parse_args(['--reference-loop', 'fused', '--config', '9', '--views', '3', '--stage', 'sp',
                                              '--superpoints', str(M), '--knn', str(K), '--lbs-method', lbs])
    return reference_loop.setup(args, {9: dict(name=f'sp-fix-{P}', P=P, M=12, K=K, W=W, H=H)})


def fallback_outputs(s, v):
    """the sp_fix sequence on the per-method fast paths (warp LBS, no sep_rot: what reference_loop's accelerated sp branch restates)"""
    ra, L, p = s.ra, s.L, s.p
    me = s.fallback_self
    points = p['_xyz'].detach()
    if '_sp_radius' in p:
        me.kernel_radius = torch.exp(p['_sp_radius'])
    if '_sp_weight' in p:
        me.kernel_weight = torch.sigmoid(p['_sp_weight'])
    w, idx = ra.calc_LBS_weight(me, points, p['sp_points'], p['hyper_feature'], p['sp_hyper_feature'])
    out = ra.deform_network_forward(s.net, p['sp_points'].detach(), s.times[v])
    d_rot = F.normalize(out['d_rotation'] + points.new_tensor([0, 0, 0, 1.]), dim=-1)
    spT = L.SE3.InitFromVec(torch.cat([out['d_xyz'], d_rot], dim=-1))
    d_points = (spT[idx].act(points[:, None]) * w[..., None]).sum(dim=1) - points
    d_rotation, d_scales = (d_rot[idx] * w[..., None]).sum(dim=1), (out['d_scaling'][idx] * w[..., None]).sum(dim=1)
    return {'points': p['_xyz'] + d_points.detach(), 'scales': torch.exp(p['_scaling']) + d_scales.detach(),
            'rotations': F.normalize(p['_rotation'] + d_rotation.detach()), 'opacity': torch.sigmoid(p['_opacity'])}


def iteration(s, i, stage, route):
    v = i % 3
    if route:
        out = s.rf.render(s.model, t=s.times[v], info=s.infos[v], background=s.bg, time_id=s.time_ids[v], stage=stage)
        loss = sum(s.model_loss(out, s.targets_hwc[v]).values())
    else:
        loss = s.loss_of(s.render(v, fallback_outputs(s, v)), s.targets[v])
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
    import types
    ap = argparse.ArgumentParser()
    ap.add_argument('--P', type=int, nargs='+', default=[20000, 100000])
    ap.add_argument('--lbs', nargs='+', default=['W', 'weighted_kernel'])
    ap.add_argument('--W', type=int, default=800)
    ap.add_argument('--H', type=int, default=800)
    ap.add_argument('--M', type=int, default=512)
    ap.add_argument('--K', type=int, default=5)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--route-only', action='store_true', help='(profiling) time the sp_fix route alone')
    a = ap.parse_args()
    from sk_gs_amd import reference_fused as rf
    print(f'# stage sp_fix, {a.W}x{a.H}, {a.M} superpoints, K = {a.K}; one iteration = render + image terms + backward + Adam.step + '
          f'zero_grad; HIP events over {a.iters} iterations after {a.warmup}')
    print(f'{"LBS_method":>15} {"P":>7} {"sp_fix route ms":>15} {"sp route ms":>11} {"fallback ms":>11} {"speed-up":>8}')
    for lbs in a.lbs:
        for P in a.P:
            s = setup(P, a.W, a.H, a.M, a.K, lbs)
            p = s.p
            s.fallback_self = types.SimpleNamespace(training=True, sk_is_init=False, num_knn=a.K, sp_W=p.get('sp_W'), _sp_radius=p.get('_sp_radius'),
                                                    _sp_weight=p.get('_sp_weight'))
            fall = None if a.route_only else time_ms(lambda i: iteration(s, i, 'sp_fix', False), a.iters, a.warmup)
            fix = time_ms(lambda i: iteration(s, i, 'sp_fix', True), a.iters, a.warmup)
            sp = None if a.route_only else time_ms(lambda i: iteration(s, i, 'sp', True), a.iters, a.warmup)
            assert rf.calls['render_reference'] == 0 and rf.calls['routes_built'] == 1, (rf.why_not, rf.calls)
            print(f'{lbs:>15} {P:>7} {fix:15.3f} ' + (f'{sp:11.3f} {fall:11.3f} {fall / fix:8.2f}' if fall else f'{"-":>11} {"-":>11} {"-":>8}'),
                  flush=True)
            if 'sp_W' in p and hasattr(p['sp_W'], '_skgs_logit_tiles'):
                del p['sp_W']._skgs_logit_tiles
            s.ra.restore_reference()
            if 'adam' in s.ra._originals:
                torch.optim.Adam.step = s.ra._originals.pop('adam')
            for k in list(s.ra._originals):
                s.ra._originals.pop(k)
            for k in rf.calls:
                rf.calls[k] = 0
            del s


if __name__ == '__main__':
    main()
