"""Stage sp_fix on the fused reference route (sk_gs_amd/reference_fused.py + superpoint.FusedSuperpointStep.fix): the forward of stage sp,
a backward in which the image's cotangent ends at the six Gaussian tensors (networks/sk_gs.py:1174-1178 detach d_xyz / d_rotation /
d_scaling), against the reference's sp_fix sequence restated from benchlib.ref_sequence.sp_stage on the stand-ins."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SMALL = {9: dict(name='small-4k-160', P=4000, M=12, K=4, W=160, H=120)}
GAUSSIANS = ('_xyz', '_features_dc', '_features_rest', '_scaling', '_rotation', '_opacity')


def _setup(mode, extra=()):
    from benchlib import options, reference_loop
    from sk_gs_amd import reference_accel as ra, reference_fused as rf
    ra.restore_reference()
    for k in list(ra._originals):
        ra._originals.pop(k)
    for k in rf.calls:
        rf.calls[k] = 0
    rf.why_not['render'] = None
    args = options.build_parser().parse_args(['--reference-loop', mode, '--config', '9', '--views', '3', '--scale-mult', '2.0', '--stage', 'sp',
                                              '--superpoints', '128', '--knn', '4', *extra])
    s = reference_loop.setup(args, SMALL)
    s.warp, s.sep = args.warp_method, bool(args.sep_rot)
    return s


def _teardown(s):
    import torch.optim
    if 'sp_W' in s.p and hasattr(s.p['sp_W'], '_skgs_logit_tiles'):
        del s.p['sp_W']._skgs_logit_tiles
    if 'adam' in s.ra._originals:
        torch.optim.Adam.step = s.ra._originals.pop('adam')
    for k in list(s.ra._originals):
        s.ra._originals.pop(k)


def _sp_fix_stage(s, v):
    """ref_sequence.sp_stage with the stage's detach (sk_gs.py:1174-1178): d_xyz, d_rotation, d_scaling leave the graph"""
    from benchlib import ref_sequence as rs
    SE3, SO3 = s.L.SE3, s.L.SO3
    out = s.net.reference_forward(s.p['sp_points'].detach(), s.times[v])
    a = dict(s.p)
    points, sp_points = a['_xyz'].detach(), a['sp_points']
    bias = points.new_tensor([0, 0, 0, 1.])
    w, idx = rs._lbs_weights(s.p3d.knn_points, a, points, sp_points, s.K, a['hyper_feature'], a['sp_hyper_feature'])
    d_rot = F.normalize(out['d_rotation'] + bias, dim=-1)
    g_rot = F.normalize(out['g_rotation'] + bias, dim=-1) if s.sep else None
    p2sp = torch.gather(idx, -1, w.argmax(dim=-1, keepdim=True))[:, 0] if s.warp == 'largest' else None
    sp_t = out['d_xyz']
    if s.warp == 'LBS_c':
        sp_t = sp_t + sp_points + SO3.InitFromVec(d_rot).act(-sp_points)
    spT = SE3.InitFromVec(torch.cat([sp_t, d_rot], dim=-1))
    if s.warp in ('LBS', 'LBS_c'):
        d_points = (spT[idx].act(points[:, None]) * w[..., None]).sum(dim=1) - points
    else:
        d_points = spT[p2sp].act(points) - points
    d_rotation = ((g_rot if g_rot is not None else d_rot)[idx] * w[..., None]).sum(dim=1)
    d_scales = (out['d_scaling'][idx] * w[..., None]).sum(dim=1)
    res = rs._activate(a, d_points.detach(), d_rotation.detach(), d_scales.detach())
    res.update(_spT=spT.vec(), _knn_w=w, _knn_i=idx, _sp_scale=out['d_scaling'])
    if s.sep:
        res['_sp_rot'] = g_rot
    if p2sp is not None:
        res['p2sp'] = p2sp
    return res


def _names(s):
    names = dict(s.p)
    names.update({f'net.{n}': q for n, q in s.net.named_parameters()})
    return names


def _clear(names):
    for q in names.values():
        q.grad = None


def _render(s, v, stage):
    return s.rf.render(s.model, t=s.times[v], info=s.infos[v], background=s.bg, time_id=s.time_ids[v], stage=stage)


def _close(got, want, rel):
    scale = float(want.abs().max())
    return float((got - want).abs().max()) <= rel * scale + 1e-12, (float((got - want).abs().max()), scale)


@pytest.mark.parametrize('warp,lbs,sep', [('LBS', 'weighted_kernel', False), ('largest', 'W', False), ('LBS_c', 'dist', True)])
def test_one_sp_fix_iteration_matches_the_reference(warp, lbs, sep):
    """forward values, the loss and the six Gaussian gradients equal the reference's sp_fix sequence; every deform parameter -- the
    network, the weighting's tables, sp_points -- ends the backward with ``.grad is None``, as in the reference"""
    s = _setup('fused', ('--warp-method', warp, '--lbs-method', lbs) + (('--sep-rot',) if sep else ()))
    try:
        rf, v, names = s.rf, 2, _names(s)
        _clear(names)
        res = _sp_fix_stage(s, v)
        loss_ref = s.loss_of(s.render(v, res), s.targets[v])
        loss_ref.backward()
        want = {n: (None if q.grad is None else q.grad.detach().clone()) for n, q in names.items()}
        assert all(want[n] is None for n in names if n not in GAUSSIANS)       # (the restatement detaches what the reference detaches)
        _clear(names)
        out = _render(s, v, 'sp_fix')
        assert rf.calls['render_fused'] == 1 and rf.calls['render_reference'] == 0, rf.why_not
        assert out['stage'] == 'sp_fix' and tuple(out['_knn_i'].shape) == (1, s.P, s.K) and ('_sp_rot' in out) == sep
        assert float((out['_spT'][0] - res['_spT']).abs().max()) <= 2e-6 and float((out['_knn_w'][0] - res['_knn_w']).abs().max()) <= 2e-6
        assert float((out['points'][0] - res['points']).abs().max()) <= 2e-5
        if sep:
            assert float((out['_sp_rot'][0] - res['_sp_rot']).abs().max()) <= 2e-6
        if warp == 'largest':
            assert torch.equal(s.model.p2sp, res['p2sp'])
        assert s.model.sp_weights is not None and s.model.sp_knn is not None
        loss = sum(s.model_loss(out, s.targets_hwc[v]).values())
        assert abs(float(loss) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref))
        loss.backward()
        for n, q in names.items():
            if n in GAUSSIANS:
                ok, info = _close(q.grad, want[n], 3e-4)
                assert ok, (n, info)
            else:
                assert q.grad is None, n
        assert rf.route_of_model(s.model, 'sp_fix') is rf.route_of_model(s.model, 'sp') is not None
    finally:
        _teardown(s)


def test_sp_fix_and_sp_give_the_same_gaussian_gradients():
    """the same state and view rendered in sp and in sp_fix: one route, and the six Gaussian gradients come from the same expressions
    (they differ by the rounding of the blend backward's float atomics at most)"""
    s = _setup('fused')
    try:
        rf, v, names = s.rf, 1, _names(s)
        got = {}
        for stage in ('sp', 'sp_fix', 'sp'):
            _clear(names)
            out = _render(s, v, stage)
            sum(s.model_loss(out, s.targets_hwc[v]).values()).backward()
            got.setdefault(stage, {n: names[n].grad.detach().clone() for n in GAUSSIANS})
            if stage == 'sp_fix':
                assert all(names[n].grad is None for n in names if n not in GAUSSIANS)
            else:
                assert names['sp_W' if 'sp_W' in names else '_sp_radius'].grad is not None
        for n in GAUSSIANS:
            ok, info = _close(got['sp_fix'][n], got['sp'][n], 1e-5)
            assert ok, (n, info)
        assert rf.calls['routes_built'] == 1 and rf.calls['render_fused'] == 3
    finally:
        _teardown(s)


@pytest.mark.parametrize('lbs', ['weighted_kernel', 'W'])
def test_sp_fix_cotangents_on_the_weights_and_transforms_are_exact(lbs):
    """sp_fix with the shipped regularisers on outputs['_knn_w'] and a term on outputs['_spT']: the Gaussians get the image's gradient
    alone, the weighting's parameters and the network (but its scaling head) get what the extra terms give them"""
    s = _setup('fused', ('--sp-regularisers', '--lbs-method', lbs))
    try:
        rf, v, names = s.rf, 1, _names(s)
        gT = torch.randn(s.M, 7, generator=torch.Generator().manual_seed(5)).cuda() * 1e-3
        _clear(names)
        res = _sp_fix_stage(s, v)
        loss_ref = s.loss_of(s.render(v, res), s.targets[v]) + s.weight_regularisers(res['_knn_w'][None]) + (res['_spT'] * gT).sum()
        loss_ref.backward()
        want = {n: (None if q.grad is None else q.grad.detach().clone()) for n, q in names.items()}
        _clear(names)
        out = _render(s, v, 'sp_fix')
        assert rf.calls['render_fused'] == 1, rf.why_not
        loss = sum(s.model_loss(out, s.targets_hwc[v]).values()) + (out['_spT'][0] * gT).sum()
        assert abs(float(loss) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref))
        loss.backward()
        assert rf.calls['backward_extras'] == 1
        for n, q in names.items():
            if want[n] is None:
                assert q.grad is None, n
                continue
            assert q.grad is not None, n
            # (the network's gradients here come from the small random-sign `_spT` term alone; the MFMA backward against torch's lands
            # up to ~3e-2 of the largest entry of a tensor -- measured, not explained: the bound below is that, not a derived one)
            ok, info = _close(q.grad, want[n], 5e-2 if n.startswith('net.') else 3e-4)
            assert ok, (n, info)
        assert names['net.gaussian_warp.weight'].grad is not None and names['net.gaussian_scaling.weight'].grad is None
    finally:
        _teardown(s)


@pytest.mark.parametrize('lbs', ['weighted_kernel', 'W'])
def test_schedule_boundary_sp_fix_then_sp(lbs):
    """10 iterations of sp_fix, then 10 of sp, on one model: through the route and through the per-method fast paths (the restated
    sequence); same losses, the logit table where the dense update leaves it, one route across the boundary"""
    runs, tables = {}, {}
    for mode in ('accelerated', 'fused'):
        s = _setup(mode, ('--lbs-method', lbs))
        try:
            losses = []
            for i in range(20):
                stage, v = ('sp_fix' if i < 10 else 'sp'), i % 3
                if mode == 'fused':
                    out = _render(s, v, stage)
                    loss = sum(s.model_loss(out, s.targets_hwc[v]).values())
                    loss.backward()
                    s.opt.step()
                    s.opt.zero_grad(set_to_none=True)
                else:
                    s.opt.zero_grad(set_to_none=True)
                    res = _sp_fix_stage(s, v) if stage == 'sp_fix' else s.deform(v)
                    loss = s.loss_of(s.render(v, res), s.targets[v])
                    loss.backward()
                    s.opt.step()
                losses.append(float(loss))
            torch.cuda.synchronize()
            runs[mode] = losses
            if lbs == 'W':
                tables[mode] = s.p['sp_W'].detach().clone()
            if mode == 'fused':
                assert s.rf.calls['render_fused'] == 20 and s.rf.calls['render_reference'] == 0, s.rf.why_not
                assert s.rf.calls['routes_built'] == 1
        finally:
            _teardown(s)
    for a, b in zip(runs['accelerated'], runs['fused']):
        assert abs(a - b) <= 2e-3 * abs(a), runs
    if lbs == 'W':
        d = (tables['accelerated'] - tables['fused']).abs()
        assert float((d > 1e-4).float().mean()) < 2e-3, float((d > 1e-4).float().mean())


def test_building_the_sp_route_releases_the_init_route(monkeypatch):
    """a stand-in that both stages accept: the init route, then sp_fix -- the init route is dropped before the sp route is built, and
    its network buffers (skgs_sp_net_rows saved + workspace) go with it"""
    s = _setup('fused')
    try:
        rf, v, names = s.rf, 0, _names(s)
        _clear(names)
        out = _render(s, v, 'init')
        sum(s.model_loss(out, s.targets_hwc[v]).values()).backward()
        init = rf.route_of_model(s.model, 'init')
        assert init is not None and rf.calls['render_fused'] == 1, rf.why_not
        held = init.step.saved.numel() + init.step.net_ws.numel()
        del out, init
        _clear(names)
        seen = []
        release = rf.FusedReferenceRoute.release

        def measured(self):
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            release(self)
            torch.cuda.synchronize()
            seen.append(before - torch.cuda.memory_allocated())
        monkeypatch.setattr(rf.FusedReferenceRoute, 'release', measured)
        out = _render(s, v, 'sp_fix')
        sum(s.model_loss(out, s.targets_hwc[v]).values()).backward()
        assert rf.route_of_model(s.model, 'init') is None and rf.route_of_model(s.model, 'sp_fix') is not None
        assert rf.calls['routes_released'] == 1 and len(seen) == 1
        assert seen[0] >= held, (seen, held)
    finally:
        _teardown(s)


def test_abi_image_to_deform_off_leaves_the_deform_side_untouched():
    """fixed upstream gradients through the standalone entry point with and without the flag: bit-identical Gaussian gradients; with the
    flag the weights' / superpoints' gradient buffers keep their sentinel.  Through skgs_rasterize_backward the fix job does the same."""
    from sk_gs_amd import _C
    s = _setup('fused', ('--lbs-method', 'weighted_kernel'))
    try:
        rf, v, names = s.rf, 0, _names(s)
        _clear(names)
        out = _render(s, v, 'sp_fix')
        route = rf.route_of_model(s.model, 'sp_fix')
        st, lib = route.step, route.lib
        P, M, K, dev = s.P, s.M, s.K, s.p['_xyz'].device
        # ---- through the rasterizer's backward (the route's plain sp_fix graph): the deform side's buffers keep a sentinel
        SENT = 1234.5
        side = [st.g_weights, st.g_bone_T, st.g_d_rot, st.g_d_scale] + [route.grads[q] for q in route.grads if not any(
            q is names[n] for n in GAUSSIANS)]
        for b in side:
            b.fill_(SENT)
        sum(s.model_loss(out, s.targets_hwc[v]).values()).backward()
        torch.cuda.synchronize()
        assert all(bool((b == SENT).all()) for b in side)
        # ---- standalone, with fixed upstream gradients
        g = torch.Generator(device='cpu').manual_seed(3)
        up = [torch.randn(P, c, generator=g).to(dev) for c in (3, 3, 4, 1)]
        d = st._deform_inputs(None)

        def run(flag):
            outs = {k: torch.full(shape, SENT, device=dev) for k, shape in (
                ('g_xyz', (P, 3)), ('g_log_scale', (P, 3)), ('g_rot', (P, 4)), ('g_opacity_logit', (P, 1)), ('g_weights', (P, K)),
                ('g_feature', (P, 8)), ('g_bone_T', (M, 7)), ('g_bone_drot', (M, 4)), ('g_bone_dscale', (M, 3)), ('g_sp_feature', (M, 8)),
                ('g_sp_radius', (M,)), ('g_sp_weight', (M,)))}
            j = st._skinning_job(d)
            for k, t in outs.items():
                setattr(j, k, t.data_ptr())
            j.g_weights_extra, j.image_to_deform_off = None, flag     # (the step keeps the cotangent buffer of its last eager extras call)
            _C._check(lib.skgs_sp_skinning_backward_job(C.byref(j), *[C.c_void_p(t.data_ptr()) for t in up], _C._stream()))
            torch.cuda.synchronize()
            return outs
        a, b = run(0), run(1)
        for k in ('g_xyz', 'g_log_scale', 'g_rot', 'g_opacity_logit'):
            assert torch.equal(a[k], b[k]) and not bool((a[k] == SENT).any()), k
        for k in ('g_weights', 'g_feature', 'g_bone_T', 'g_bone_drot', 'g_bone_dscale', 'g_sp_feature', 'g_sp_radius', 'g_sp_weight'):
            assert bool((b[k] == SENT).all()) and not bool((a[k] == SENT).all()), k
    finally:
        _teardown(s)
