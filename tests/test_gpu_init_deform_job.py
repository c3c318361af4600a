"""Stages init_fix / init as a job of the rasterizer's per-Gaussian launches (include/skgs.h: skgs_offset_deform_job), through the C ABI:
the forward job's image is bit-identical to the plain rasterizer fed the tensors the job wrote; its backward gives the plain backward's
mean gradient bit for bit (into g_xyz and columns 0:3 of the network's g_raw), the normalize / sigmoid chain and the log-scale mean's
backward within fp32 rounding of fp64; repeated calls give the same bits; every refused combination returns an error and launches
nothing."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

W, H = 320, 240


def _lib():
    from sk_gs_amd import _C
    return _C, _C.load_library()


class _Scene:
    def __init__(self, P, stride, seed=0):
        from sk_gs_amd import _C, scene
        dev = torch.device('cuda')
        g = torch.Generator().manual_seed(seed + 11)
        gs = scene.make_gaussians(P, seed=seed, sh_degree=3, scale_mult=2.0)
        f32 = dict(dtype=torch.float32, device=dev)
        self.P, self.stride = P, stride
        self.xyz = gs['xyz'].to(dev).contiguous()
        self.log_scale = gs['log_scale'].to(dev).contiguous()
        self.rot = gs['rot'].to(dev).contiguous()
        self.op = gs['opacity_logit'].reshape(P, 1).to(dev).contiguous()
        self.dc, self.rest = gs['sh'][:, :1].to(dev).contiguous(), gs['sh'][:, 1:].to(dev).contiguous()
        self.raw = (torch.randn(P, stride, generator=g) * 0.02).to(dev)
        self.rs = scene.raster_settings_from_camera(scene.make_camera(W, H, seed=seed), sh_degree=3, colmap=True, device=dev)
        self.bg = torch.ones(3, **f32)
        self.dimage = (torch.randn(3, H, W, generator=g) * 1e-3).to(dev)
        _, lib = _lib()
        self.ws_bytes = int(lib.skgs_offset_deform_workspace_bytes(C.c_int32(P)))
        self.f32 = f32

    def buffers(self):
        from sk_gs_amd import _C
        _, lib = _lib()
        dev = self.xyz.device
        u8 = dict(dtype=torch.uint8, device=dev)
        geom = torch.zeros((lib.skgs_geom_buffer_bytes(C.c_int32(self.P)),), **u8)
        img = torch.zeros((lib.skgs_img_buffer_bytes(C.c_int32(W), C.c_int32(H)),), **u8)
        binning = torch.zeros((lib.skgs_binning_buffer_bytes(C.c_int64(64 * self.P + 64 * 1200)),), **u8)
        return geom, binning, img, _C._buffers(geom, binning, img)

    def inputs(self, means, scales, rots, op):
        from sk_gs_amd import _C
        a = _C._RasterInputs()
        rs = self.rs
        a.P, a.sh_degree, a.sh_coeffs, a.E, a.image_height, a.image_width = self.P, 3, 16, 0, H, W
        a.tanfovx, a.tanfovy, a.scale_modifier, a.prefiltered, a.debug, a.colmap = rs.tanfovx, rs.tanfovy, 1.0, 0, 0, 1
        a.viewmatrix, a.projmatrix, a.campos = rs.viewmatrix.data_ptr(), rs.projmatrix.data_ptr(), rs.campos.data_ptr()
        a.means3D, a.scales, a.rotations, a.opacity = means.data_ptr(), scales.data_ptr(), rots.data_ptr(), op.data_ptr()
        a.sh, a.sh_rest, a.background = self.dc.data_ptr(), self.rest.data_ptr(), self.bg.data_ptr()
        return a

    def outputs(self):
        P, f32 = self.P, self.f32
        return torch.full((P, 3), 7.0, **f32), torch.full((P, 3), 7.0, **f32), torch.full((P, 4), 7.0, **f32), torch.full((P, 1), 7.0, **f32)

    def job(self, mode, means, scales, rots, op, ws, mean_word):
        from sk_gs_amd import _C
        j = _C._OffsetDeformJob()
        j.scale_mode, j.d_xyz_stride = mode, self.stride
        j.xyz, j.d_xyz, j.log_scale, j.rot, j.opacity_logit = (self.xyz.data_ptr(), self.raw.data_ptr(), self.log_scale.data_ptr(),
                                                              self.rot.data_ptr(), self.op.data_ptr())
        j.scale_mean = mean_word.data_ptr()
        j.means, j.scales, j.rotations, j.opacity = means.data_ptr(), scales.data_ptr(), rots.data_ptr(), op.data_ptr()
        j.workspace, j.workspace_bytes = ws.data_ptr(), ws.numel()
        return j


def _forward(s, a, bufs, radii, image, opac):
    _C, lib = _lib()
    return lib.skgs_rasterize_forward(C.byref(a), C.byref(bufs), C.c_void_p(radii.data_ptr()), C.c_void_p(image.data_ptr()),
                                      C.c_void_p(opac.data_ptr()), None, None, _C._stream())


def _grads(s, P, ws_bw):
    from sk_gs_amd import _C
    g = _C._RasterGrads()
    g.dL_dout_color = s.dimage.data_ptr()
    g.workspace, g.workspace_bytes, g.workspace_is_zero = ws_bw.data_ptr(), ws_bw.numel(), 0
    return g


def _run_job(s, mode, with_g_raw=True):
    """forward + backward with the job: (means, scales, rots, op, image, radii, mean word, gradients dict)"""
    _C, lib = _lib()
    P, f32 = s.P, s.f32
    means, scales, rots, op = s.outputs()
    ws = torch.zeros((s.ws_bytes,), dtype=torch.uint8, device=s.xyz.device)
    mean_word = torch.zeros(1, **f32)
    j = s.job(mode, means, scales, rots, op, ws, mean_word)
    a = s.inputs(means, scales, rots, op)
    a.offset_job = C.cast(C.pointer(j), C.c_void_p)
    geom, binning, img, bufs = s.buffers()
    radii, image, opac = torch.zeros(P, dtype=torch.int32, device=s.xyz.device), torch.zeros(3, H, W, **f32), torch.zeros(H, W, **f32)
    _C._check(_forward(s, a, bufs, radii, image, opac))
    a.offset_job = None
    out = dict(g_xyz=torch.full((P, 3), 5.0, **f32), g_raw=torch.zeros((P, s.stride), **f32), g_ls=torch.full((P, 3), 5.0, **f32),
               g_rot=torch.full((P, 4), 5.0, **f32), g_op=torch.full((P, 1), 5.0, **f32), g_m2=torch.zeros((P, 3), **f32),
               g_dc=torch.zeros((P, 1, 3), **f32), g_rest=torch.zeros((P, 15, 3), **f32),
               # the rasterizer's own per-Gaussian gradients of the SAME launch (a job leaves them optional): the blend backward sums
               # with float atomics, so two backward calls may differ in the last bits -- the job is compared with its own launch
               r_m3=torch.zeros((P, 3), **f32), r_s=torch.zeros((P, 3), **f32), r_r=torch.zeros((P, 4), **f32), r_op=torch.zeros((P, 1), **f32),
               r_col=torch.zeros((P, 3), **f32), r_cov=torch.zeros((P, 6), **f32))
    j.g_xyz, j.g_log_scale, j.g_rot, j.g_opacity_logit = out['g_xyz'].data_ptr(), out['g_ls'].data_ptr(), out['g_rot'].data_ptr(), out['g_op'].data_ptr()
    j.g_d_xyz = out['g_raw'].data_ptr() if with_g_raw else None
    ws_bw = torch.zeros((lib.skgs_backward_workspace_bytes(C.c_int32(P)),), dtype=torch.uint8, device=s.xyz.device)
    g = _grads(s, P, ws_bw)
    g.dL_dmeans2D, g.dL_dsh, g.dL_dsh_rest = out['g_m2'].data_ptr(), out['g_dc'].data_ptr(), out['g_rest'].data_ptr()
    g.dL_dmeans3D, g.dL_dscales, g.dL_drotations, g.dL_dopacity = (out['r_m3'].data_ptr(), out['r_s'].data_ptr(), out['r_r'].data_ptr(),
                                                                   out['r_op'].data_ptr())
    g.dL_dcolors, g.dL_dcov3D = out['r_col'].data_ptr(), out['r_cov'].data_ptr()
    g.offset_job = C.cast(C.pointer(j), C.c_void_p)
    _C._check(lib.skgs_rasterize_backward(C.byref(a), C.byref(bufs), C.c_void_p(radii.data_ptr()), C.c_void_p(opac.data_ptr()), C.byref(g),
                                          _C._stream()))
    torch.cuda.synchronize()
    return means, scales, rots, op, image, radii, mean_word, out


def _run_plain(s, means, scales, rots, op):
    _C, lib = _lib()
    P, f32 = s.P, s.f32
    means, scales, rots, op = means.clone(), scales.clone(), rots.clone(), op.clone()
    a = s.inputs(means, scales, rots, op)
    geom, binning, img, bufs = s.buffers()
    radii, image, opac = torch.zeros(P, dtype=torch.int32, device=s.xyz.device), torch.zeros(3, H, W, **f32), torch.zeros(H, W, **f32)
    _C._check(_forward(s, a, bufs, radii, image, opac))
    out = dict(g_m2=torch.zeros((P, 3), **f32), g_col=torch.zeros((P, 3), **f32), g_op=torch.zeros((P, 1), **f32), g_m3=torch.zeros((P, 3), **f32),
               g_cov=torch.zeros((P, 6), **f32), g_dc=torch.zeros((P, 1, 3), **f32), g_rest=torch.zeros((P, 15, 3), **f32),
               g_s=torch.zeros((P, 3), **f32), g_r=torch.zeros((P, 4), **f32))
    ws_bw = torch.zeros((lib.skgs_backward_workspace_bytes(C.c_int32(P)),), dtype=torch.uint8, device=s.xyz.device)
    g = _grads(s, P, ws_bw)
    g.dL_dmeans2D, g.dL_dcolors, g.dL_dopacity, g.dL_dmeans3D = out['g_m2'].data_ptr(), out['g_col'].data_ptr(), out['g_op'].data_ptr(), out['g_m3'].data_ptr()
    g.dL_dcov3D, g.dL_dsh, g.dL_dsh_rest = out['g_cov'].data_ptr(), out['g_dc'].data_ptr(), out['g_rest'].data_ptr()
    g.dL_dscales, g.dL_drotations = out['g_s'].data_ptr(), out['g_r'].data_ptr()
    _C._check(lib.skgs_rasterize_backward(C.byref(a), C.byref(bufs), C.c_void_p(radii.data_ptr()), C.c_void_p(opac.data_ptr()), C.byref(g),
                                          _C._stream()))
    torch.cuda.synchronize()
    return image, radii, out


@pytest.mark.parametrize('mode,stride,P', [(0, 10, 20011), (1, 14, 20011), (0, 14, 3000), (1, 10, 3000)])
def test_offset_job_forward_and_backward_against_the_plain_rasterizer(mode, stride, P):
    s = _Scene(P, stride, seed=mode + stride)
    means, scales, rots, op, image, radii, mean_word, jg = _run_job(s, mode)
    # forward: means = xyz + d_xyz bitwise; the mean, the scales, rotation and opacity against fp64
    assert torch.equal(means, s.xyz + s.raw[:, 0:3])
    ls64 = s.log_scale.double()
    if mode == 0:
        want = ls64.mean()
        assert abs(float(mean_word[0]) - float(want)) <= 1e-6 * abs(float(want))
        assert torch.equal(scales, torch.exp(mean_word).expand(P, 3))
    else:
        want = torch.exp(ls64.mean(dim=1, keepdim=True)).expand(P, 3)
        assert float(((scales.double() - want) / want).abs().max()) <= 1e-6
    r64 = s.rot.double()
    assert float((rots.double() - r64 / r64.norm(dim=-1, keepdim=True).clamp_min(1e-12)).abs().max()) <= 1e-6
    assert float((op.double() - torch.sigmoid(s.op.double())).abs().max()) <= 1e-6
    # the image: bit-identical to the plain rasterizer fed the tensors the job wrote
    image2, radii2, pg = _run_plain(s, means, scales, rots, op)
    assert torch.equal(image, image2) and torch.equal(radii, radii2) and int((radii > 0).sum()) > P // 10
    # backward: the mean gradient bit for bit, into g_xyz and columns 0:3 of g_raw (the other columns untouched)
    assert torch.equal(jg['g_xyz'], jg['r_m3']) and torch.equal(jg['g_raw'][:, 0:3], jg['r_m3'])
    assert float(jg['g_raw'][:, 3:].abs().max()) == 0.0 and float(jg['r_m3'].abs().max()) > 0
    # ... and the plain rasterizer's backward of the same image computes the same gradients (up to the blend's atomics)
    for k_job, k_plain in (('r_m3', 'g_m3'), ('r_s', 'g_s'), ('r_r', 'g_r'), ('r_op', 'g_op'), ('g_m2', 'g_m2'), ('g_rest', 'g_rest')):
        assert float((jg[k_job] - pg[k_plain]).abs().max()) <= 1e-5 * float(pg[k_plain].abs().max()), k_job
    # normalize / sigmoid of the rasterizer's outputs in fp64
    n = r64.norm(dim=-1, keepdim=True)
    u, gr = r64 / n, jg['r_r'].double()
    want_rot = (gr - u * (u * gr).sum(-1, keepdim=True)) / n
    # (every Gaussian here is a sphere -- one scale for its three axes -- so the true rotation gradient is ~0 and what both sides hold is
    # the projection's cancellation of a radial component: bounded by fp32 rounding of the chain's INPUT, |dL/drotation| / |rot|)
    assert float((jg['g_rot'].double() - want_rot).abs().max()) <= 1e-5 * float((gr / n).abs().max())
    sg = torch.sigmoid(s.op.double())
    want_op = jg['r_op'].double() * sg * (1 - sg)
    assert float((jg['g_op'].double() - want_op).abs().max()) <= 1e-5 * float(want_op.abs().max())
    # the log-scale mean's backward
    terms = jg['r_s'].double() * scales.double()
    if mode == 0:
        want = terms.sum() / (3 * P)
        assert torch.equal(jg['g_ls'], jg['g_ls'][0, 0].expand(P, 3))
        assert abs(float(jg['g_ls'][0, 0]) - float(want)) <= 1e-6 * float(terms.abs().sum()) / (3 * P)
    else:
        want = (terms.sum(dim=1, keepdim=True) / 3).expand(P, 3)
        assert float((jg['g_ls'].double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    # same inputs, same bits: the forward always; the job's gradients whenever the rasterizer's (atomics) came out the same
    again = _run_job(s, mode)
    for x, y in zip((means, scales, rots, op, image, radii, mean_word), again[:7]):
        assert torch.equal(x, y)
    ag = again[7]
    if all(torch.equal(jg[k], ag[k]) for k in ('r_m3', 'r_s', 'r_r', 'r_op')):
        for k in ('g_xyz', 'g_raw', 'g_ls', 'g_rot', 'g_op'):
            assert torch.equal(jg[k], ag[k]), k
    # init_fix: no g_d_xyz pointer, the rest unchanged
    fix = _run_job(s, mode, with_g_raw=False)[7]
    assert float(fix['g_raw'].abs().max()) == 0.0 and torch.equal(fix['g_xyz'], fix['r_m3'])


def test_refused_combinations_return_an_error_and_launch_nothing():
    _C, lib = _lib()
    s = _Scene(2000, 10)
    P, f32 = s.P, s.f32
    knn = _C._KnnDeformJob()
    live = torch.tensor([P], dtype=torch.int32, device=s.xyz.device)
    cov = torch.zeros((P, 6), **f32)

    def attempt(edit_job=None, edit_inputs=None):
        means, scales, rots, op = s.outputs()
        ws = torch.zeros((s.ws_bytes,), dtype=torch.uint8, device=s.xyz.device)
        mean_word = torch.full((1,), 3.0, **f32)
        j = s.job(0, means, scales, rots, op, ws, mean_word)
        if edit_job:
            edit_job(j)
        a = s.inputs(means, scales, rots, op)
        a.offset_job = C.cast(C.pointer(j), C.c_void_p)
        if edit_inputs:
            edit_inputs(a)
        geom, binning, img, bufs = s.buffers()
        radii, image, opac = torch.zeros(P, dtype=torch.int32, device=s.xyz.device), torch.zeros(3, H, W, **f32), torch.zeros(H, W, **f32)
        rc = _forward(s, a, bufs, radii, image, opac)
        torch.cuda.synchronize()
        untouched = float((means - 7.0).abs().max()) == 0.0 and float(mean_word[0]) == 3.0 and float(image.abs().max()) == 0.0
        return rc, lib.skgs_last_error().decode(), untouched

    assert attempt()[0] == 0
    cases = [(None, lambda a: setattr(a, 'deform_job', C.pointer(knn)), 'deform_job'),
             (None, lambda a: setattr(a, 'live_count', live.data_ptr()), 'live_count'),
             (None, lambda a: [setattr(a, 'cov3D_precomp', cov.data_ptr()), setattr(a, 'scales', None), setattr(a, 'rotations', None)],
              'cov3D_precomp'),
             (lambda j: setattr(j, 'd_xyz_stride', 2), None, 'stride'),
             (lambda j: setattr(j, 'd_xyz', None), None, 'NULL'),
             (lambda j: setattr(j, 'scale_mean', None), None, 'NULL'),
             (lambda j: setattr(j, 'workspace', None), None, 'workspace')]
    for ej, ei, word in cases:
        rc, msg, untouched = attempt(ej, ei)
        assert rc != 0 and word in msg and untouched, (word, msg)
    # the backward: with another job, with a row capacity, a NULL gradient pointer, a stride below 3
    from sk_gs_amd import _C as CC
    means, scales, rots, op, image, radii, mean_word, jg = _run_job(s, 0)
    ws = torch.zeros((s.ws_bytes,), dtype=torch.uint8, device=s.xyz.device)
    sentinel = torch.full((P, 3), 5.0, **f32)
    bufs = s.buffers()[3]
    ws_bw = torch.zeros((lib.skgs_backward_workspace_bytes(C.c_int32(P)),), dtype=torch.uint8, device=s.xyz.device)
    g_m2 = torch.zeros((P, 3), **f32)
    spj = CC._SpSkinningJob()
    for edit, word in ((lambda g, j, a: setattr(g, 'sp_skinning_job', C.cast(C.pointer(spj), C.c_void_p)), 'sp_skinning_job'),
                       (lambda g, j, a: setattr(a, 'live_count', live.data_ptr()), 'live_count'),
                       (lambda g, j, a: setattr(j, 'g_rot', None), 'NULL'),
                       (lambda g, j, a: setattr(j, 'd_xyz_stride', 1), 'stride')):
        j = s.job(0, means, scales, rots, op, ws, mean_word)
        j.g_xyz, j.g_log_scale, j.g_rot, j.g_opacity_logit = sentinel.data_ptr(), sentinel.data_ptr(), jg['g_rot'].data_ptr(), jg['g_op'].data_ptr()
        a = s.inputs(means, scales, rots, op)
        g = _grads(s, P, ws_bw)
        g.dL_dmeans2D, g.dL_dsh, g.dL_dsh_rest = g_m2.data_ptr(), jg['g_dc'].data_ptr(), jg['g_rest'].data_ptr()
        g.offset_job = C.cast(C.pointer(j), C.c_void_p)
        edit(g, j, a)
        rc = lib.skgs_rasterize_backward(C.byref(a), C.byref(bufs), C.c_void_p(radii.data_ptr()), C.c_void_p(image.data_ptr()), C.byref(g),
                                         CC._stream())
        torch.cuda.synchronize()
        assert rc != 0 and word in lib.skgs_last_error().decode(), (word, lib.skgs_last_error())
        assert float((sentinel - 5.0).abs().max()) == 0.0 and float(g_m2.abs().max()) == 0.0
