"""GPU tests of the superpoint stage's deform network on P rows (csrc/sp_net_rows.hip: stages init_fix / init, every Gaussian):
raw outputs and every parameter gradient against fp64 restatements of ``SpDeformNet.reference_forward`` (itself pinned to the
reference's DeformNetwork by tests/golden/sp_deformnet.npz), bit-identical repeats, the init iteration's interleaved calls, the
routing of ``reference_accel.deform_network_forward``, the memory of a no-grad call, and the C ABI's edge cases.

Gradients are compared on the kernel's own ReLU decisions (read from its saved activations): at 100 k rows x 8 x 256 features some
pre-activations lie within rounding of 0, and one flip moves a weight gradient by a whole row's contribution, which says nothing
about either evaluation.  The decisions themselves are checked against fp64's: they may differ only where fp64's pre-activation
is within rounding of 0."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REF_ERR_FACTOR = 2.0
VARIANTS = {  # name: (is_blender, t_degree, sep_rot)
    'blender': (True, 6, False),
    'raw10': (False, 10, False),
    'raw0': (False, 0, False),
    'sep_rot': (True, 6, True),
}


def rel_err(a, b) -> float:
    """max-norm relative error, the reference's metric"""
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) if b.numel() else 0.0


def _net(variant='blender', seed=0):
    from sk_gs_amd.superpoint import SpDeformNet
    blender, t_degree, sep = VARIANTS[variant]
    torch.manual_seed(seed)
    net = SpDeformNet(is_blender=blender, t_degree=t_degree, sep_rot=sep)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():  # heads of a readable size (reset_parameters leaves them at 1e-5 / 1e-8), as the superpoint tests draw them
        heads = [net.gaussian_warp, net.gaussian_scaling, net.gaussian_rotation] + ([net.local_rotation] if sep else [])
        for head in heads:
            head.weight.normal_(0, 0.05, generator=g)
            head.bias.normal_(0, 0.1, generator=g)
        for layer in net.linear:
            layer.bias.normal_(0, 0.05, generator=g)
        if blender:
            net.timenet[0].bias.normal_(0, 0.1, generator=g)
    return net.cuda()


def _points(P, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(P, 3, generator=g) * 2 - 1).cuda()


def _keys(net):
    return ('d_xyz', 'd_rotation', 'd_scaling') + (('g_rotation',) if net.sep_rot else ())


def _raw_of(out, net):
    return torch.cat([out[k] for k in _keys(net)], 1)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def _lib():
    from sk_gs_amd.superpoint import _rows_lib
    return _rows_lib()


def _abi_forward(net, x, t, saved=True):
    """(rc, raw, saved buffer or None)"""
    from sk_gs_amd import _C
    from sk_gs_amd.superpoint import _net_desc
    lib, P = _lib(), x.shape[0]
    raw = torch.full((P, 14 if net.sep_rot else 10), float('nan'), device='cuda')
    sv = torch.empty((int(lib.skgs_sp_net_rows_saved_bytes(C.c_int32(P))),), dtype=torch.uint8, device='cuda') if saved else None
    d = _net_desc(net, P, x, t)
    rc = lib.skgs_sp_net_rows_forward(C.byref(d), C.c_void_p(raw.data_ptr()), C.c_void_p(None if sv is None else sv.data_ptr()),
                                      C.c_size_t(0 if sv is None else sv.numel()), _C._stream())
    return rc, raw, sv


def _abi_backward(net, g_raw, sv):
    """every parameter's gradient (a list in net.parameters() order), written by the kernels into NaN-filled tensors"""
    from sk_gs_amd import _C
    from sk_gs_amd.superpoint import _net_desc
    lib, P = _lib(), g_raw.shape[0]
    ws = torch.empty((int(lib.skgs_sp_net_rows_workspace_bytes(C.c_int32(P))),), dtype=torch.uint8, device='cuda')
    params = list(net.parameters())
    keep = [p.grad for p in params]
    for p in params:
        p.grad = torch.full_like(p, float('nan'))
    try:
        d, dg = _net_desc(net, P, None, None), _net_desc(net, P, None, None, grads=True)
        _C._check(lib.skgs_sp_net_rows_backward(C.byref(d), C.byref(dg), C.c_void_p(g_raw.data_ptr()), C.c_void_p(sv.data_ptr()),
                                                C.c_size_t(sv.numel()), C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel()), _C._stream()))
        return [p.grad for p in params]
    finally:
        for p, k in zip(params, keep):
            p.grad = k


def _kernel_masks(sv, P):
    """the kernel's ReLU decisions [8][P,256] from its saved activations: header 512 floats | x0 [Pp][64] | Y [8][Pp][256]"""
    Pp = (P + 63) // 64 * 64
    Y = sv.view(torch.float32)[512 + Pp * 64: 512 + Pp * 64 + 8 * Pp * 256].view(8, Pp, 256)[:, :P]
    return [Y[i] > 0 for i in range(8)]


# ---- the restatement on given ReLU decisions --------------------------------------------------------------------------------
def _masked_forward(net, x, t, masks=None, pre=None):
    """``net.reference_forward`` in net's dtype, with ``relu`` replaced by the given decisions (None: its own).  ``pre``: a list that
    receives every layer's pre-activation"""
    from sk_gs_amd.deform_net import freq_encode_torch
    t_emb = freq_encode_torch(t.view(-1, 1), net.t_degree).expand(x.shape[0], net.t_dim)
    if net.is_blender:
        t_emb = net.timenet(t_emb)
    x_emb = freq_encode_torch(x, net.p_degree)
    h = torch.cat([x_emb, t_emb], dim=-1)
    for i, layer in enumerate(net.linear):
        z = layer(h)
        if pre is not None:
            pre.append(z.detach())
        h = F.relu(z) if masks is None else z * masks[i].to(z.dtype)
        if i in net.skips:
            h = torch.cat([x_emb, t_emb, h], -1)
    out = dict(d_xyz=net.gaussian_warp(h), d_rotation=net.gaussian_rotation(h), d_scaling=net.gaussian_scaling(h))
    if net.sep_rot:
        out['g_rotation'] = net.local_rotation(h)
    return out


def _check_masks(masks, pre64):
    """the kernel's decisions equal fp64's except where fp64's pre-activation is within rounding of 0"""
    flips = 0
    for m, z in zip(masks, pre64):
        diff = m != (z > 0)
        n = int(diff.sum())
        if n:
            tol = 1e-5 * float(z.abs().max())
            assert float(z[diff].abs().max()) <= tol, ('a ReLU decision differs away from a tie', float(z[diff].abs().max()), tol)
            flips += n
    return flips


def _grads_on(net, x, t, masks, cot, dtype):
    n = copy.deepcopy(net).to(dtype)
    out = _masked_forward(n, x.to(dtype), t.to(dtype), masks)
    loss = sum((out[k] * cot[k].to(dtype)).sum() for k in _keys(net))
    return list(torch.autograd.grad(loss, list(n.parameters())))


def _assert_grads(net, got, g64, g32, what=''):
    for (name, _), a, b, c in zip(net.named_parameters(), got, g64, g32):
        assert torch.isfinite(a).all(), (what, name)
        bound = max(1e-4, REF_ERR_FACTOR * rel_err(c, b))
        assert rel_err(a, b) <= bound, (what, name, rel_err(a, b), bound)


# ---- 1. forward parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('P', [4097, 65537, 100000])
def test_rows_forward_matches_fp64(P, variant):
    from sk_gs_amd.superpoint import _SpNetRowsFn
    net = _net(variant, seed=P % 97)
    x, t = _points(P, P), torch.tensor([0.4375], device='cuda')
    with torch.no_grad():
        got = torch.cat(_SpNetRowsFn.apply(net, False, x, t, *net.parameters()), 1)
        want = _raw_of(copy.deepcopy(net).double().reference_forward(x.double(), t.double()), net)
    assert got.shape == want.shape and torch.isfinite(got).all()
    assert rel_err(got, want) <= 1e-4, rel_err(got, want)


# ---- 2. gradient parity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['blender', 'raw10', 'sep_rot'])
def test_rows_gradients_match_fp64_autograd(variant):
    P = 100000
    net = _net(variant, seed=7)
    x, t = _points(P, 11), torch.tensor([0.3], device='cuda')
    rc, raw, sv = _abi_forward(net, x, t)
    assert rc == 0
    masks = _kernel_masks(sv, P)
    pre64 = []
    with torch.no_grad():
        ref64 = _masked_forward(copy.deepcopy(net).double(), x.double(), t.double(), pre=pre64)
    assert rel_err(raw, _raw_of(ref64, net)) <= 1e-4
    _check_masks(masks, pre64)
    del pre64, ref64
    g = torch.Generator().manual_seed(3)
    cot = {k: torch.randn(P, 4 if 'rot' in k else 3, generator=g).cuda() for k in _keys(net)}
    got = _abi_backward(net, _raw_of(cot, net).contiguous(), sv)
    g64 = _grads_on(net, x, t, masks, cot, torch.float64)
    g32 = _grads_on(net, x, t, masks, cot, torch.float32)
    _assert_grads(net, got, g64, g32, variant)
    # and through the autograd operator (its own buffers): the same bits as the C ABI
    from sk_gs_amd.superpoint import _SpNetRowsFn
    params = list(net.parameters())
    outs = _SpNetRowsFn.apply(net, True, x, t, *params)
    via_fn = torch.autograd.grad(list(outs), params, [cot[k] for k in _keys(net)])
    for a, b in zip(via_fn, got):
        assert torch.equal(a, b)


# ---- 3. determinism ---------------------------------------------------------------------------------------------------------
def test_rows_forward_and_backward_are_bit_identical_when_repeated():
    P = 65537
    net = _net('blender', seed=5)
    x, t = _points(P, 5), torch.tensor([0.71], device='cuda')
    rc1, raw1, sv1 = _abi_forward(net, x, t)
    rc2, raw2, sv2 = _abi_forward(net, x, t)
    assert rc1 == 0 and rc2 == 0 and torch.equal(raw1, raw2) and torch.equal(sv1, sv2)
    g_raw = torch.randn(P, 10, generator=torch.Generator().manual_seed(9)).cuda()
    ga = _abi_backward(net, g_raw, sv1)
    gb = _abi_backward(net, g_raw, sv1)
    for a, b in zip(ga, gb):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- 4. the init iteration's pattern ----------------------------------------------------------------------------------------
def test_init_iteration_pattern_keeps_each_calls_state():
    """init_stage (sk_gs.py:741-749) and the c_net loss (:1501-1508): a(x, t) with grad, a(x, tc) under no_grad, b(a's output + x, t)
    with grad, one backward over both.  Each autograd node owns its buffers: the interleaved no-grad call does not disturb a's"""
    P = 65537
    a, b = _net('blender', seed=21), _net('blender', seed=22)
    x = _points(P, 23)
    t, tc = torch.tensor([0.25], device='cuda'), torch.tensor([0.0], device='cuda')
    g = torch.Generator().manual_seed(4)
    cot_a = {k: torch.randn(P, 4 if 'rot' in k else 3, generator=g).cuda() for k in _keys(a)}
    cot_b = {k: torch.randn(P, 4 if 'rot' in k else 3, generator=g).cuda() for k in _keys(b)}
    for p in list(a.parameters()) + list(b.parameters()):
        p.grad = None
    out = a(x, t)
    with torch.no_grad():
        xc = a(x, tc)['d_xyz'] + x
    out_b = b(xc, t)
    loss = sum((out[k] * cot_a[k]).sum() for k in _keys(a)) + sum((out_b[k] * cot_b[k]).sum() for k in _keys(b))
    loss.backward()
    # the fp64 sequence on the kernel's decisions (the same calls through the C ABI: same inputs, same bits)
    with torch.no_grad():
        want_xc = copy.deepcopy(a).double().reference_forward(x.double(), tc.double())['d_xyz'] + x.double()
    assert rel_err(xc, want_xc) <= 1e-4
    for net, xin, cot in ((a, x, cot_a), (b, xc, cot_b)):
        rc, raw, sv = _abi_forward(net, xin, t)
        assert rc == 0
        masks = _kernel_masks(sv, P)
        pre64 = []
        with torch.no_grad():
            _masked_forward(copy.deepcopy(net).double(), xin.double(), t.double(), pre=pre64)
        _check_masks(masks, pre64)
        del pre64
        g64 = _grads_on(net, xin, t, masks, cot, torch.float64)
        g32 = _grads_on(net, xin, t, masks, cot, torch.float32)
        _assert_grads(net, [p.grad for p in net.parameters()], g64, g32, 'a' if net is a else 'b')


# ---- 5. routing of the reference hook ---------------------------------------------------------------------------------------
def test_reference_hook_routes_p_row_calls_to_the_row_kernels():
    from benchlib import ref_sequence as rs
    from sk_gs_amd import reference_accel as ra
    from sk_gs_amd.superpoint import SpDeformNet
    torch.manual_seed(31)
    ref = SpDeformNet()
    ref.pos_enc_p, ref.pos_enc_t, ref.max_d_scale = rs.RefFreqEncoder(3, 10), rs.RefFreqEncoder(1, 6), -1.0
    with torch.no_grad():
        for h in (ref.gaussian_warp, ref.gaussian_rotation, ref.gaussian_scaling):
            h.weight.normal_(0, 0.05)
    ref = ref.cuda()
    had = 'sp_net' in ra._originals
    saved_orig = ra._originals.get('sp_net')
    ra._originals['sp_net'] = lambda self, x, t, **kw: self.reference_forward(x, t)
    try:
        t = torch.tensor([0.5], device='cuda')
        x = _points(100000, 32)
        before = dict(ra.calls)
        out = ra.deform_network_forward(ref, x, t)
        assert ra.calls['sp_net_rows_fused'] == before['sp_net_rows_fused'] + 1
        assert ra.calls['sp_net_reference'] == before['sp_net_reference']
        with torch.no_grad():
            want = copy.deepcopy(ref).double().reference_forward(x.double(), t.double())
        assert set(out) == set(_keys(ref)) and all(rel_err(out[k], want[k]) <= 1e-4 for k in _keys(ref))
        # gradients reach the reference module's own parameters
        loss = sum(out[k].sum() for k in _keys(ref))
        grads = torch.autograd.grad(loss, list(ref.parameters()))
        assert all(torch.isfinite(gr).all() for gr in grads)
        # x that requires a gradient, and one time per row: the reference's forward
        n_ref = ra.calls['sp_net_reference']
        ra.deform_network_forward(ref, x.clone().requires_grad_(), t)
        ra.deform_network_forward(ref, x, torch.full((x.shape[0], 1), 0.5, device='cuda'))
        assert ra.calls['sp_net_reference'] == n_ref + 2
        assert ra.calls['sp_net_rows_fused'] == before['sp_net_rows_fused'] + 1
        # the superpoint-sized call keeps its kernels
        n_small = ra.calls['sp_net_fused']
        ra.deform_network_forward(ref, x[:512].contiguous(), t)
        assert ra.calls['sp_net_fused'] == n_small + 1 and ra.calls['sp_net_rows_fused'] == before['sp_net_rows_fused'] + 1
    finally:
        if had:
            ra._originals['sp_net'] = saved_orig
        else:
            ra._originals.pop('sp_net', None)


# ---- 6. memory of a no-grad call --------------------------------------------------------------------------------------------
def test_no_grad_forward_allocates_only_its_outputs():
    P = 100000
    net = _net('blender', seed=41)
    x, t = _points(P, 42), torch.tensor([0.6], device='cuda')
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        out = net(x, t)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak <= P * 10 * 4 + 16 * 2 ** 20, peak
    assert out['d_xyz'].shape == (P, 3) and torch.isfinite(out['d_xyz']).all()


# ---- 7. the C ABI's edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [1, 7])
def test_abi_tiny_row_counts_match_fp64(P):
    net = _net('sep_rot', seed=P)
    x, t = _points(P, 50 + P), torch.tensor([0.2], device='cuda')
    rc, raw, sv = _abi_forward(net, x, t)
    assert rc == 0
    with torch.no_grad():
        want = _raw_of(copy.deepcopy(net).double().reference_forward(x.double(), t.double()), net)
    assert rel_err(raw, want) <= 1e-4
    cot = {k: torch.randn(P, 4 if 'rot' in k else 3, generator=torch.Generator().manual_seed(P)).cuda() for k in _keys(net)}
    got = _abi_backward(net, _raw_of(cot, net).contiguous(), sv)
    masks = _kernel_masks(sv, P)
    _assert_grads(net, got, _grads_on(net, x, t, masks, cot, torch.float64), _grads_on(net, x, t, masks, cot, torch.float32), P)


def test_abi_refuses_bad_calls():
    from sk_gs_amd import _C
    from sk_gs_amd.superpoint import _net_desc
    lib = _lib()
    net = _net('blender', seed=1)
    x, t = _points(64, 1), torch.tensor([0.2], device='cuda')
    raw = torch.zeros(64, 10, device='cuda')
    assert lib.skgs_sp_net_rows_saved_bytes(C.c_int32(0)) == 0 and lib.skgs_sp_net_rows_workspace_bytes(C.c_int32(-3)) == 0
    for P, flags in ((0, 0), (-5, 0), (64, 1)):   # P <= 0; SKGS_SP_NET_LBS_C
        d = _net_desc(net, 64, x, t)
        d.M, d.flags = P, flags
        assert lib.skgs_sp_net_rows_forward(C.byref(d), C.c_void_p(raw.data_ptr()), None, C.c_size_t(0), _C._stream()) != 0
    d = _net_desc(net, 64, x, t)
    small = torch.empty(1024, dtype=torch.uint8, device='cuda')
    assert lib.skgs_sp_net_rows_forward(C.byref(d), C.c_void_p(raw.data_ptr()), C.c_void_p(small.data_ptr()), C.c_size_t(1024),
                                        _C._stream()) != 0
    dg = _net_desc(net, 64, None, None)
    for P, flags in ((0, 0), (64, 1)):
        d = _net_desc(net, 64, x, t)
        d.M, d.flags = P, flags
        assert lib.skgs_sp_net_rows_backward(C.byref(d), C.byref(dg), C.c_void_p(raw.data_ptr()), C.c_void_p(small.data_ptr()),
                                             C.c_size_t(1 << 30), C.c_void_p(small.data_ptr()), C.c_size_t(1 << 30), _C._stream()) != 0
    torch.cuda.synchronize()
    assert torch.all(raw == 0)
