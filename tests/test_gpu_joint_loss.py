"""Stage sp's joint-discovery loss through sk_gs_amd/joint_loss.py (csrc/joint_loss.hip) against the golden fixture of the reference's own
``loss_joint_discovery`` / ``update_joint`` (tests/golden/joint_loss.npz, made by make_golden_joint.py) and against the reference's torch
lines restated in fp64 on the device.  The model here restates the attributes and the three methods of ``SkeletonGaussianSplatting`` the
loss touches (init_joint_pos :859-865, update_joint :1245-1265, joint_pair :1267-1275); the loss itself is the patched method."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'joint_loss.npz')
DEV = torch.device('cuda:0')


class JointModel(torch.nn.Module):
    """what loss_joint_discovery reads and calls on the reference's model (networks/sk_gs.py), restated"""

    def __init__(self, M, canonical_time_id=0, sp_guided_detach=True, sk_momentum=0.9, sk_knn_num=3):
        super().__init__()
        self.num_superpoints, self.canonical_time_id, self.sp_guided_detach = M, canonical_time_id, sp_guided_detach
        self.sk_momentum, self.sk_knn_num, self.hyper_dim = sk_momentum, sk_knn_num, 0
        self.sp_points = torch.nn.Parameter(torch.zeros(M, 3))
        self.joint_pos = torch.nn.Parameter(torch.zeros(M, M, 3))
        self.register_buffer('joint_is_init', torch.tensor(True))
        self.register_buffer('joint_cost', torch.zeros(M, M))
        self.register_buffer('joint_parents', torch.full((M, 1), -1, dtype=torch.int32))
        self.register_buffer('joint_depth', torch.zeros(M, dtype=torch.int32))
        self.register_buffer('joint_root', torch.arange(M, dtype=torch.int32))
        self._joint_pair = None

    @torch.no_grad()
    def init_joint_pos(self, force=False):
        if self.joint_is_init and not force:
            return
        self.joint_is_init = self.joint_is_init.new_tensor(True)
        sp_points = self.sp_points[..., :3]
        self.joint_pos.data.copy_((sp_points[:, None] + sp_points[None, :]) * 0.5)

    @torch.no_grad()
    def update_joint(self, verbose=True, use_hyper=False):
        from sk_gs_amd import joint_loss as jl
        cost = self.joint_cost.clone()
        sp_dist = torch.cdist(self.sp_points, self.sp_points)
        knn_dist, _ = torch.kthvalue(sp_dist, min(self.num_superpoints, self.sk_knn_num + 1), dim=-1, keepdim=True)
        cost[sp_dist > knn_dist] += cost.max().abs() + 1
        self.joint_parents, self.joint_depth, root = jl.joint_discovery(cost)
        self.joint_root = self.joint_depth.new_tensor(root)
        self._joint_pair = None
        self._joint_pair = self.joint_pair

    @property
    def joint_pair(self):
        if self._joint_pair is None:
            mask = torch.ones_like(self.joint_parents[:, 0], dtype=torch.bool)
            mask[self.joint_root] = 0
            a = torch.arange(self.num_superpoints, device=self.joint_parents.device)[mask]
            b = self.joint_parents[mask, 0]
            self._joint_pair = (a, b, mask)
        return self._joint_pair


def loss(model, spT, update_joint):
    from sk_gs_amd import joint_loss as jl
    jl._originals.setdefault('loss', _no_fallback)
    return jl.loss_joint_discovery(model, spT, None, update_joint)


def _no_fallback(*args, **kwargs):
    raise AssertionError('the call left the fast path')


def eager(spT, jp, canonical_time_id, a, b):
    """the reference's lines (sk_gs.py:1313-1335, quaternion_to_Rt rigid.py:110-130, apply xfm.py:60-79), restated"""
    t, (x, y, z, w) = spT[:, :3], spT[:, 3:].unbind(-1)
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    T = torch.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z, t[:, 0],
                     2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x, t[:, 1],
                     2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, 1 - 2 * x * x - 2 * y * y, t[:, 2],
                     zero, zero, zero, one], dim=-1).reshape(-1, 4, 4)

    def apply(p, m):
        if p.shape[-1] + 1 == m.shape[-1]:
            p = torch.constant_pad_nd(p, (0, 1), 1.0)
        return torch.sum(m * p[..., None, :], dim=-1)[..., :3]

    if canonical_time_id < 0:
        Tab = torch.inverse(T[None, :]) @ T[:, None]
        d1 = Tab[..., :3, 3] - (jp - apply(jp, Tab[..., :3, :3]))
    else:
        d1 = apply(jp, T[None, :]) - apply(jp, T[:, None, :3, :3]) - T[:, None, :3, 3]
    jd = d1.norm(dim=-1)
    jpt = apply(jp, T)
    jd = jd + (jpt - jpt.transpose(0, 1)).norm(dim=-1)
    return ((jd[a, b] + jd[b, a]) * 0.5).mean(), jd.mean(), jd


def _model_from_fixture(z, name):
    g = lambda k: torch.from_numpy(np.asarray(z[f'{name}/in/{k}']))  # noqa: E731
    M = g('spT').shape[0]
    m = JointModel(M, int(g('canonical_time_id')), bool(g('sp_guided_detach')), float(g('sk_momentum')), int(g('sk_knn_num'))).to(DEV)
    with torch.no_grad():
        m.sp_points.copy_(g('sp_points'))
        m.joint_pos.copy_(g('joint_pos'))
    m.joint_cost = g('joint_cost').to(DEV)
    m.joint_is_init = torch.tensor(bool(g('joint_is_init')), device=DEV)
    m.joint_parents, m.joint_root = g('parents').to(DEV), torch.tensor(int(g('root')), dtype=torch.int32, device=DEV)
    m.joint_pair     # (the pair list of the tree before the call, as the reference holds it)
    m.train()
    return m, g('spT').to(DEV), bool(g('update_joint'))


def _edges(parents, root):
    p = parents[:, 0].tolist()
    return sorted(tuple(sorted((i, p[i]))) for i in range(len(p)) if i != root)


def _rel(x, ref):
    return float((x.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize('name', ['m48_c0_detach', 'm48_cneg_grad', 'm37_c0_grad_update', 'm37_cneg_detach_init'])
def test_fixture(name):
    from sk_gs_amd import joint_loss as jl
    z = np.load(GOLDEN)
    for w1, w2 in ((1.0, 1.0), (0.7, 0.0)):
        m, spT, upd = _model_from_fixture(z, name)
        T = spT.clone().requires_grad_(not m.sp_guided_detach)
        n0 = jl.calls['joint_loss_fused']
        best, all_ = loss(m, T, upd)
        assert jl.calls['joint_loss_fused'] == n0 + 1
        (w1 * best + w2 * all_).backward()
        out = lambda k: torch.from_numpy(np.asarray(z[f'{name}/out/{k}']))  # noqa: E731
        assert abs(float(best) - float(out('best'))) <= 1e-5 * abs(float(out('best'))), (float(best), float(out('best')))
        assert abs(float(all_) - float(out('all'))) <= 1e-5 * abs(float(out('all'))), (float(all_), float(out('all')))
        assert _rel(m.joint_cost.cpu(), out('joint_cost')) < 1e-5
        assert torch.equal(m.joint_pos.detach().cpu(), out('joint_pos'))
        assert bool(m.joint_is_init)
        ref_par, ref_root = out('parents').numpy(), int(out('root'))
        our_par, our_root = m.joint_parents.cpu().numpy(), int(m.joint_root)
        assert _edges(our_par, our_root) == _edges(ref_par, ref_root)
        if not upd:
            assert np.array_equal(our_par, ref_par) and our_root == ref_root
        key = f'{name}/grad_{w1:g}_{w2:g}'
        e = _rel(m.joint_pos.grad.cpu(), torch.from_numpy(z[f'{key}/joint_pos']))
        assert e < 1e-5, e
        if not m.sp_guided_detach:
            e = _rel(T.grad.cpu(), torch.from_numpy(z[f'{key}/spT']))
            assert e < 1e-5, e
        else:
            assert T.grad is None


def _random_model(M, ct, detach, seed):
    g = torch.Generator().manual_seed(seed)
    m = JointModel(M, ct, detach).to(DEV)
    with torch.no_grad():
        m.sp_points.copy_(torch.randn(M, 3, generator=g))
        m.joint_pos.copy_(torch.randn(M, M, 3, generator=g) * 0.5)
    m.joint_cost = torch.rand(M, M, generator=g).to(DEV)
    m.update_joint()
    m.train()
    spT = torch.cat([torch.randn(M, 3, generator=g) * 0.3, torch.randn(M, 4, generator=g) * 0.15 + torch.tensor([0, 0, 0, 1.])], -1).to(DEV)
    return m, spT


@pytest.mark.parametrize('M', [512, 1000])
@pytest.mark.parametrize('ct', [0, -1])
def test_against_fp64_restatement(M, ct):
    m, spT = _random_model(M, ct, False, M + 7 * (ct + 2))
    cost0 = m.joint_cost.clone()
    T = spT.clone().requires_grad_()
    best, all_ = loss(m, T, False)
    (best + 0.5 * all_).backward()
    a, b, _ = m.joint_pair
    T64 = spT.double().requires_grad_()
    jp64 = m.joint_pos.detach().double().requires_grad_()
    rb, ra, rjd = eager(T64, jp64, ct, a, b)
    (rb + 0.5 * ra).backward()
    assert abs(float(best) - float(rb)) <= 1e-5 * abs(float(rb)) and abs(float(all_) - float(ra)) <= 1e-5 * abs(float(ra))
    assert _rel(m.joint_cost, cost0.double() * 0.9 + rjd.detach() * (1 - 0.9)) < 1e-5
    assert _rel(m.joint_pos.grad, jp64.grad) < 1e-5, _rel(m.joint_pos.grad, jp64.grad)
    assert _rel(T.grad, T64.grad) < 1e-5, _rel(T.grad, T64.grad)


def test_bitwise_and_no_host_sync():
    m, spT = _random_model(512, 0, False, 11)
    cost0 = m.joint_cost.clone()
    res = []
    for _ in range(2):
        m.joint_cost = cost0.clone()
        m.joint_pos.grad = None
        T = spT.clone().requires_grad_()
        best, all_ = loss(m, T, False)
        (best + all_).backward()
        res.append((best.detach().clone(), all_.detach().clone(), m.joint_cost.clone(), m.joint_pos.grad.clone(), T.grad.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    # a call with no tree update: no host synchronisation, forward or backward
    m.joint_pos.grad = None
    T = spT.clone().requires_grad_()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        best, all_ = loss(m, T, False)
        (best + all_).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.equal(T.grad, res[0][4])


def test_update_joint_uses_the_new_edges():
    from sk_gs_amd import joint_loss as jl
    m, spT = _random_model(200, 0, True, 5)
    old = m.joint_pair
    m.joint_cost = torch.rand(200, 200, device=DEV)        # a different cost: the rebuilt tree differs from the current one
    n0 = jl.calls['joint_discovery_fused']
    best, all_ = loss(m, spT, True)
    assert jl.calls['joint_discovery_fused'] == n0 + 1
    a, b, _ = m.joint_pair
    assert m.joint_pair is not old and not (torch.equal(old[0], a) and torch.equal(old[1], b))
    rb, ra, _ = eager(spT.double(), m.joint_pos.detach().double(), 0, a, b)
    ob, _, _ = eager(spT.double(), m.joint_pos.detach().double(), 0, old[0], old[1])
    assert abs(float(best) - float(rb)) <= 1e-5 * abs(float(rb)) and abs(float(rb) - float(ob)) > 1e-4


@pytest.mark.parametrize('which', ['best', 'all', 'both'])
def test_cotangent_on_either_output(which):
    m, spT = _random_model(96, -1, False, 21)
    T = spT.clone().requires_grad_()
    best, all_ = loss(m, T, False)
    {'best': best, 'all': all_, 'both': 0.3 * best + 2.0 * all_}[which].backward()
    a, b, _ = m.joint_pair
    T64, jp64 = spT.double().requires_grad_(), m.joint_pos.detach().double().requires_grad_()
    rb, ra, _ = eager(T64, jp64, -1, a, b)
    {'best': rb, 'all': ra, 'both': 0.3 * rb + 2.0 * ra}[which].backward()
    assert _rel(m.joint_pos.grad, jp64.grad) < 1e-5 and _rel(T.grad, T64.grad) < 1e-5
