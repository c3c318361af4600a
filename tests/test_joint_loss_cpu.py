"""The joint-discovery patch without a GPU (sk_gs_amd/joint_loss.py): ``accelerate_reference(joint_loss=True)`` patches exactly
``loss_joint_discovery`` and the module global ``joint_discovery`` and ``restore_reference()`` undoes both; on CPU tensors the patched
method is the reference's own (same values); the host tree rebuild gives the reference's edge set and, where the tree has one centre,
its parents, depth and root (else a root that is a centre).  The reference parts run in a child process, as
tests/test_sp_fix_route_cpu.py does, and are skipped where the reference checkout is absent."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REFERENCE = '/root/reference'
sys.path.insert(0, ROOT)

_SCRIPT = r"""
import sys, warnings
sys.dont_write_bytecode = True
sys.path[:0] = [{root!r}, {golden!r}, {ref!r}]
import make_golden
make_golden.STUBS = make_golden.STUBS - {{'lietorch', 'pytorch3d', 'diff_gaussian_rasterization'}}
sys.meta_path.insert(0, make_golden._Finder())
import sk_gs_amd
sk_gs_amd.install_reference_hooks()
warnings.simplefilter('ignore')
import numpy as np, torch
import networks.sk_gs as sk
from sk_gs_amd import reference_accel as ra, joint_loss as jl
S = sk.SkeletonGaussianSplatting
orig_loss, orig_disc = S.loss_joint_discovery, sk.joint_discovery
base = sorted(sk_gs_amd.accelerate_reference(adam=False))
assert S.loss_joint_discovery is orig_loss and sk.joint_discovery is orig_disc     # opt-in: not patched by default
ra.restore_reference()
extra = sorted(set(sk_gs_amd.accelerate_reference(adam=False, joint_loss=True)) - set(base))
assert extra == ['networks.sk_gs.SkeletonGaussianSplatting.loss_joint_discovery', 'networks.sk_gs.joint_discovery'], extra
assert S.loss_joint_discovery is jl.loss_joint_discovery and sk.joint_discovery is jl.joint_discovery
assert ra._originals['joint_loss'] is orig_loss and ra._originals['joint_discovery'] is orig_disc

# on CPU tensors the patched method is the reference's own: the same values as the unpatched method on the same state
NET = dict(pos_enc_p='freq_torch', pos_enc_p_cfg={{'degree': 2}}, pos_enc_t='freq_torch', pos_enc_t_cfg={{'degree': 2}}, width=16, depth=2, skips=[])
M = 20
m = S(sh_degree=3, net_cfg=NET, sk_deform_net_cfg=NET, hyper_dim=8, is_blender=True, train_schedule={{'sp': 10, 'sk': 10}}, num_superpoints=M,
      num_knn=3, LBS_method='W', warp_method='LBS', sep_rot=False, sk_knn_num=3)
m.train()
g = torch.Generator().manual_seed(3)
m.sp_points = torch.nn.Parameter(torch.randn(M, 3, generator=g))
m.joint_pos = torch.nn.Parameter(torch.randn(M, M, 3, generator=g))
m.joint_cost = torch.rand(M, M, generator=g)
m.joint_is_init = torch.tensor(True)
spT = torch.cat([torch.randn(M, 3, generator=g) * 0.3, torch.randn(M, 4, generator=g) * 0.1 + torch.tensor([0, 0, 0, 1.])], -1)
cost0 = m.joint_cost.clone()
res = []
for f in (orig_loss, S.loss_joint_discovery):
    m.joint_cost, m._joint_pair = cost0.clone(), None
    best, all_ = f(m, spT, None, True)
    res.append((float(best), float(all_), m.joint_cost.clone(), m.joint_parents.clone()))
assert jl.calls['joint_loss_reference'] == 1 and jl.calls['joint_loss_fused'] == 0, jl.calls
assert res[0][:2] == res[1][:2] and torch.equal(res[0][2], res[1][2]), (res[0][:2], res[1][:2])

# the tree rebuild against the reference's own function, plain and in the masked form update_joint builds
ref_disc = orig_disc


def edges(parents, root):
    p = np.asarray(parents)[:, 0]
    return sorted(tuple(sorted((a, int(p[a])))) for a in range(len(p)) if a != root)


def centres(edge_list, M):
    adj = [[] for _ in range(M)]
    for a, b in edge_list:
        adj[a].append(b), adj[b].append(a)
    ecc = []
    for s in range(M):
        d = [-1] * M
        d[s], q = 0, [s]
        for u in q:
            for v in adj[u]:
                if d[v] < 0:
                    d[v] = d[u] + 1
                    q.append(v)
        ecc.append(max(d))
    return [i for i in range(M) if ecc[i] == min(ecc)]


seen = []
for M in (3, 17, 128, 512):
    g = torch.Generator().manual_seed(M)
    plain = torch.rand(M, M, generator=g)
    costs = [plain]
    # the masked form: what update_joint hands to joint_discovery (non-neighbours raised by max + 1)
    m2 = S(sh_degree=3, net_cfg=NET, sk_deform_net_cfg=NET, hyper_dim=8, is_blender=True, train_schedule={{'sp': 10, 'sk': 10}}, num_superpoints=M,
           num_knn=3, LBS_method='W', warp_method='LBS', sep_rot=False, sk_knn_num=3)
    m2.sp_points = torch.nn.Parameter(torch.randn(M, 3, generator=g))
    m2.joint_cost = torch.rand(M, M, generator=g)
    captured = []
    sk.joint_discovery = lambda c: captured.append(c.clone()) or ref_disc(c)
    try:
        m2.update_joint(verbose=False)
    finally:
        sk.joint_discovery = jl.joint_discovery
    costs.append(captured[0])
    for cost in costs:
        rp, rd, rr = ref_disc(cost)
        op, od, orr = jl.joint_discovery(cost)
        assert op.dtype == torch.int32 and od.dtype == torch.int32 and isinstance(orr, int)
        e_ref, e_our = edges(rp, rr), edges(op, orr)
        assert e_ref == e_our, M
        c = centres(e_ref, M)
        if len(c) == 1:
            assert orr == rr and np.array_equal(op.numpy(), rp.numpy().astype(np.int32)) and np.array_equal(od.numpy(), rd.numpy()), M
        else:
            assert orr in c and op.shape == rp.shape, (M, c, orr)
        seen.append(len(c))
assert jl.calls['joint_discovery_fused'] == 2 + 8, jl.calls     # (the two update_joint calls of the fall-through check above, too)
ra.restore_reference()
assert S.loss_joint_discovery is orig_loss and sk.joint_discovery is orig_disc and 'joint_loss' not in ra._originals
print('JOINT-LOSS-CPU-OK', seen)
"""


@pytest.mark.skipif(not os.path.isdir(_REFERENCE), reason='the reference is only mounted in the build container')
def test_patch_fallthrough_and_tree_rebuild_against_the_reference():
    code = _SCRIPT.format(root=ROOT, golden=os.path.join(ROOT, 'tests', 'golden'), ref=_REFERENCE)
    env = {k: v for k, v in os.environ.items() if k != 'PYTHONPATH'}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd='/tmp', env=env, timeout=900)
    assert r.returncode == 0 and 'JOINT-LOSS-CPU-OK' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_discovery_host_path_and_star():
    """no reference needed: a path 0-1-2-3-4 (one centre, 2) and a star around 3, from cost matrices whose cheapest entries are those
    edges; ties go to the lower flat index"""
    from sk_gs_amd.joint_loss import discovery_host
    M = 5
    cost = np.full((M, M), 10.0, dtype=np.float32)
    for a in range(M - 1):
        cost[a + 1, a] = 1.0 + a
    parents, depth, root = discovery_host(cost)
    assert root == 2 and parents.shape == (5, 2)        # peeling depth 3 (leaves 1, their neighbours 2, the centre 3): 2^L >= 3
    assert list(parents[:, 0]) == [1, 2, 2, 2, 3] and list(depth) == [2, 1, 0, 1, 2]
    star = np.full((M, M), 5.0, dtype=np.float32)
    star[3, :] = 1.0                                    # ties: row 3 in flat-index order -> edges (0,3), (1,3), (2,3), (4,3)
    parents, depth, root = discovery_host(star)
    assert root == 3 and list(parents[:, 0]) == [3, 3, 3, 3, 3] and list(depth) == [1, 1, 1, 0, 1]


@pytest.mark.skipif(not os.path.isdir(_REFERENCE), reason='the reference is only mounted in the build container')
def test_golden_fixture_reproduces():
    env = {k: v for k, v in os.environ.items() if k != 'PYTHONPATH'}
    env['PYTHONDONTWRITEBYTECODE'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'golden', 'make_golden_joint.py'), '--check'], capture_output=True, text=True,
                       cwd='/tmp', env=env, timeout=600)
    assert r.returncode == 0 and 'reproduced' in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
