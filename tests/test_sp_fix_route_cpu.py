"""Stage sp_fix on the fused route, without a GPU: the reference's REAL ``SkeletonGaussianSplatting`` built from the shipped YAML
(exps/default.yaml) in stage sp_fix is refused only for the device, with a reason that names the stage; the plain sp_fix backward attaches
exactly the six Gaussian tensors; sp_fix and sp share the light identity (one route).  Runs in a child process, as
tests/test_init_route_cpu.py does; skipped where the reference checkout is absent."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REFERENCE = '/root/reference'

_SCRIPT = r"""
import sys, types, warnings
sys.dont_write_bytecode = True
sys.path[:0] = [{root!r}, {golden!r}, {ref!r}]
import make_golden
make_golden.STUBS = make_golden.STUBS - {{'lietorch', 'pytorch3d', 'diff_gaussian_rasterization'}}
sys.meta_path.insert(0, make_golden._Finder())
import sk_gs_amd
sk_gs_amd.install_reference_hooks()
warnings.simplefilter('ignore')
import yaml, torch
from torch import nn
import networks.sk_gs as sk
from sk_gs_amd import reference_accel as ra, reference_fused as rf
sk_gs_amd.accelerate_reference()
cfg = yaml.safe_load(open({ref!r} + '/exps/default.yaml'))['arch_cfg']
m = sk.SkeletonGaussianSplatting(**cfg)
g = torch.Generator().manual_seed(0)
P, M = 300, 128
for name, shape in (('_xyz', (P, 3)), ('_features_dc', (P, 1, 3)), ('_features_rest', (P, 15, 3)), ('_scaling', (P, 3)), ('_rotation', (P, 4)),
                    ('_opacity', (P, 1))):
    setattr(m, name, nn.Parameter(torch.randn(*shape, generator=g)))
# what stage sp's initialisation leaves (sk_gs.py:583-602): superpoints, hyper features and, under LBS_method W, the dense logit table
m.sp_points = nn.Parameter(torch.randn(M, 3, generator=g))
if m.hyper_dim > 0:
    m.hyper_feature = nn.Parameter(torch.randn(P, m.hyper_dim, generator=g))
    m.sp_hyper_feature = nn.Parameter(torch.randn(M, m.hyper_dim, generator=g))
assert m.LBS_method == 'W', m.LBS_method
m.sp_W = nn.Parameter(torch.randn(P, M, generator=g))
assert rf._conditions_sp(m) == 'parameters are not contiguous fp32 tensors on a HIP device', rf._conditions_sp(m)
# ... and it is the device alone: with is_cuda answered True, every other condition holds
real = torch.Tensor.is_cuda
torch.Tensor.is_cuda = property(lambda self: True)
try:
    assert rf._conditions_sp(m) is None, rf._conditions_sp(m)
finally:
    torch.Tensor.is_cuda = real
# one route for both stages: the same light identity, the same key
assert rf._light_identity(m, rf._route_key('sp_fix')) == rf._light_identity(m, 'sp') and rf._route_key('sp_fix') == 'sp'
# the plain sp_fix backward attaches exactly the six Gaussian tensors (a route's attach lists, built on the view of the real model)
view = rf._ModelViewSp(m, ra.sp_net_shadow(m.sp_deform_net))
fake = types.SimpleNamespace(view=view, shadow=view.sp_deform_net, _attach=[(q, None, False) for q in view.parameters()])
lists = rf.FusedReferenceRoute._fix_attach_lists(fake)
six = [m._xyz, m._features_dc, m._features_rest, m._scaling, m._rotation, m._opacity]
assert [id(q) for q, _, _ in lists[(False, False)]] == [id(q) for q in six]
assert any(q is m.sp_W for q, _, _ in lists[(True, False)]) and not any(q is m.sp_W for q, _, _ in lists[(False, True)])
net = view.sp_deform_net
assert not any(q is net.gaussian_scaling.weight for q, _, _ in lists[(True, True)]) and any(q is net.gaussian_warp.weight for q, _, _ in lists[(False, True)])
# render: the reference's own method, the reason names the stage
seen = []
ra._originals['render'] = lambda self, *a, **kw: seen.append(kw) or 'the reference render'
m.train()
info = dict(Tw2v=torch.eye(4)[None], Tv2c=torch.eye(4)[None], campos=torch.zeros(1, 3), FoV=torch.tensor([[0.7, 0.7]]), size=(64, 48))
assert m.render(t=torch.tensor([0.5]), info=info, time_id=torch.tensor([1]), stage='sp_fix') == 'the reference render'
assert seen[-1]['stage'] == 'sp_fix' and "stage 'sp_fix'" in rf.why_not['render'] and rf.calls['render_fused'] == 0, rf.why_not
print('SP-FIX-ROUTE-OK')
"""


@pytest.mark.skipif(not os.path.isdir(_REFERENCE), reason='the reference is only mounted in the build container')
def test_real_model_in_stage_sp_fix_is_refused_only_for_the_device():
    code = _SCRIPT.format(root=ROOT, golden=os.path.join(ROOT, 'tests', 'golden'), ref=_REFERENCE)
    env = {k: v for k, v in os.environ.items() if k != 'PYTHONPATH'}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd='/tmp', env=env, timeout=600)
    assert r.returncode == 0 and 'SP-FIX-ROUTE-OK' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
