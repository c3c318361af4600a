"""Stages init_fix / init on the fused route, without a GPU: the reference's REAL ``SkeletonGaussianSplatting`` built from the shipped
YAML (exps/default.yaml) passes every condition of ``reference_fused._conditions_init`` but the device one, a replaced ``_xyz`` changes the
route's light identity (densification rebuilds the route), and ``render`` hands the call to the reference's own method with a reason that
names the stage.  Runs in a child process, as tests/test_host_cpu.py does; skipped where the reference checkout is absent."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REFERENCE = '/root/reference'

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
import yaml, torch
from torch import nn
import networks.sk_gs as sk
from sk_gs_amd import reference_accel as ra, reference_fused as rf
sk_gs_amd.accelerate_reference()
m = sk.SkeletonGaussianSplatting(**yaml.safe_load(open({ref!r} + '/exps/default.yaml'))['arch_cfg'])
g = torch.Generator().manual_seed(0)
P = 300
for name, shape in (('_xyz', (P, 3)), ('_features_dc', (P, 1, 3)), ('_features_rest', (P, 15, 3)), ('_scaling', (P, 3)), ('_rotation', (P, 4)),
                    ('_opacity', (P, 1))):
    setattr(m, name, nn.Parameter(torch.randn(*shape, generator=g)))
assert m.sp_deform_net.is_blender and float(m.loss_funcs.w('p_arap_ct_init')) == 0.0
# every condition but the device one holds (the device test is the last one)
assert rf._conditions_init(m) == 'parameters are not on a HIP device', rf._conditions_init(m)
m.convert_SHs_python = True
assert 'convert_SHs_python' in rf._conditions_init(m)
m.convert_SHs_python = False
view = rf._ModelViewInit(m, ra.sp_net_shadow(m.sp_deform_net), 'init')
heads = {{id(q) for mod in (m.sp_deform_net.gaussian_rotation, m.sp_deform_net.gaussian_scaling) for q in mod.parameters()}}
assert len(view.parameters()) == 6 + len(list(m.sp_deform_net.parameters())) - len(heads) and not any(id(q) in heads for q in view.parameters())
assert len(rf._ModelViewInit(m, ra.sp_net_shadow(m.sp_deform_net), 'init_fix').parameters()) == 6
# densification replaces _xyz: the light identity changes, so the next call rebuilds the route
before = rf._light_identity(m, 'init')
assert rf._light_identity(m, 'init') == before
m._xyz = nn.Parameter(m._xyz.detach().clone())
assert rf._light_identity(m, 'init') != before
# render: the reference's own method, the reason names the stage
seen = []
ra._originals['render'] = lambda self, *a, **kw: seen.append(kw) or 'the reference render'
m.train()
info = dict(Tw2v=torch.eye(4)[None], Tv2c=torch.eye(4)[None], campos=torch.zeros(1, 3), FoV=torch.tensor([[0.7, 0.7]]), size=(64, 48))
for stage in ('init_fix', 'init'):
    assert m.render(t=torch.tensor([0.5]), info=info, time_id=torch.tensor([1]), stage=stage) == 'the reference render'
    assert seen[-1]['stage'] == stage and ("stage %r" % stage) in rf.why_not['render'] and rf.calls['render_fused'] == 0
print('INIT-ROUTE-OK')
"""


@pytest.mark.skipif(not os.path.isdir(_REFERENCE), reason='the reference is only mounted in the build container')
def test_real_model_in_stage_init_is_refused_only_for_the_device():
    code = _SCRIPT.format(root=ROOT, golden=os.path.join(ROOT, 'tests', 'golden'), ref=_REFERENCE)
    env = {k: v for k, v in os.environ.items() if k != 'PYTHONPATH'}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd='/tmp', env=env, timeout=600)
    assert r.returncode == 0 and 'INIT-ROUTE-OK' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
