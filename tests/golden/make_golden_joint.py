#!/usr/bin/env python3
"""Golden fixture of the reference's JOINT-DISCOVERY loss, produced by running the UNMODIFIED ``networks/sk_gs.py`` on CPU.

Run in the build container only (needs /root/reference, read-only):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_joint.py            (--check: compare with the committed file instead)
Only ``joint_loss.npz`` travels.  Third-party modules this image lacks are the inert stubs of make_golden.py, except lietorch and
pytorch3d, which are this repository's stand-ins (the model's constructor imports them; the loss never calls them).

What runs is the reference's own class and methods: ``SkeletonGaussianSplatting(...)`` with M superpoints, its ``joint_pos`` /
``joint_cost`` / ``sp_points`` filled from a seeded generator, a tree from its own ``update_joint()`` (sk_gs.py:1245-1265 -> the Python
``joint_discovery`` :106-131, the function the reference runs where ``my_ext._C`` does not serve it), then
``loss_joint_discovery(spT, None, update_joint)`` (:1309-1336) in training mode and ``backward`` of ``w1 * best + w2 * all``.

Per scenario ``<name>/in/*``: spT [M, 7], joint_pos [M, M, 3], joint_cost [M, M], sp_points [M, 3], the tree before the call
(parents, root), the flags (canonical_time_id, sp_guided_detach, sk_momentum, sk_knn_num, update_joint, joint_is_init);
``<name>/out/*``: best, all, joint_cost (the EMA), joint_pos (after init_joint_pos), the tree after the call (parents, depth, root);
``<name>/grad_<w1>_<w2>/*``: the gradients of joint_pos and (sp_guided_detach false) spT.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (stub finder only)

REF = make_golden.REF
OUT = os.path.join(HERE, 'joint_loss.npz')

# name -> (M, canonical_time_id, sp_guided_detach, update_joint, joint_is_init)
SCENARIOS = {
    'm48_c0_detach': (48, 0, True, False, True),           # exps/default.yaml: canonical_time_id 0, sp_guided_detach true
    'm48_cneg_grad': (48, -1, False, False, True),         # the inverse branch, the gradient reaches spT
    'm37_c0_grad_update': (37, 0, False, True, True),      # not a tile multiple; the tree is rebuilt inside the call
    'm37_cneg_detach_init': (37, -1, True, False, False),  # joint_pos set to the superpoint midpoints by init_joint_pos
}
WEIGHTS = ((1.0, 1.0), (0.7, 0.0))
NET_CFG = dict(pos_enc_p='freq_torch', pos_enc_p_cfg={'degree': 4}, pos_enc_t='freq_torch', pos_enc_t_cfg={'degree': 2}, width=16,
               depth=2, skips=[])


def generate():
    assert os.path.isdir(REF), 'the reference is only mounted in the build container'
    sys.dont_write_bytecode = True
    make_golden.STUBS = make_golden.STUBS - {'lietorch', 'pytorch3d'}
    sys.meta_path.insert(0, make_golden._Finder())
    sys.path[:0] = [ROOT, REF]
    import warnings
    warnings.filterwarnings('ignore')
    import torch
    import sk_gs_amd
    sk_gs_amd.install_as_lietorch()
    sk_gs_amd.install_as_pytorch3d()
    import networks.sk_gs as sk                       # the reference, unmodified
    assert sk.__file__.startswith(REF)
    f32 = lambda t: t.detach().numpy().astype(np.float32)  # noqa: E731
    rec = {}
    for name, (M, ct, detach, upd, is_init) in SCENARIOS.items():
        g = torch.Generator().manual_seed(sum(map(ord, name)) * 104729)
        rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale  # noqa: E731
        model = sk.SkeletonGaussianSplatting(sh_degree=3, net_cfg=NET_CFG, sk_deform_net_cfg=NET_CFG, hyper_dim=8, is_blender=True,
                                             train_schedule={'sp': 10, 'sk': 10}, num_superpoints=M, num_knn=3, LBS_method='W',
                                             warp_method='LBS', sep_rot=False, sk_momentum=0.9, sk_knn_num=3)
        model.train()
        model.canonical_time_id, model.sp_guided_detach = ct, detach
        with torch.no_grad():
            model.sp_points = torch.nn.Parameter(rn(M, 3, scale=0.8))
            model.joint_pos = torch.nn.Parameter(rn(M, M, 3, scale=0.5))
            model.joint_cost = rn(M, M).abs()
            model.update_joint(verbose=False)          # a tree before the call (the reference's own discovery)
            model.joint_cost = rn(M, M).abs() * 0.5
            model.joint_is_init = torch.tensor(is_init)
        spT = torch.cat([rn(M, 3, scale=0.3), rn(M, 4, scale=0.15) + torch.tensor([0, 0, 0, 1.0])], dim=-1)   # q NOT normalised
        ins = dict(spT=f32(spT), joint_pos=f32(model.joint_pos), joint_cost=f32(model.joint_cost), sp_points=f32(model.sp_points),
                   parents=model.joint_parents.numpy().astype(np.int32), root=np.int64(int(model.joint_root)),
                   canonical_time_id=np.int64(ct), sp_guided_detach=np.bool_(detach), sk_momentum=np.float64(model.sk_momentum),
                   sk_knn_num=np.int64(model.sk_knn_num), update_joint=np.bool_(upd), joint_is_init=np.bool_(is_init))
        state = (model.joint_pos.detach().clone(), model.joint_cost.clone(), model.joint_parents.clone(), model.joint_depth.clone(),
                 model.joint_root.clone(), model._joint_pair, model.joint_is_init.clone())
        for w1, w2 in WEIGHTS:
            with torch.no_grad():
                model.joint_pos.data.copy_(state[0])
            model.joint_cost, model.joint_parents, model.joint_depth, model.joint_root = state[1], state[2], state[3], state[4]
            model._joint_pair, model.joint_is_init = state[5], state[6]
            model.joint_pos.grad = None
            T = spT.clone().requires_grad_(not detach)
            best, all_ = model.loss_joint_discovery(T, None, upd)
            (w1 * best + w2 * all_).backward()
            key = f'{name}/grad_{w1:g}_{w2:g}'
            rec[f'{key}/joint_pos'] = f32(model.joint_pos.grad)
            if not detach:
                rec[f'{key}/spT'] = f32(T.grad)
        for k, v in ins.items():
            rec[f'{name}/in/{k}'] = v
        rec[f'{name}/out/best'], rec[f'{name}/out/all'] = f32(best), f32(all_)
        rec[f'{name}/out/joint_cost'], rec[f'{name}/out/joint_pos'] = f32(model.joint_cost), f32(model.joint_pos)
        rec[f'{name}/out/parents'] = model.joint_parents.numpy().astype(np.int32)
        rec[f'{name}/out/depth'] = model.joint_depth.numpy().astype(np.int32)
        rec[f'{name}/out/root'] = np.int64(int(model.joint_root))
        print(f'{name:22s} M {M:3d}  best {float(best):.6f}  all {float(all_):.6f}  root {int(model.joint_root)}')
    return rec


def main():
    rec = generate()
    if '--check' in sys.argv:
        have = np.load(OUT)
        assert sorted(have.files) == sorted(rec), 'key sets differ'
        for k in rec:
            assert np.array_equal(have[k], rec[k]), k
        print(f'{OUT}: reproduced ({len(rec)} arrays)')
        return
    np.savez_compressed(OUT, **rec)
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    main()
