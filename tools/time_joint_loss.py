#!/usr/bin/env python3
"""Times stage sp's joint-discovery loss (sk_gs_amd/joint_loss.py) against the reference's torch lines, and the tree rebuild against the
reference's Python fallback (both restated here: networks/sk_gs.py:1309-1336, :50-131).

    python tools/time_joint_loss.py [--out FILE] [--iters N]

For M in {128, 512, 1024}, canonical_time_id >= 0 / < 0, sp_guided_detach true / false: forward + backward of best + all, HIP events
around N iterations after a warm-up (the eager form includes the EMA of joint_cost and the two gathers, as the reference runs them; the
fast path includes the same EMA and no tree update).  Then one tree rebuild per M: the Python fallback (511 argmin rounds with host
syncs at M = 512, then find_root) against sk_gs_amd.joint_loss.joint_discovery, wall clock after torch.cuda.synchronize()."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sk_gs_amd import joint_loss as jl  # noqa: E402

DEV = torch.device('cuda:0')


class Model(torch.nn.Module):
    """the attributes loss_joint_discovery reads on the reference's model, restated (a fixed tree: no update in the timed calls)"""

    def __init__(self, M, ct, detach, g):
        super().__init__()
        self.num_superpoints, self.canonical_time_id, self.sp_guided_detach, self.sk_momentum = M, ct, detach, 0.9
        self.joint_pos = torch.nn.Parameter((torch.randn(M, M, 3, generator=g) * 0.5).to(DEV))
        self.register_buffer('joint_is_init', torch.tensor(True, device=DEV))
        self.register_buffer('joint_cost', torch.rand(M, M, generator=g).to(DEV))
        parents, depth, root = jl.joint_discovery(self.joint_cost)
        mask = torch.ones(M, dtype=torch.bool, device=DEV)
        mask[root] = False
        self._joint_pair = (torch.arange(M, device=DEV)[mask], parents[mask, 0], mask)
        self.train()

    @property
    def joint_pair(self):
        return self._joint_pair


def eager_loss(m, sp_T):
    """sk_gs.py:1312-1335 with quaternion_to_Rt (rigid.py:110-130) and apply (xfm.py:60-79)"""
    sp_T = sp_T.detach() if m.sp_guided_detach else sp_T
    t, (x, y, z, w) = sp_T[:, :3], sp_T[:, 3:].unbind(-1)
    T = torch.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z, t[:, 0],
                     2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x, t[:, 1],
                     2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, 1 - 2 * x * x - 2 * y * y, t[:, 2],
                     torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x), torch.ones_like(x)], dim=-1).reshape(-1, 4, 4)

    def apply(p, mat):
        if p.shape[-1] + 1 == mat.shape[-1]:
            p = torch.constant_pad_nd(p, (0, 1), 1.0)
        return torch.sum(mat * p[..., None, :], dim=-1)[..., :3]

    jp = m.joint_pos
    if m.canonical_time_id < 0:
        Tab = torch.inverse(T[None, :]) @ T[:, None]
        d = Tab[..., :3, 3] - (jp - apply(jp, Tab[..., :3, :3]))
    else:
        d = apply(jp, T[None, :]) - apply(jp, T[:, None, :3, :3]) - T[:, None, :3, 3]
    jd = d.norm(dim=-1)
    jpt = apply(jp, T)
    jd = jd + (jpt - jpt.transpose(0, 1)).norm(dim=-1)
    with torch.no_grad():
        m.joint_cost = m.joint_cost * m.sk_momentum + jd * (1. - m.sk_momentum)
    a, b, _ = m.joint_pair
    return ((jd[a, b] + jd[b, a]) * 0.5).mean(), jd.mean()


def fast_loss(m, sp_T):
    return jl.loss_joint_discovery(m, sp_T, None, False)


def time_ms(fn, m, spT, iters):
    for _ in range(5):
        T = spT.clone().requires_grad_()
        best, all_ = fn(m, T)
        (best + all_).backward()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    Ts = [spT.clone().requires_grad_() for _ in range(iters)]
    s.record()
    for T in Ts:
        m.joint_pos.grad = None
        best, all_ = fn(m, T)
        (best + all_).backward()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def python_discovery(joint_cost):
    """sk_gs.py:106-131 + find_root :50-103 (the Python function the reference runs where my_ext._C does not serve it), restated"""
    M = joint_cost.shape[0]
    connectivity = torch.eye(M, device=joint_cost.device, dtype=torch.long)
    joint_connection = torch.full((M,), -1, device=joint_cost.device, dtype=torch.long)
    for _ in range(M - 1):
        connected = torch.argmin(joint_cost + connectivity * 1e10)
        idx_0, idx_1 = connected // M, connected % M
        connectivity[idx_0] = torch.maximum(connectivity[idx_0].clone(), connectivity[idx_1].clone())
        connectivity[torch.where(connectivity[idx_0] == 1)] = connectivity[idx_0].clone()
        if joint_connection[idx_0] == -1:
            joint_connection[idx_0] = idx_1
        else:
            parents = [idx_1]
            a = joint_connection[idx_1]
            while a != -1:
                parents.append(a)
                a = joint_connection[a]
            for i in range(len(parents) - 1, 0, -1):
                joint_connection[parents[i]] = parents[i - 1]
            joint_connection[idx_1] = idx_0
    father = joint_connection
    edges = {i: [] for i in range(M)}
    for i in range(M):
        if father[i] < 0:
            continue
        j = father[i].item()
        edges[i].append(j)
        edges[j].append(i)
    visited = np.zeros(M, dtype=np.int32)
    num_edges = np.array([len(edges[i]) for i in range(M)])
    que = [i for i in range(M) if num_edges[i] == 1]
    for node in que:
        visited[node] = 1
    i = 0
    while i < len(que):
        now = que[i]
        i += 1
        for node in edges[now]:
            if num_edges[node] > 1:
                num_edges[node] -= 1
                visited[node] = max(visited[node], visited[now] + 1)
                if num_edges[node] == 1:
                    que.append(node)
    root = que[-1]
    max_depth, max_level = visited.max(), 0
    while 2 ** max_level < max_depth:
        max_level += 1
    parents = father.new_full((M, max_level), root)
    depth = parents.new_zeros(M)
    que, visited[:] = [root], 0
    visited[root] = 1
    i = 0
    while i < len(que):
        now = que[i]
        i += 1
        for node in edges[now]:
            if visited[node] == 0:
                parents[node, 0] = now
                depth[node] = depth[now] + 1
                que.append(node)
                visited[node] = 1
    for i in range(1, max_level):
        for j in range(M):
            parents[j, i] = parents[parents[j, i - 1], i - 1]
    return parents, depth, root


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--sizes', default='128,512,1024')
    ap.add_argument('--skip-python-rebuild-above', type=int, default=1024)
    args = ap.parse_args()
    jl._originals.setdefault('loss', lambda *a, **k: (_ for _ in ()).throw(AssertionError('left the fast path')))
    lines = [f'# stage sp joint-discovery loss, forward + backward of best + all, mean of {args.iters} iterations after warm-up (HIP events)',
             f'# {torch.cuda.get_device_name(0)}; eager = the reference torch lines restated; fast = sk_gs_amd.joint_loss',
             f'{"M":>5} {"branch":>8} {"detach":>6} {"eager_ms":>9} {"fast_ms":>8} {"speedup":>7}']
    for M in [int(s) for s in args.sizes.split(',')]:
        for ct in (0, -1):
            for detach in (True, False):
                g = torch.Generator().manual_seed(M)
                m = Model(M, ct, detach, g)
                spT = torch.cat([torch.randn(M, 3, generator=g) * 0.3, torch.randn(M, 4, generator=g) * 0.15 + torch.tensor([0, 0, 0, 1.])], -1).to(DEV)
                te = time_ms(eager_loss, m, spT, args.iters)
                tf = time_ms(fast_loss, m, spT, args.iters)
                lines.append(f'{M:5d} {"ct>=0" if ct >= 0 else "ct<0":>8} {str(detach):>6} {te:9.3f} {tf:8.3f} {te / tf:6.1f}x')
                print(lines[-1], flush=True)
    lines.append('# tree rebuild (joint_discovery on a [M, M] device cost), wall clock incl. the copies')
    lines.append(f'{"M":>5} {"python_fallback_ms":>18} {"host_kruskal_ms":>15}')
    for M in [int(s) for s in args.sizes.split(',')]:
        cost = torch.rand(M, M, generator=torch.Generator().manual_seed(M + 1)).to(DEV)
        jl.joint_discovery(cost)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        jl.joint_discovery(cost)
        torch.cuda.synchronize()
        t_ours = (time.perf_counter() - t0) * 1e3
        t_py = float('nan')
        if M <= args.skip_python_rebuild_above:
            t0 = time.perf_counter()
            python_discovery(cost)
            torch.cuda.synchronize()
            t_py = (time.perf_counter() - t0) * 1e3
        lines.append(f'{M:5d} {t_py:18.1f} {t_ours:15.1f}')
        print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text)
    print(text)


if __name__ == '__main__':
    main()
