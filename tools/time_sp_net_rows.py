"""time the deform network on P rows (csrc/sp_net_rows.hip) against the same work in torch fp32 autograd
(``SpDeformNet.reference_forward``: the op sequence the reference's own DeformNetwork.forward runs), with HIP events.

    python tools/time_sp_net_rows.py [P ...]        (default: 8192 30000 100000 300000)

For every P: forward (no grad) and forward + backward (gradients of every parameter), each the mean of `reps` calls after a
warm-up, both paths in the same process.  TFLOP/s from the algorithmic count per row (508 928 multiply-adds forward, 970 240
backward); the share is of the 157.3 TF fp32 MFMA peak of the MI355X."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from sk_gs_amd.superpoint import SpDeformNet

PEAK_TF = 157.3
FWD_MACS = 93 * 256 + 6 * 256 * 256 + 349 * 256 + 10 * 256   # 508 928
BWD_MACS = 7 * 256 * 256 + 10 * 256 + FWD_MACS               # 970 240: activation chain + weight gradients


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [8192, 30000, 100000, 300000]
    torch.manual_seed(0)
    net = SpDeformNet().cuda()
    params = list(net.parameters())
    t = torch.tensor([0.3], device='cuda')
    rows = []
    for P in sizes:
        x = (torch.rand(P, 3, device='cuda') * 2 - 1)
        cot = [torch.randn(P, 3, device='cuda'), torch.randn(P, 4, device='cuda'), torch.randn(P, 3, device='cuda')]
        keys = ('d_xyz', 'd_rotation', 'd_scaling')
        reps = max(5, min(50, int(2e6 // P)))

        def kern_fwd():
            with torch.no_grad():
                net(x, t)

        def kern_fb():
            out = net(x, t)
            torch.autograd.grad([out[k] for k in keys], params, cot)

        def ref_fwd():
            with torch.no_grad():
                net.reference_forward(x, t)

        def ref_fb():
            out = net.reference_forward(x, t)
            torch.autograd.grad([out[k] for k in keys], params, cot)

        r = dict(P=P, reps=reps)
        for name, fn, macs in (('kernel_fwd', kern_fwd, FWD_MACS), ('kernel_fwd_bwd', kern_fb, FWD_MACS + BWD_MACS),
                               ('torch_fwd', ref_fwd, FWD_MACS), ('torch_fwd_bwd', ref_fb, FWD_MACS + BWD_MACS)):
            ms = timed(fn, 3, reps)
            tf = 2.0 * macs * P / (ms * 1e-3) / 1e12
            r[name] = dict(ms=round(ms, 4), tflops=round(tf, 2), share_of_peak=round(tf / PEAK_TF, 4))
        rows.append(r)
        print(f"P = {P:7d}  forward  kernels {r['kernel_fwd']['ms']:8.3f} ms ({r['kernel_fwd']['tflops']:6.1f} TF, "
              f"{100 * r['kernel_fwd']['share_of_peak']:5.1f} %)   torch {r['torch_fwd']['ms']:8.3f} ms ({r['torch_fwd']['tflops']:6.1f} TF)")
        print(f"              fwd+bwd  kernels {r['kernel_fwd_bwd']['ms']:8.3f} ms ({r['kernel_fwd_bwd']['tflops']:6.1f} TF, "
              f"{100 * r['kernel_fwd_bwd']['share_of_peak']:5.1f} %)   torch {r['torch_fwd_bwd']['ms']:8.3f} ms "
              f"({r['torch_fwd_bwd']['tflops']:6.1f} TF)", flush=True)
        del x, cot
    print(json.dumps(dict(tool='time_sp_net_rows', device=torch.cuda.get_device_name(0), peak_tflops=PEAK_TF, rows=rows)))


if __name__ == '__main__':
    main()
