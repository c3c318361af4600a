"""`bench.py --dump-outputs DIR`: what the timed path computes from the benchmark's seeded inputs, as one .npy file per array, so that
two builds can be compared output for output.

Which step: the timed steps feed on each other, and the blend backward's float atomics do not order their additions -- two runs of ONE
build end their timed region ~300 Adam steps apart in rounding, which the training carries into the trained values (measured on config
#1 after 200 timed steps: the deform network's weights up to 0.15 of their largest element apart, the image up to 0.03).  So after the
timed region the benchmark goes back to its seeded start -- the parameters as generated, every optimizer at step 0 with zero moments,
the views rewound (`restart`) -- and runs ONE step of the timed path (the same captured graph); that step's inputs are the same in every
run.  Written are what that step computed from them, in float32 (float64 stays float64):

  image.npy, opacity.npy, loss.npy   the rendered image and opacity, the loss terms {total, L1, SSIM}: the same bit for bit in every run
  grad.<name>.npy                    the gradients as the step left them (the per-frame table gradients the optimizer clears after its
                                     update are left out: `cleared_grads`).  They differ by the rounding of the atomics' order --
                                     measured at config #1: 1.5e-6 of a tensor's largest element at most; 1e-10 in absolute terms on
                                     `sp_W`, whose softmax gradient is a difference of nearly equal per-bone terms, 2e-7 at most itself
  param.<name>.npy                   the parameters after the step's update.  From zero moments Adam's first update is lr x g / |g|:
                                     each element moves by its group's rate against the sign of its gradient; one whose gradient is
                                     0 stays put.  An element whose gradient is rounding noise around zero moves by +lr in one run
                                     and by -lr in the next (438 of the 2 M `sp_W` elements at config #1): such elements can be up to
                                     about 2 lr apart, all others agree up to rounding

Above LIMIT_BYTES in all, the arrays of more than SAMPLE_MIN_ROWS rows keep a fixed, seeded sample of their rows -- the SAME rows in
every array with the same number of rows, so that a parameter and its gradient stay aligned -- listed in `sampled_rows.<rows>.npy`."""
import os

import numpy as np
import torch

LIMIT_BYTES = 64 * 2 ** 20
SAMPLE_MIN_ROWS = 4096


def snapshot(model) -> list:
    """the parameters' values, taken before the first step -- in host memory: a device copy would move every later allocation
    (optimizer state, workspaces) and with it the timed region's memory layout"""
    return [p.detach().to('cpu', copy=True) for p in model.parameters()]


def restart(model, start, optimizers):
    """back to the seeded start, in place (captured graphs keep their addresses): the parameters as `snapshot` took them, every
    optimizer at step 0 with zero moments"""
    with torch.no_grad():
        for p, s in zip(model.parameters(), start):
            p.copy_(s)
    for opt in optimizers:
        if hasattr(opt, 'step_state'):  # FusedAdam: moments, the device step counter and the scheduled rates it derives from it
            with torch.no_grad():
                for p in opt.params:
                    opt.state[p]['exp_avg'].zero_(), opt.state[p]['exp_avg_sq'].zero_()
                opt._set_step_count(0.0)
            opt._upload()
            opt._refresh_captured_rates()
            opt._notify_state_changed()
        else:
            for st in opt.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()


def cleared_grads(model, optimizers) -> set:
    """names of the parameters whose gradients an optimizer clears after its update (FusedAdam(zero_after_step=...): the per-frame
    tables): read after the step, they are zeros, not what the step computed"""
    spans = [(z.data_ptr(), z.data_ptr() + z.numel() * z.element_size())
             for z in (getattr(o, 'zero_after_step', None) for o in optimizers) if z is not None]
    return {name for name, p in model.named_parameters()
            if p.grad is not None and any(a <= p.grad.data_ptr() < b for a, b in spans)}


def last_step_outputs(step, model, skip_grads=()) -> dict:
    """{name: tensor} of one training step: `step` is the fused step object (None on the operator path, which keeps no image)"""
    out = {}
    if step is not None:
        out.update(image=step.image, opacity=step.out_opacity, loss=step.loss3)
    for name, p in model.named_parameters():
        if p.grad is not None and name not in skip_grads:
            out['grad.' + name] = p.grad
        out['param.' + name] = p
    return out


def _host(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a if a.dtype == np.float64 else a.astype(np.float32)


def write(out_dir, arrays, limit=LIMIT_BYTES) -> dict:
    """writes `arrays` ({name: tensor}) to out_dir/<name>.npy within `limit` bytes; returns {name: shape written}"""
    os.makedirs(out_dir, exist_ok=True)
    host = {k: _host(v) for k, v in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    if total > limit:
        big = sorted(k for k, a in host.items() if a.ndim and a.shape[0] > SAMPLE_MIN_ROWS)
        counts = sorted({host[k].shape[0] for k in big})
        big_bytes = sum(host[k].nbytes for k in big)
        rest = total - big_bytes + sum(8 * n for n in counts)  # (+ the row lists, float64, at most)
        frac = max(0.0, (limit - rest) / max(1, big_bytes)) * 0.99
        rows = {n: np.sort(np.random.default_rng(n).choice(n, max(1, int(n * frac)), replace=False)) for n in counts}
        for k in big:
            host[k] = host[k][rows[host[k].shape[0]]]
        host.update({f'sampled_rows.{n}': r.astype(np.float64) for n, r in rows.items()})
    assert sum(a.nbytes for a in host.values()) <= limit, 'outputs exceed the dump limit'
    for k, a in host.items():
        np.save(os.path.join(out_dir, k + '.npy'), np.ascontiguousarray(a))
    return {k: list(a.shape) for k, a in host.items()}
