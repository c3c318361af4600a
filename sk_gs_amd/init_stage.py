"""Stages ``init_fix`` / ``init`` of the hot path (networks/sk_gs.py:741-749,1169-1173): the deform network over EVERY Gaussian.

In the first 10 000 of the reference's 80 000 default steps (``init_fix`` 2 000 + ``init`` 8 000, exps/default.yaml:12-19) a Gaussian's
offset is ``sp_deform_net(xyz.detach(), t)['d_xyz']`` on all P rows, and the rest of ``forward`` is an activation epilogue:

    points    = xyz + d_xyz                      (init_fix: d_xyz detached -- the network gets no gradient)
    scales    = exp(mean(_scaling))              scales_all_same (hard-coded True, sk_gs.py:535): ONE mean over all P x 3 values
    rotations = normalize(_rotation + 0),  opacity = sigmoid(_opacity),  d_rotation = d_scaling = the constant 0

``FusedInitStep`` runs one view of it as a straight line of C-ABI calls on persistent buffers (the sibling of ``FusedViewStep`` /
``FusedSuperpointStep``, sharing their rasterizer / loss half):

    skgs_sp_net_rows_forward      the network on P rows -> raw [P,10|14] (init: the activations for the backward)   (1 launch)
    rasterize forward + offset_job   the log-scale mean (1 small launch), then the epilogue in the lane that projects each
                                     Gaussian, reading columns 0:3 of ``raw`` in place (skgs_offset_deform_job)
    rasterize backward + offset_job  g_xyz, g_raw[:, 0:3] (init), g_rotation / g_opacity through normalize / sigmoid, and the
                                     log-scale mean's backward: one constant for all of ``_scaling.grad`` (1 small launch)
    skgs_sp_net_rows_backward     (init) every network parameter's gradient from g_raw                              (3 launches)

The network's backward writes a gradient for every parameter; the heads the stage leaves without one (``gaussian_rotation``,
``gaussian_scaling``, ``local_rotation``: their ``.grad`` stays None in the reference) write into scratch tensors of the step.
"""
import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from sk_gs_amd import _C
from sk_gs_amd.fused_step import FusedViewStep, _p
from sk_gs_amd.superpoint import SpDeformNet, _net_desc, _rows_lib

INIT_STAGES = ('init_fix', 'init')
SCALE_GLOBAL, SCALE_PER_ROW = 0, 1      # include/skgs.h: SKGS_OFFSET_SCALE_GLOBAL / _PER_ROW


def untrained_heads(net: SpDeformNet):
    """the network's parameters stage init gives no gradient: the rotation / scaling heads (and ``local_rotation`` with sep_rot)"""
    mods = [net.gaussian_rotation, net.gaussian_scaling] + ([net.local_rotation] if net.sep_rot else [])
    return [q for m in mods for q in (m.weight, m.bias)]


def trained_net_parameters(net: SpDeformNet):
    """the network's parameters that receive a gradient in stage init, in ``net.parameters()`` order"""
    skip = {id(q) for q in untrained_heads(net)}
    return [q for q in net.parameters() if id(q) not in skip]


class FusedInitStep(FusedViewStep):
    """forward + loss + backward of one view in stage ``init_fix`` or ``init``.  ``model``: the six Gaussian tensors under the reference's
    names, ``sp_deform_net`` (an ``SpDeformNet`` the kernels cover, ``is_blender``), ``max_sh_degree``, ``P``, ``parameters()``; every
    gradient is WRITTEN into the parameter's ``.grad`` storage."""

    def __init__(self, model, W: int, H: int, capacity: int, stage: str = 'init', lambda_dssim: float = 0.2,
                 background: Optional[Tensor] = None, tile_bucket: int = 0, view_table=None, scale_mode: int = SCALE_GLOBAL):
        net = model.sp_deform_net
        assert stage in INIT_STAGES and isinstance(net, SpDeformNet) and net.kernel_supported() and net.is_blender
        assert getattr(model, 'capacity', None) is None, 'stage init: no row capacity'
        model.sk_deform_net = None  # (what FusedViewStep's constructor probes for the stage-sk network)
        super().__init__(model, W, H, capacity, lambda_dssim=lambda_dssim, background=background, tile_bucket=tile_bucket, view_table=None)
        self.view_table = view_table
        if view_table is not None:
            vs = view_table.settings
            assert (vs.image_height, vs.image_width) == (self.H, self.W)
        self.stage, self.train_net, self.scale_mode = stage, stage == 'init', int(scale_mode)
        self.net_module = net
        lib, dev, P = self.lib, model._xyz.device, self.P
        f32, u8 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.uint8, device=dev)
        self.nout = 14 if net.sep_rot else 10
        self.raw = torch.empty((P, self.nout), **f32)         # d_xyz | d_rotation | d_scaling (| g_rotation): the job reads columns 0:3
        self.scale_mean = torch.zeros(1, **f32)                # exp(this) is every Gaussian's scale (written by the forward)
        self.offset_ws = torch.zeros((int(lib.skgs_offset_deform_workspace_bytes(C.c_int32(P))),), **u8)   # zero before the first call
        self.saved = self.net_ws = self.g_raw = None
        self._scratch = {}
        if self.train_net:
            rl = _rows_lib()
            self.saved = torch.empty((int(rl.skgs_sp_net_rows_saved_bytes(C.c_int32(P))),), **u8)
            self.net_ws = torch.empty((int(rl.skgs_sp_net_rows_workspace_bytes(C.c_int32(P))),), **u8)
            # columns 3: stay zero -- d_rotation / d_scaling / g_rotation reach nothing in this stage; the job writes columns 0:3
            self.g_raw = torch.zeros((P, self.nout), **f32)
            self._scratch = {id(q): torch.empty_like(q) for q in untrained_heads(net)}
        self.wide = False

    # ---- the pieces FusedViewStep asks its subclass for --------------------------------------------------------------
    def table_grad_span(self):
        return None

    def _zero_table_grads(self):
        pass  # no per-frame tables in these stages

    def _time(self, time_id) -> Tensor:
        if time_id is not None:
            return self.model.frame_times[time_id]
        from sk_gs_amd import view_slot as vsl
        return self.view_table.slot[vsl.W_TIME:vsl.W_TIME + 1]

    def _offset_job(self) -> '_C._OffsetDeformJob':
        m = self.model
        j = _C._OffsetDeformJob()
        j.scale_mode, j.d_xyz_stride = self.scale_mode, self.nout
        j.xyz, j.d_xyz, j.log_scale = m._xyz.data_ptr(), self.raw.data_ptr(), m._scaling.data_ptr()
        j.rot, j.opacity_logit, j.scale_mean = m._rotation.data_ptr(), m._opacity.data_ptr(), self.scale_mean.data_ptr()
        j.means, j.scales, j.rotations, j.opacity = self.means.data_ptr(), self.scales.data_ptr(), self.rotations.data_ptr(), self.opacity.data_ptr()
        j.workspace, j.workspace_bytes = self.offset_ws.data_ptr(), self.offset_ws.numel()
        return j

    @torch.no_grad()
    def forward(self, rs=None, time_id=None):
        lib, m, st, chk = self.lib, self.model, _C._stream(), _C._check
        assert (rs is None) == (time_id is None) and (rs is not None or self.view_table is not None)
        P = self.P
        d = _net_desc(self.net_module, P, m._xyz, self._time(time_id))   # (points = xyz.detach(): the same storage)
        chk(lib.skgs_sp_net_rows_forward(C.byref(d), _p(self.raw), _p(self.saved), C.c_size_t(0 if self.saved is None else self.saved.numel()), st))
        a = self._raster_inputs(rs)
        j = self._offset_job()
        a.offset_job = C.cast(C.pointer(j), C.c_void_p)
        chk(lib.skgs_rasterize_forward(C.byref(a), C.byref(self._bufs), _p(self.radii), _p(self.image), _p(self.out_opacity), None, None, st))
        a.offset_job = None  # (the backward's copy of the inputs: the job was the forward's)
        return a, None

    def _attach_backward_job(self, g, d, time_id):
        """the epilogue's backward as a job of the rasterizer's per-Gaussian backward launch (skgs_raster_grads.offset_job)"""
        m = self.model
        j = self._offset_job()
        j.g_xyz, j.g_log_scale = m._xyz.grad.data_ptr(), m._scaling.grad.data_ptr()
        j.g_rot, j.g_opacity_logit = m._rotation.grad.data_ptr(), m._opacity.grad.data_ptr()
        j.g_d_xyz = self.g_raw.data_ptr() if self.train_net else None
        g.offset_job = C.cast(C.pointer(j), C.c_void_p)
        self._rows_backward_done = True
        return j

    def _grad_desc(self):
        """the network's gradient targets: the parameters' ``.grad``, scratch for the heads the stage does not train"""
        net = self.net_module
        saved = {}
        try:
            for q in untrained_heads(net):
                saved[q] = q.grad
                q.grad = self._scratch[id(q)]
            return _net_desc(net, self.P, None, None, grads=True)
        finally:
            for q, gq in saved.items():
                q.grad = gq

    @torch.no_grad()
    def backward_skinning(self, time_id=None, part=None):
        assert part is None
        if not self.train_net:   # init_fix: d_xyz is detached, the network gets no gradient
            return
        lib, st = _rows_lib(), _C._stream()
        d = _net_desc(self.net_module, self.P, None, None)
        dg = self._grad_desc()
        _C._check(lib.skgs_sp_net_rows_backward(C.byref(d), C.byref(dg), _p(self.g_raw), _p(self.saved), C.c_size_t(self.saved.numel()),
                                                _p(self.net_ws), C.c_size_t(self.net_ws.numel()), st))

    def status(self) -> dict:
        return _C.read_status(self.geom)
