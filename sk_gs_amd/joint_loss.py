"""The joint-discovery loss of stage ``sp`` (``SkeletonGaussianSplatting.loss_joint_discovery``, networks/sk_gs.py:1309-1336) and its tree
rebuild (``joint_discovery``, :106-131) for an UNMODIFIED checkout of the reference: ``accelerate_reference(joint_loss=True)``.

The shipped schedule runs the pair ``joint`` / ``joint_all`` (exps/default.yaml:93-94) in every stage-sp iteration from step 20 000 to
40 000 (sk_gs.py:1554-1560).  torch writes it as two [M, M, 4, 4] broadcast products plus ~35 element-wise launches of
``quaternion_to_Rt``, three norms, the EMA of ``joint_cost`` and two gathers; here it is one launch over the M^2 pairs, one small reduce
after the reference's own ``update_joint`` (when it runs), and one pair launch plus one finalize launch backward (csrc/joint_loss.hip).

``loss_joint_discovery`` keeps the reference's order: ``init_joint_pos()``; the EMA ``joint_cost = joint_cost * sk_momentum + jd * (1 -
sk_momentum)`` (training); the reference's ``update_joint()`` when asked or when there is no pair list yet; only THEN the pairs ``(a, b)``
of ``self.joint_pair`` and ``best = mean((jd[a, b] + jd[b, a]) / 2)``, ``all = jd.mean()``.  Calls outside the conditions (``sp_T_c``
given, a CPU or non-fp32 tensor, M outside 2..1024, ``joint_pos`` not a contiguous [M, M, 3], ``joint_cost`` not [M, M]) reach the
reference's own method.

``joint_discovery(cost)`` follows the compiled reference (my_ext/_C/src/nerf/sp_gs_joint.cu:55-85): Kruskal over all M^2 entries in
ascending cost order (the matrix is not symmetric; entry (a, b) is a candidate edge between a and b), ties broken by the flat index; the
root is the last node of the FIFO leaf peeling (leaves in index order, each node's neighbours most recently added edge first); the
binary-lifting table has L columns, the smallest L with 2^L >= the peeling depth, filled with the root.  Host code: one device-to-host
copy of ``cost``, one host-to-device copy of the result.
"""
import ctypes as C

import numpy as np
import torch

from sk_gs_amd import _C

calls = {'joint_loss_fused': 0, 'joint_loss_reference': 0, 'joint_discovery_fused': 0, 'joint_discovery_reference': 0}  # (tests)
_originals = {}     # filled by reference_accel.accelerate_reference(joint_loss=True): 'loss' -> the method, 'discovery' -> the function


def _p(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def _lib():
    lib = _C.load_library()
    lib.skgs_joint_loss_backward_workspace_bytes.restype = C.c_size_t
    lib.skgs_joint_loss_partials.restype = C.c_int32
    return lib


# ------------------------------------------------------------------------------------------------ the tree rebuild
def discovery_host(cost: np.ndarray):
    """(parents int32 [M, L], depth int32 [M], root) of the cost matrix [M, M] (M >= 3), as numpy; see the module's docstring"""
    M = cost.shape[0]
    flat = cost.reshape(-1)
    take = 8 * M
    while True:
        # the `take` cheapest entries and every entry tied with the last of them, in ascending order (ties: the lower flat index
        # first); a full sort only when the scan runs out before M - 1 unions
        if take >= flat.size:
            order = np.argsort(flat, kind='stable')
        else:
            cand = np.flatnonzero(flat <= np.partition(flat, take - 1)[take - 1])
            order = cand[np.argsort(flat[cand], kind='stable')]
        comp = list(range(M))

        def find(x):
            while comp[x] != x:
                comp[x] = comp[comp[x]]
                x = comp[x]
            return x

        adj = [[] for _ in range(M)]     # neighbours, most recently added edge first (the head-inserted lists of sp_gs_joint.cu)
        unions = 0
        for e in order.tolist():
            b, a = divmod(e, M)
            ra, rb = find(a), find(b)
            if ra == rb:
                continue
            comp[ra] = rb
            adj[a].insert(0, b)
            adj[b].insert(0, a)
            unions += 1
            if unions == M - 1:
                break
        if unions == M - 1 or take >= flat.size:
            break
        take *= 4
    # the root: the last node the FIFO leaf peeling removes (find_joint_root)
    n_edges = [len(x) for x in adj]
    visited = [0] * M
    que = [i for i in range(M) if n_edges[i] <= 1]
    for i in que:
        visited[i] = 1
    i = 0
    while i < len(que):
        u = que[i]
        i += 1
        for v in adj[u]:
            if n_edges[v] > 1:
                visited[v] = max(visited[v], visited[u] + 1)
                n_edges[v] -= 1
                if n_edges[v] <= 1:
                    que.append(v)
    root = que[-1]
    max_depth = max(visited)
    L = 0
    while (1 << L) < max_depth:
        L += 1
    parents = np.full((M, L), root, dtype=np.int32)
    depth = np.zeros(M, dtype=np.int32)
    seen = np.zeros(M, dtype=bool)
    seen[root] = True
    bfs = [root]
    i = 0
    while i < len(bfs):
        u = bfs[i]
        i += 1
        for v in adj[u]:
            if not seen[v]:
                seen[v] = True
                if L > 0:
                    parents[v, 0] = u
                depth[v] = depth[u] + 1
                bfs.append(v)
    for lv in range(1, L):
        parents[:, lv] = parents[parents[:, lv - 1], lv - 1]
    return parents, depth, root


def joint_discovery(joint_cost: torch.Tensor):
    """``networks.sk_gs.joint_discovery`` (sk_gs.py:106-131) on the host: (parents int32 [M, L], depth int32 [M], root int) on
    ``joint_cost``'s device.  M < 3 goes to the reference's own function (L is 0 there)."""
    M = joint_cost.shape[0]
    if M < 3 or joint_cost.dim() != 2 or joint_cost.shape[1] != M:
        if 'discovery' not in _originals:
            raise RuntimeError('joint_discovery(): M < 3 is the reference function\'s; accelerate_reference(joint_loss=True) provides it')
        calls['joint_discovery_reference'] += 1
        return _originals['discovery'](joint_cost)
    calls['joint_discovery_fused'] += 1
    with torch.no_grad():
        cost = joint_cost.detach().to('cpu', torch.float32).numpy()
    parents, depth, root = discovery_host(cost)
    L = parents.shape[1]
    flat = torch.from_numpy(np.concatenate([parents.reshape(-1), depth])).to(joint_cost.device)   # (one copy: both tables in one buffer)
    return flat[:M * L].view(M, L), flat[M * L:], int(root)


# ------------------------------------------------------------------------------------------------ the loss
_init_cache = {}     # model -> (the joint_is_init buffer object, its version, its value)
_parent_cache = {}   # model -> (the _joint_pair tuple, parent table int32 [M], number of edges)


def _joint_is_init(model) -> bool:
    """``bool(self.joint_is_init)`` is a read-back; ``init_joint_pos`` REPLACES the buffer, so the value is cached per buffer object"""
    buf = model.joint_is_init
    hit = _init_cache.get(id(model))
    if hit is None or hit[0] is not buf or hit[1] != buf._version:
        hit = _init_cache[id(model)] = (buf, buf._version, bool(buf))
    return hit[2]


def _parents(model, M, device):
    """the pair list ``self.joint_pair`` = (a, b, mask) as a per-node table parent[a] = b (-1: no edge), cached by the tuple's identity.
    A negative b indexes from the end as torch's jd[a, b] does."""
    pair = model.joint_pair
    hit = _parent_cache.get(id(model))
    if hit is None or hit[0] is not pair:
        a, b = pair[0], pair[1]
        with torch.no_grad():
            b = b.to(device=device, dtype=torch.int64)
            b = torch.where(b < 0, b + M, b).to(torch.int32)
            par = torch.full((M,), -1, dtype=torch.int32, device=device)
            par.scatter_(0, a.to(device=device, dtype=torch.int64), b)
        hit = _parent_cache[id(model)] = (pair, par, int(a.numel()))
    return hit[1], hit[2]


class _JointLoss(torch.autograd.Function):
    """(best, all) from the forward's jd and partials: ONE node with two scalar outputs"""

    @staticmethod
    def forward(ctx, spT, joint_pos, jd, partials, parent, edges, inverse):
        M = jd.shape[0]
        out = torch.empty(2, dtype=torch.float32, device=jd.device)
        _C._check(_lib().skgs_joint_loss_reduce(C.c_int32(M), C.c_int32(edges), _p(parent), _p(jd), _p(partials), _p(out), _C._stream()))
        ctx.save_for_backward(spT, joint_pos, parent)
        ctx.edges, ctx.inverse = edges, inverse
        return out[0], out[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_best, g_all):
        spT, joint_pos, parent = ctx.saved_tensors
        M = spT.shape[0]
        want_T = ctx.needs_input_grad[0]
        g_jp = torch.empty_like(joint_pos)
        g_T = torch.empty_like(spT) if want_T else None
        lib = _lib()
        ws = None
        if want_T:
            ws = torch.empty(int(lib.skgs_joint_loss_backward_workspace_bytes(C.c_int32(M))), dtype=torch.uint8, device=spT.device)
        gb = g_best.detach().to(torch.float32).contiguous() if g_best is not None else None
        ga = g_all.detach().to(torch.float32).contiguous() if g_all is not None else None
        _C._check(lib.skgs_joint_loss_backward(C.c_int32(M), C.c_int32(ctx.inverse), C.c_int32(ctx.edges), _p(spT), _p(joint_pos), _p(parent),
                                               _p(gb), _p(ga), _p(g_jp), _p(g_T), _p(ws), C.c_size_t(0 if ws is None else ws.numel()),
                                               _C._stream()))
        return g_T, g_jp, None, None, None, None, None


def supported(model, sp_T, sp_T_c) -> bool:
    jp, cost = getattr(model, 'joint_pos', None), getattr(model, 'joint_cost', None)
    if sp_T_c is not None or not (torch.is_tensor(sp_T) and torch.is_tensor(jp) and torch.is_tensor(cost)):
        return False
    if not (sp_T.is_cuda and sp_T.dtype == torch.float32 and sp_T.dim() == 2 and sp_T.shape[1] == 7):
        return False
    M = sp_T.shape[0]
    return (2 <= M <= 1024 and jp.dtype == torch.float32 and jp.device == sp_T.device and jp.is_contiguous() and tuple(jp.shape) == (M, M, 3)
            and cost.dtype == torch.float32 and cost.device == sp_T.device and tuple(cost.shape) == (M, M))


def loss_joint_discovery(self, sp_T, sp_T_c=None, update_joint=True):
    """``SkeletonGaussianSplatting.loss_joint_discovery`` (networks/sk_gs.py:1309-1336) through csrc/joint_loss.hip"""
    if not supported(self, sp_T, sp_T_c):
        calls['joint_loss_reference'] += 1
        return _originals['loss'](self, sp_T, sp_T_c, update_joint)
    calls['joint_loss_fused'] += 1
    if not _joint_is_init(self):
        self.init_joint_pos()                     # the reference's own (sets joint_pos to the superpoint midpoints, replaces the flag)
    spT = sp_T.detach() if self.sp_guided_detach else sp_T
    M, dev = spT.shape[0], spT.device
    inverse = 1 if self.canonical_time_id < 0 else 0
    lib = _lib()
    jd = torch.empty((M, M), dtype=torch.float32, device=dev)
    partials = torch.empty(int(lib.skgs_joint_loss_partials(C.c_int32(M))), dtype=torch.float32, device=dev)
    spT_c = spT.detach().contiguous()
    jp = self.joint_pos.detach()
    cost_in, cost_out, m = None, None, 0.0
    if self.training:
        cost_in = self.joint_cost.detach().contiguous()
        cost_out = torch.empty_like(cost_in)
        m = float(self.sk_momentum)
    _C._check(lib.skgs_joint_loss_forward(C.c_int32(M), C.c_int32(inverse), _p(spT_c), _p(jp), _p(cost_in), C.c_float(m), C.c_float(1.0 - m),
                                          _p(cost_out), _p(jd), _p(partials), _C._stream()))
    if self.training:
        with torch.no_grad():
            self.joint_cost = cost_out
            if update_joint or self._joint_pair is None:
                self.update_joint()
    parent, edges = _parents(self, M, dev)
    if edges < 1:
        raise RuntimeError('loss_joint_discovery(): the pair list is empty')
    T_in = spT if spT.requires_grad else spT_c
    return _JointLoss.apply(T_in if T_in.is_contiguous() else T_in.contiguous(), self.joint_pos, jd, partials, parent, edges, inverse)
