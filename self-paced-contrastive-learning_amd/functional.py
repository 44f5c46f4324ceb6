"""torch.autograd.Function wrappers around the C ABI (native.py).  Device tensors in, device tensors out;
no host synchronisation anywhere in this file."""
from __future__ import annotations

import collections
import ctypes
import math
import os
import struct
from ctypes import c_double, c_float, c_int

import torch

from . import native as _n

SP_NONE, SP_HARD, SP_SOFT = 0, 1, 2


# --------------------------------------------------------------------------------------------- gradient sinks
def take_grad_sink(param, needed: bool = True):
    """Where a parameter's gradient should be written: its ARMED sink (a contiguous fp32 view of a flat gradient bucket,
    installed by ddp.FlatParams.zero_grad) or None (allocate).  Claimed IN BACKWARD, at the point the kernel writes
    (a forward that never runs backward leaves the arming untouched).  A sink serves one backward per arming: the
    backward kernels write the gradient straight into the bucket and return a fresh view of it, which autograd adopts
    as ``param.grad`` without a copy; a second use of the same parameter in that step allocates normally and autograd
    adds it into the bucket in place.  ``ddp.GradBucket.gather`` disarms whatever was not claimed."""
    if not needed or param is None:
        return None
    sink = getattr(param, "_grad_sink", None)
    if sink is None or not getattr(param, "_grad_sink_armed", False):
        return None
    if sink.shape != param.shape or sink.dtype != torch.float32 or not sink.is_contiguous() or sink.device != param.device:
        return None
    param._grad_sink_armed = False
    return sink


def _grad_buffer(sink, shape, dev):
    return sink.view(shape) if sink is not None else torch.empty(shape, dtype=torch.float32, device=dev)


# --------------------------------------------------------------------------------------------- contrastive loss
class SupConState:
    """Device-side results of one loss evaluation (kept for backward and for the lazily materialised taps)."""
    __slots__ = ("n", "d", "t", "sp_mode", "gamma", "labels", "mask", "ws", "out")


class _SupConFn(torch.autograd.Function):
    """``stacked``: z1 is the whole [2n, d] projection (view 1 rows, then view 2 rows) and z2 is None; the gradient
    comes back as one [2n, d] tensor (no chunk / cat copies around the loss)."""

    @staticmethod
    def forward(ctx, z1, z2, labels, mask, t, sp_mode, gamma, correct_grad, state: SupConState, raw=False):
        stacked = z2 is None
        _n.require_gpu(z1, labels, mask) if stacked else _n.require_gpu(z1, z2, labels, mask)
        z1c = z1.detach().contiguous().float()
        if stacked:
            assert z1c.dim() == 2 and z1c.shape[0] % 2 == 0, z1c.shape
            n, d = z1c.shape[0] // 2, z1c.shape[1]
            z2c = z1c[n:]
        else:
            z2c = z2.detach().contiguous().float()
            n, d = z1c.shape
        nbytes = _n.call("spcl_supcon_workspace_bytes", n, d)
        if nbytes == 0:
            raise RuntimeError(f"supcon: unsupported shape n={n} d={d} (d must be <= 4096)")
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=z1.device)
        out = torch.empty(8, dtype=torch.float32, device=z1.device)  # the kernel writes loss, rho, kappa, norm defect
        if raw:
            # the rows BEFORE F.normalize: the launch normalises them itself and its unit-gradient block is d loss / d raw
            # rows (spcl_supcon_forward_rows; supcon_loss has checked that the shape is supported and there is no mask)
            gam = (c_float * 1)(float(gamma))
            _n.call("spcl_supcon_forward_rows", 1, _n.ptr(z1c), _n.ptr(z2c), 0, _n.ptr(labels), n, d, c_float(t), sp_mode,
                    gam, int(bool(correct_grad)), _n.ptr(ws), 0, _n.ptr(out), _n.stream())
        else:
            _n.call("spcl_supcon_forward", _n.ptr(z1c), _n.ptr(z2c), _n.ptr(labels), _n.ptr(mask), n, d, c_float(t),
                    sp_mode, c_float(gamma), int(bool(correct_grad)), _n.ptr(ws), _n.ptr(out), _n.stream())
        state.n, state.d, state.t, state.sp_mode, state.gamma = n, d, t, sp_mode, gamma
        state.labels, state.mask, state.ws, state.out = labels, mask, ws, out
        ctx.state = state
        ctx.stacked = stacked
        ctx.in_dtypes = (z1.dtype, z1.dtype if stacked else z2.dtype)
        # a LEAF input keeps the gradient it is handed as its .grad (AccumulateGrad steals the buffer): it must then own it
        ctx.leaf_input = bool(z1.is_leaf)
        return out[0]

    @staticmethod
    def backward(ctx, grad_out):
        s = ctx.state
        dev = s.ws.device
        if ctx.stacked and ctx.in_dtypes[0] == torch.float32 and is_unit_gradient(grad_out):
            # the epocher's own ``backward(gradient=ones)``: the forward already left dLoss/dP for a unit gradient in its
            # workspace (training sizes) -- that block IS the gradient, no scaling launch
            off, pitch = ctypes.c_size_t(0), ctypes.c_int(0)
            if (_n.call("spcl_supcon_unit_gradient_block", s.n, s.d, ctypes.byref(off), ctypes.byref(pitch))
                    and pitch.value == s.d):
                dz = s.ws[off.value:off.value + 2 * s.n * s.d].view(2 * s.n, s.d)
                if ctx.leaf_input:  # (in-place operations on that .grad would write into the workspace the taps read)
                    dz = dz.clone()
                return dz, None, None, None, None, None, None, None, None, None
        dz = torch.empty(2 * s.n, s.d, dtype=torch.float32, device=dev)
        dz1, dz2 = dz[:s.n], dz[s.n:]
        wsb = torch.empty(_n.call("spcl_supcon_bwd_workspace_bytes", s.n, s.d) // 4, dtype=torch.float32, device=dev)
        go = grad_out.detach().reshape(1).float().contiguous()
        _n.call("spcl_supcon_backward", _n.ptr(s.labels), _n.ptr(s.mask), s.n, s.d, c_float(s.t), s.sp_mode,
                c_float(s.gamma), _n.ptr(s.ws), _n.ptr(wsb), _n.ptr(s.out), _n.ptr(go), _n.ptr(dz1), _n.ptr(dz2),
                _n.stream())
        if ctx.stacked:
            return dz.to(ctx.in_dtypes[0]), None, None, None, None, None, None, None, None, None
        return dz1.to(ctx.in_dtypes[0]), dz2.to(ctx.in_dtypes[1]), None, None, None, None, None, None, None, None


def supcon_rows_supported(n, d, mask=None):
    """can the loss launch take the rows BEFORE F.normalize (``normalize_inputs``)?  training sizes, no explicit mask"""
    return mask is None and bool(_n.call("spcl_supcon_rows_supported", int(n), int(d)))


def supcon_loss(z1, z2, labels=None, mask=None, *, t=0.07, sp_mode=SP_NONE, gamma=1e6, correct_grad=False,
                state: SupConState = None, normalize_inputs=False):
    """loss (0-dim tensor with grad_fn).  ``state`` receives the device-side statistics (rho = state.out[1]).
    ``normalize_inputs``: z1 / z2 are rows BEFORE ``F.normalize(dim=1)``; the loss is that of the normalised rows and
    the gradient the one w.r.t. the given rows -- inside the loss launch where its schedule allows
    (``supcon_rows_supported``), by the row-normalisation kernels in front of it otherwise."""
    if state is None:
        state = SupConState()
    raw = False
    if normalize_inputs:
        n = z1.shape[0] // 2 if z2 is None else z1.shape[0]
        if z1.dtype == torch.float32 and supcon_rows_supported(n, z1.shape[1], mask):
            raw = True
        else:
            z1 = l2norm_rows(z1)
            z2 = l2norm_rows(z2) if z2 is not None else None
    return _SupConFn.apply(z1, z2, labels, mask, float(t), int(sp_mode), float(gamma), bool(correct_grad), state, raw)


class _SupConHeadsFn(torch.autograd.Function):
    """K (2..4) losses of one shape in the launches of one (spcl_supcon_forward_heads / _backward_heads): the K meta-label
    hooks on one feature, each with its own labels and age parameter.  Inputs after the fixed ones: the K stacked
    [2n, d] projections; output: a [K] tensor of losses.  Per head the arithmetic (and the workspace / result block the
    ``states`` receive) is exactly that of ``_SupConFn``."""

    @staticmethod
    def forward(ctx, labels, t, sp_mode, gammas, correct_grad, states, raw, *zs):
        K = len(zs)
        _n.require_gpu(*zs)
        n2, d = zs[0].shape
        assert n2 % 2 == 0 and all(z.shape == zs[0].shape for z in zs), [tuple(z.shape) for z in zs]
        n = n2 // 2
        dev = zs[0].device
        step = n2 * d * 4
        if all(z.dtype == torch.float32 and z.is_contiguous() and z.data_ptr() == zs[0].data_ptr() + k * step
               for k, z in enumerate(zs)):
            zall = zs[0].detach()  # the batched projection wrote its heads back to back: no copy
        else:
            zall = torch.stack([z.detach().float() for z in zs])
        nbytes = _n.call("spcl_supcon_workspace_bytes", n, d)
        if nbytes == 0:
            raise RuntimeError(f"supcon: unsupported shape n={n} d={d} (d must be <= 4096)")
        ws_stride = (nbytes // 4 + 63) // 64 * 64
        ws = torch.empty(K * ws_stride, dtype=torch.float32, device=dev)
        out = torch.empty(K, 8, dtype=torch.float32, device=dev)
        gam = (c_float * K)(*[float(g) for g in gammas])
        base = zall.data_ptr()
        _n.call("spcl_supcon_forward_rows" if raw else "spcl_supcon_forward_heads", K, base, base + n * d * 4, n2 * d,
                _n.ptr(labels), n, d, c_float(t), sp_mode, gam, int(bool(correct_grad)), _n.ptr(ws), ws_stride, _n.ptr(out),
                _n.stream())
        for k, st in enumerate(states):
            st.n, st.d, st.t, st.sp_mode, st.gamma = n, d, t, sp_mode, float(gammas[k])
            st.labels, st.mask = (labels[k] if labels is not None else None), None
            st.ws, st.out = ws[k * ws_stride:(k + 1) * ws_stride], out[k]
        ctx.keep = (labels, ws, out, zall)
        ctx.meta = (K, n, d, t, sp_mode, tuple(float(g) for g in gammas), ws_stride, [z.dtype for z in zs])
        # K separate 0-dim losses (views of the result block: no copy; a [K] tensor that the hooks then unbind costs a
        # stacking launch in its backward)
        return tuple(out[k, 0] for k in range(K))

    @staticmethod
    def backward(ctx, *grads_out):
        K, n, d, t, sp_mode, gammas, ws_stride, dtypes = ctx.meta
        labels, ws, out, _ = ctx.keep
        dev = ws.device
        dz = torch.empty(K, 2 * n, d, dtype=torch.float32, device=dev)
        wsb_stride = (_n.call("spcl_supcon_bwd_workspace_bytes", n, d) // 4 + 63) // 64 * 64
        wsb = torch.empty(K * wsb_stride, dtype=torch.float32, device=dev)
        if all(g is not None and is_unit_gradient(g) for g in grads_out):
            go = _ones_k(K, dev)  # every head's upstream gradient is the epocher's registered 1: a cached vector of ones
        else:
            go = torch.stack([torch.zeros((), dtype=torch.float32, device=dev) if g is None else g.detach().float().reshape(())
                              for g in grads_out])
        gam = (c_float * K)(*gammas)
        base = dz.data_ptr()
        _n.call("spcl_supcon_backward_heads", K, _n.ptr(labels), n, d, c_float(t), sp_mode, gam, _n.ptr(ws), ws_stride,
                _n.ptr(wsb), wsb_stride, _n.ptr(out), _n.ptr(go), base, base + n * d * 4, 2 * n * d, _n.stream())
        return (None, None, None, None, None, None, None) + tuple(dz[k].to(dtypes[k]) for k in range(K))


_ONES_K = {}


def _ones_k(K, dev):
    key = (K, str(dev))
    t = _ONES_K.get(key)
    if t is None:
        t = _ONES_K[key] = torch.ones(K, dtype=torch.float32, device=dev)
    return t


def supcon_loss_heads(zs, labels=None, *, t=0.07, sp_mode=SP_NONE, gammas=None, correct_grad=False, states=None,
                      normalize_inputs=False):
    """K 0-dim losses (a tuple) of the K stacked [2n, d] projections ``zs`` (2 <= K <= 4); ``labels``: [K, n] float tensor or
    None; ``gammas``: K floats; ``states``: K SupConState objects that receive each head's device-side statistics.
    ``normalize_inputs``: as in ``supcon_loss``."""
    K = len(zs)
    if states is None:
        states = [SupConState() for _ in range(K)]
    if gammas is None:
        gammas = [1e6] * K
    raw = False
    if normalize_inputs:
        if all(z.dtype == torch.float32 for z in zs) and supcon_rows_supported(zs[0].shape[0] // 2, zs[0].shape[1]):
            raw = True
        else:
            zs = [l2norm_rows(z) for z in zs]
    return _SupConHeadsFn.apply(labels, float(t), int(sp_mode), tuple(gammas), bool(correct_grad), states, raw, *zs)


class _SupConXposFn(torch.autograd.Function):
    """SupConLoss1(exclude_other_pos=True), contrast_loss3.py:97-100 (csrc/supcon_xpos.hip)"""

    @staticmethod
    def forward(ctx, z1, z2, labels, mask, t, out):
        _n.require_gpu(z1, z2, labels, mask)
        z1c, z2c = z1.detach().contiguous().float(), z2.detach().contiguous().float()
        n, d = z1c.shape
        nbytes = _n.call("spcl_supcon_xpos_workspace_bytes", n, d)
        if nbytes == 0:
            raise RuntimeError(f"supcon (exclude_other_pos): unsupported shape n={n} d={d} (n <= 4096)")
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=z1.device)
        _n.call("spcl_supcon_xpos_forward", _n.ptr(z1c), _n.ptr(z2c), _n.ptr(labels), _n.ptr(mask), n, d, c_float(t),
                _n.ptr(ws), _n.ptr(out), _n.stream())
        ctx.save_for_backward(z1c, z2c, ws)
        ctx.meta = (n, d, t, z1.dtype, z2.dtype)
        return out[0]

    @staticmethod
    def backward(ctx, grad_out):
        z1c, z2c, ws = ctx.saved_tensors
        n, d, t, dt1, dt2 = ctx.meta
        dz1, dz2 = torch.empty_like(z1c), torch.empty_like(z2c)
        go = grad_out.detach().reshape(1).float().contiguous()
        _n.call("spcl_supcon_xpos_backward", _n.ptr(z1c), _n.ptr(z2c), n, d, c_float(t), _n.ptr(ws), _n.ptr(go),
                _n.ptr(dz1), _n.ptr(dz2), _n.stream())
        return dz1.to(dt1), dz2.to(dt2), None, None, None, None


def supcon_loss_exclude_other_pos(z1, z2, labels=None, mask=None, *, t=0.07, out=None):
    """-> loss (0-dim tensor with grad_fn); ``out`` (8 floats on the device) receives loss / norm defect"""
    if out is None:
        out = torch.empty(8, dtype=torch.float32, device=z1.device)
    return _SupConXposFn.apply(z1, z2, labels, mask, float(t), out)


class SupConWeightedState:
    """Device-side results of one weighted-loss evaluation (kept for the lazily materialised taps)."""
    __slots__ = ("n", "d", "t", "z1", "z2", "labels", "w11", "w22", "w12", "blocks", "mask_semantics", "ws", "out")


_WEIGHTED_UNIT_ROWS, _WEIGHTED_UNIT_D = 64, 256  # up to here the forward leaves dLoss/dz at the start of ws (spcl_hip.h)


class _SupConWeightedFn(torch.autograd.Function):
    """SupConLoss2 / 3 / 4 of contrast_loss.py:34-270 (csrc/supcon_weighted.hip).  ``z2 is None``: z1 is the whole [2n, d]
    projection (view 1 rows, then view 2 rows) and the gradient comes back as one [2n, d] tensor."""

    @staticmethod
    def forward(ctx, z1, z2, labels, w11, w22, w12, blocks, mask_semantics, in_mode, t, state):
        stacked = z2 is None
        _n.require_gpu(z1, z2, labels, w11, w22, w12)
        z1c = z1.detach().contiguous().float()
        if stacked:
            assert z1c.dim() == 2 and z1c.shape[0] % 2 == 0, z1c.shape
            n, d = z1c.shape[0] // 2, z1c.shape[1]
            z1c, z2c = z1c[:n], z1c[n:]
        else:
            z2c = z2.detach().contiguous().float()
            n, d = z1c.shape
        nbytes = _n.call("spcl_supcon_weighted_workspace_bytes", n, d)
        if nbytes == 0:
            raise RuntimeError(f"supcon (weighted): unsupported shape n={n} d={d} (n <= 4096, d <= 4096)")
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=z1.device)
        out = torch.empty(8, dtype=torch.float32, device=z1.device)
        _n.call("spcl_supcon_weighted_forward", _n.ptr(z1c), _n.ptr(z2c), _n.ptr(labels), _n.ptr(w11), _n.ptr(w22),
                _n.ptr(w12), blocks, int(mask_semantics), int(in_mode), n, d, c_float(t), _n.ptr(ws), _n.ptr(out),
                _n.stream())
        state.n, state.d, state.t, state.z1, state.z2 = n, d, t, z1c, z2c
        state.labels, state.w11, state.w22, state.w12 = labels, w11, w22, w12
        state.blocks, state.mask_semantics, state.ws, state.out = blocks, int(mask_semantics), ws, out
        ctx.state = state
        ctx.stacked = stacked
        ctx.in_dtypes = (z1.dtype, z1.dtype if stacked else z2.dtype)
        ctx.leaf_input = bool(z1.is_leaf or (z2 is not None and z2.is_leaf))
        return out[0]

    @staticmethod
    def backward(ctx, grad_out):
        s = ctx.state
        n, d = s.n, s.d
        tail = (None,) * 9
        if (2 * n <= _WEIGHTED_UNIT_ROWS and d <= _WEIGHTED_UNIT_D and is_unit_gradient(grad_out)
                and all(dt == torch.float32 for dt in ctx.in_dtypes)):
            # the forward already left dLoss/dz for a unit gradient at the start of its workspace: that block IS the gradient
            dz = s.ws[:2 * n * d].view(2 * n, d)
            if ctx.leaf_input:  # (a leaf keeps what it is handed as its .grad: it must own it)
                dz = dz.clone()
            return ((dz, None) if ctx.stacked else (dz[:n], dz[n:])) + tail
        dz = torch.empty(2 * n, d, dtype=torch.float32, device=s.ws.device)
        go = grad_out.detach().reshape(1).float().contiguous()
        _n.call("spcl_supcon_weighted_backward", _n.ptr(s.z1), _n.ptr(s.z2), n, d, c_float(s.t), _n.ptr(s.ws), _n.ptr(go),
                _n.ptr(dz[:n]), _n.ptr(dz[n:]), _n.stream())
        if ctx.stacked:
            return (dz.to(ctx.in_dtypes[0]), None) + tail
        return (dz[:n].to(ctx.in_dtypes[0]), dz[n:].to(ctx.in_dtypes[1])) + tail


def supcon_weighted_loss(z1, z2, *, labels=None, w11=None, w22=None, w12=None, mask_semantics=False, in_mode=False,
                         t=0.07, state: SupConWeightedState = None):
    """loss (0-dim tensor with grad_fn) of the (P, E) criterion of csrc/supcon_weighted.hip.  ``labels`` [n] float32, or up to
    three contiguous float32 [n, n] blocks -- ``w11`` block (1,1), ``w22`` block (2,2), ``w12`` blocks (1,2) and (2,1): a
    pair in a block that is not given has no weight and is not in the denominator.  ``z2=None``: z1 holds both halves
    stacked (``stacked_halves``).  The weights receive no gradient."""
    if state is None:
        state = SupConWeightedState()
    blocks = (1 if w11 is not None else 0) | (2 if w22 is not None else 0) | (4 if w12 is not None else 0)
    return _SupConWeightedFn.apply(z1, z2, labels, w11, w22, w12, blocks, bool(mask_semantics), bool(in_mode), float(t),
                                   state)


def supcon_weighted_materialize(state: SupConWeightedState, want=("sim_logits", "sim_exp", "pos_weight", "enable_mask")):
    n2 = 2 * state.n
    dev = state.ws.device
    bufs = {k: (torch.empty(n2, n2, dtype=torch.float32, device=dev) if k in want else None)
            for k in ("sim_logits", "sim_exp", "pos_weight", "enable_mask")}
    _n.call("spcl_supcon_weighted_materialize", _n.ptr(state.z1), _n.ptr(state.z2), _n.ptr(state.labels), _n.ptr(state.w11),
            _n.ptr(state.w22), _n.ptr(state.w12), state.blocks, state.mask_semantics, state.n, state.d, c_float(state.t),
            _n.ptr(state.ws), _n.ptr(bufs["sim_logits"]), _n.ptr(bufs["sim_exp"]), _n.ptr(bufs["pos_weight"]),
            _n.ptr(bufs["enable_mask"]), _n.stream())
    return bufs


def stacked_halves(a: torch.Tensor, b: torch.Tensor):
    """the tensor whose first / second half of rows a and b are (``torch.chunk(z, 2)`` outputs), else None"""
    base = a._base
    if (base is None or base is not b._base or a.dim() != 2 or a.shape != b.shape or base.dim() != 2
            or not base.is_contiguous() or base.shape[0] != 2 * a.shape[0] or base.shape[1] != a.shape[1]
            or a.stride() != base.stride() or b.stride() != base.stride()
            or a.storage_offset() != base.storage_offset() or b.storage_offset() != a.storage_offset() + a.numel()):
        return None
    return base


def supcon_materialize(state: SupConState, want=("sim_logits", "sim_exp", "pos_mask", "neg_mask", "sp_mask")):
    n2 = 2 * state.n
    dev = state.ws.device
    bufs = {k: (torch.empty(n2, n2, dtype=torch.float32, device=dev) if k in want else None)
            for k in ("sim_logits", "sim_exp", "pos_mask", "neg_mask", "sp_mask")}
    _n.call("spcl_supcon_materialize", _n.ptr(state.labels), _n.ptr(state.mask), state.n, state.d, c_float(state.t),
            state.sp_mode, c_float(state.gamma), _n.ptr(state.ws), _n.ptr(bufs["sim_logits"]),
            _n.ptr(bufs["sim_exp"]), _n.ptr(bufs["pos_mask"]), _n.ptr(bufs["neg_mask"]), _n.ptr(bufs["sp_mask"]),
            _n.stream())
    return bufs


# --------------------------------------------------------------------------------------------- NHWC plumbing
def as_nhwc(t: torch.Tensor):
    """Return (storage, Cs) where storage is a contiguous [N,H,W,Cs] tensor aliasing (or copying) the logical
    NCHW tensor ``t``.  Zero-copy when ``t`` already is channels-last (optionally channel-padded)."""
    assert t.dim() == 4
    N, C, H, W = t.shape
    sN, sC, sH, sW = t.stride()
    if sC == 1 and sW >= C and sH == W * sW and sN == H * W * sW and t.dtype in (torch.float32, torch.bfloat16):
        cs = sW
        if cs == C:
            return t.permute(0, 2, 3, 1), cs
        base = torch.as_strided(t, (N, H, W, cs), (sN, sH, sW, 1))
        return base, cs
    if t.dtype not in (torch.float32, torch.bfloat16):
        t = t.float()
    t = t.contiguous(memory_format=torch.channels_last)
    return t.permute(0, 2, 3, 1), C


def nhwc_to_logical(storage: torch.Tensor, C: int):
    """[N,H,W,Cs] storage -> logical NCHW view with C channels (channels-last strides, no copy)."""
    v = storage.permute(0, 3, 1, 2)
    return v if storage.shape[3] == C else v[:, :C]


# --------------------------------------------------------------------------------------------- projector
class _ProjectorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, w1, b1, w2, b2, normalize):
        _n.require_gpu(feat, w1, b1, w2, b2)
        x, cs = as_nhwc(feat.detach())
        N, H, W, _ = x.shape
        C = feat.shape[1]
        dev = feat.device
        mlp = w2 is not None
        hid = w1.shape[0] if mlp else 0
        out_dim = w2.shape[0] if mlp else w1.shape[0]
        w1c, b1c = w1.detach().contiguous().float(), b1.detach().contiguous().float()
        w2c = w2.detach().contiguous().float() if mlp else None
        b2c = b2.detach().contiguous().float() if mlp else None
        gap = _gap_of(feat, N, C) if H * W > 1 else None  # (the rows the feature map's producer left: no pooling launch)
        pooled = gap if gap is not None else torch.empty(N, C, dtype=torch.float32, device=dev)
        pre = torch.empty(N, hid, dtype=torch.float32, device=dev) if mlp else None
        o = torch.empty(N, out_dim, dtype=torch.float32, device=dev)
        z = torch.empty(N, out_dim, dtype=torch.float32, device=dev) if normalize else o  # (no copy without normalisation)
        _n.call("spcl_proj_forward", None if gap is not None else _n.ptr(x), _n.dtype_code(x.dtype), N, H * W, C, cs, _n.ptr(w1c), _n.ptr(b1c),
                _n.ptr(w2c), _n.ptr(b2c), hid, out_dim, int(bool(normalize)), _n.ptr(pooled), _n.ptr(pre), _n.ptr(o),
                _n.ptr(z), _n.stream())
        # (without normalisation the output IS o: the backward does not read it then, and an output must not be saved raw)
        ctx.save_for_backward(w1c, w2c, pooled, pre, o if normalize else None)
        ctx.meta = (N, H, W, C, cs, hid, out_dim, bool(normalize), x.dtype, feat.dtype)
        ctx.params = (w1, b1, w2, b2)  # their gradient sinks are claimed in backward, where the kernels write
        return z

    @staticmethod
    def backward(ctx, dz):
        w1c, w2c, pooled, pre, o = ctx.saved_tensors
        N, H, W, C, cs, hid, out_dim, normalize, xdt, fdt = ctx.meta
        dev = dz.device
        mlp = hid > 0
        dzc = dz.detach().contiguous().float()
        ng = ctx.needs_input_grad
        sk = tuple(take_grad_sink(p, ng[i + 1]) for i, p in enumerate(ctx.params))
        dw1 = _grad_buffer(sk[0], w1c.shape, dev)
        db1 = _grad_buffer(sk[1], (w1c.shape[0],), dev)
        dw2 = _grad_buffer(sk[2], w2c.shape, dev) if mlp else None
        db2 = _grad_buffer(sk[3], (out_dim,), dev) if mlp else None
        scratch = torch.empty(N * (out_dim + hid + C), dtype=torch.float32, device=dev)
        need_dfeat = ctx.needs_input_grad[0]
        if need_dfeat and _BCAST and cs == C and H * W > 1 and xdt == fdt:
            # the gradient of the global average pool as what it is -- one value per (image, channel) -- behind a stride-0
            # view: the block it came from reads the [N, C] form (broadcast_rows), anything else sees an ordinary tensor
            dnc = torch.empty(N, C, dtype=xdt, device=dev)
            one = lambda t: _n.ptr_array([t])  # noqa: E731
            _n.call("spcl_proj_heads_backward_pooled", 1, one(dzc), _n.dtype_code(xdt), N, H * W, C, cs, one(w1c), one(w2c),
                    hid, out_dim, int(normalize), _n.ptr(pooled), one(pre), one(o), one(dw1), one(db1), one(dw2), one(db2),
                    _n.ptr(scratch), _n.ptr(dnc), _n.stream())
            return dnc.view(N, C, 1, 1).expand(N, C, H, W), dw1, db1, dw2, db2, None
        dfeat = torch.empty(N, H, W, cs, dtype=xdt, device=dev) if need_dfeat else None
        _n.call("spcl_proj_backward", _n.ptr(dzc), _n.dtype_code(xdt), N, H * W, C, cs, _n.ptr(w1c), _n.ptr(w2c), hid,
                out_dim, int(normalize), _n.ptr(pooled), _n.ptr(pre), _n.ptr(o), _n.ptr(dw1), _n.ptr(db1),
                _n.ptr(dw2), _n.ptr(db2), _n.ptr(scratch), _n.ptr(dfeat), _n.stream())
        gfeat = None
        if need_dfeat:
            gfeat = nhwc_to_logical(dfeat, C)
            if gfeat.dtype != fdt:
                gfeat = gfeat.to(fdt)
        return gfeat, dw1, db1, dw2, db2, None


def projector(feat, w1, b1, w2=None, b2=None, normalize=True):
    return _ProjectorFn.apply(feat, w1, b1, w2, b2, normalize)


class _ProjectorHeadsFn(torch.autograd.Function):
    """K <= 4 MLP heads of identical shape on the SAME feature (several meta-label hooks on one encoder tap): the feature is
    pooled once and every layer of all heads is one launch (spcl_proj_heads_forward / _backward).  Inputs: feat, normalize,
    then (w1, b1, w2, b2) per head; outputs: one z [N, out] per head."""

    @staticmethod
    def forward(ctx, feat, normalize, *params):
        K = len(params) // 4
        heads = [params[4 * k:4 * k + 4] for k in range(K)]
        _n.require_gpu(feat, *params)
        x, cs = as_nhwc(feat.detach())
        N, H, W, _ = x.shape
        C = feat.shape[1]
        dev = feat.device
        hid, out_dim = heads[0][0].shape[0], heads[0][2].shape[0]
        cont = [[t.detach().contiguous().float() for t in h] for h in heads]
        gap = _gap_of(feat, N, C) if H * W > 1 else None
        pooled = gap if gap is not None else torch.empty(N, C, dtype=torch.float32, device=dev)
        pre = torch.empty(K, N, hid, dtype=torch.float32, device=dev)
        o = torch.empty(K, N, out_dim, dtype=torch.float32, device=dev)
        # back to back: the batched loss reads them in place (without normalisation the heads' rows are the output: no copy)
        z = list((torch.empty(K, N, out_dim, dtype=torch.float32, device=dev) if normalize else o).unbind(0))
        col = lambda i: _n.ptr_array([c[i] for c in cont])  # noqa: E731
        _n.call("spcl_proj_heads_forward", K, None if gap is not None else _n.ptr(x), _n.dtype_code(x.dtype), N, H * W, C, cs, col(0), col(1), col(2),
                col(3), hid, out_dim, int(bool(normalize)), _n.ptr(pooled), _n.ptr_array(list(pre)), _n.ptr_array(list(o)),
                _n.ptr_array(z), _n.stream())
        ctx.save_for_backward(pooled, pre, o if normalize else None, *[c[0] for c in cont], *[c[2] for c in cont])
        ctx.meta = (K, N, H, W, C, cs, hid, out_dim, bool(normalize), x.dtype, feat.dtype)
        ctx.params = params
        return tuple(z)

    @staticmethod
    def backward(ctx, *dzs):
        K, N, H, W, C, cs, hid, out_dim, normalize, xdt, fdt = ctx.meta
        saved = ctx.saved_tensors
        pooled, pre, o = saved[:3]
        o = [None] * K if o is None else list(o)  # (without normalisation the backward does not read the rows)
        w1s, w2s = saved[3:3 + K], saved[3 + K:3 + 2 * K]
        dev = pooled.device
        dzc = [torch.zeros(N, out_dim, dtype=torch.float32, device=dev) if g is None else g.detach().contiguous().float()
               for g in dzs]
        ng = ctx.needs_input_grad
        sk = [take_grad_sink(p, ng[i + 2]) for i, p in enumerate(ctx.params)]
        shapes = ((hid, C), (hid,), (out_dim, hid), (out_dim,))
        grads = [_grad_buffer(sk[i], shapes[i % 4], dev) for i in range(4 * K)]
        scratch = torch.empty(K * N * (out_dim + hid) + N * C, dtype=torch.float32, device=dev)
        need_dfeat = ng[0]
        col = lambda i: _n.ptr_array([grads[4 * k + i] for k in range(K)])  # noqa: E731
        if need_dfeat and _BCAST and cs == C and H * W > 1 and xdt == fdt:  # (see _ProjectorFn.backward)
            dnc = torch.empty(N, C, dtype=xdt, device=dev)
            _n.call("spcl_proj_heads_backward_pooled", K, _n.ptr_array(dzc), _n.dtype_code(xdt), N, H * W, C, cs,
                    _n.ptr_array(list(w1s)), _n.ptr_array(list(w2s)), hid, out_dim, int(normalize), _n.ptr(pooled),
                    _n.ptr_array(list(pre)), _n.ptr_array(o), col(0), col(1), col(2), col(3), _n.ptr(scratch),
                    _n.ptr(dnc), _n.stream())
            return (dnc.view(N, C, 1, 1).expand(N, C, H, W), None) + tuple(grads)
        dfeat = torch.empty(N, H, W, cs, dtype=xdt, device=dev) if need_dfeat else None
        _n.call("spcl_proj_heads_backward", K, _n.ptr_array(dzc), _n.dtype_code(xdt), N, H * W, C, cs, _n.ptr_array(list(w1s)),
                _n.ptr_array(list(w2s)), hid, out_dim, int(normalize), _n.ptr(pooled), _n.ptr_array(list(pre)),
                _n.ptr_array(o), col(0), col(1), col(2), col(3), _n.ptr(scratch), _n.ptr(dfeat), _n.stream())
        gfeat = None
        if need_dfeat:
            gfeat = nhwc_to_logical(dfeat, C)
            if gfeat.dtype != fdt:
                gfeat = gfeat.to(fdt)
        return (gfeat, None) + tuple(grads)


def projector_heads(feat, heads, normalize=True):
    """``heads``: list of (w1, b1, w2, b2) of identical shapes (at most 4) -> list of z [N, out], one per head"""
    flat = [t for h in heads for t in h]
    return list(_ProjectorHeadsFn.apply(feat, normalize, *flat))


class _FlipBatchFn(torch.autograd.Function):
    """per-sample H / W flips of an [N,C,H,W] batch (spcl_flip_batch); a flip is its own inverse, so is its gradient"""

    @staticmethod
    def forward(ctx, x, flags):
        xc = x.detach().contiguous()
        out = torch.empty_like(xc)
        N, C, H, W = xc.shape
        _n.call("spcl_flip_batch", _n.ptr(xc), _n.ptr(out), xc.element_size(), N, C, H, W, _n.ptr(flags), _n.stream())
        ctx.flags = flags
        return out

    @staticmethod
    def backward(ctx, g):
        gc = g.contiguous()
        out = torch.empty_like(gc)
        N, C, H, W = gc.shape
        _n.call("spcl_flip_batch", _n.ptr(gc), _n.ptr(out), gc.element_size(), N, C, H, W, _n.ptr(ctx.flags), _n.stream())
        return out, None


def flip_batch(x, flags):
    """differentiable form of TensorRandomFlip.apply_batch: ``flags`` uint8 [N] (bit 0 flip H, bit 1 flip W)"""
    return _FlipBatchFn.apply(x, flags)


class _AdaptivePoolFn(torch.autograd.Function):
    """nn.AdaptiveAvgPool2d / nn.AdaptiveMaxPool2d((oh, ow)) on NHWC storage -> f32 logical [N,C,oh,ow]"""

    @staticmethod
    def forward(ctx, x, out_hw, mode):
        _n.require_gpu(x)
        xs, cs = as_nhwc(x.detach())
        N, H, W, _ = xs.shape
        C = x.shape[1]
        oh, ow = out_hw
        out = torch.empty(N, oh, ow, C, dtype=torch.float32, device=x.device)
        arg = torch.empty(N, oh, ow, C, dtype=torch.int32, device=x.device) if mode == 1 else None
        _n.call("spcl_adaptive_pool2d_forward", _n.ptr(xs), _n.dtype_code(xs.dtype), N, H, W, C, cs, oh, ow, mode,
                _n.ptr(out), _n.ptr(arg), _n.stream())
        ctx.arg = arg
        ctx.meta = (N, H, W, C, cs, oh, ow, mode, xs.dtype, x.dtype)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dout):
        N, H, W, C, cs, oh, ow, mode, sdt, xdt = ctx.meta
        do = _class_map_storage(dout)
        dx = torch.empty(N, H, W, cs, dtype=sdt, device=dout.device)
        _n.call("spcl_adaptive_pool2d_backward", _n.ptr(do), _n.ptr(ctx.arg), _n.dtype_code(sdt), N, H, W, C, cs, oh, ow,
                mode, _n.ptr(dx), _n.stream())
        g = nhwc_to_logical(dx, C)
        return (g if g.dtype == xdt else g.to(xdt)), None, None


def adaptive_pool2d(x, out_hw, mode="avg"):
    return _AdaptivePoolFn.apply(x, (int(out_hw[0]), int(out_hw[1])), 1 if mode == "max" else 0)


class _L2NormChannelsFn(torch.autograd.Function):
    """F.normalize(x, p=2, dim=1) of a logical [N,C,H,W] f32 map with NHWC storage (rows = pixels)"""

    @staticmethod
    def forward(ctx, x):
        _n.require_gpu(x)
        xs = _class_map_storage(x.detach())
        N, H, W, C = xs.shape
        z = torch.empty_like(xs)
        _n.call("spcl_l2norm_rows_forward", _n.ptr(xs), N * H * W, C, _n.ptr(z), _n.stream())
        ctx.save_for_backward(xs)
        return z.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dz):
        (xs,) = ctx.saved_tensors
        N, H, W, C = xs.shape
        dzs = _class_map_storage(dz)
        dx = torch.empty_like(xs)
        _n.call("spcl_l2norm_rows_backward", _n.ptr(xs), _n.ptr(dzs), N * H * W, C, _n.ptr(dx), _n.stream())
        return dx.permute(0, 3, 1, 2)


def l2norm_channels(x):
    return _L2NormChannelsFn.apply(x)


class _L2NormRowsFn(torch.autograd.Function):
    """F.normalize(x, p=2, dim=1) of [rows, d] f32 rows (projectors/nn.py:29-36)"""

    @staticmethod
    def forward(ctx, x):
        _n.require_gpu(x)
        xc = x.detach().contiguous().float()
        z = torch.empty_like(xc)
        _n.call("spcl_l2norm_rows_forward", _n.ptr(xc), xc.shape[0], xc.shape[1], _n.ptr(z), _n.stream())
        ctx.save_for_backward(xc)
        ctx.in_dtype = x.dtype
        return z

    @staticmethod
    def backward(ctx, dz):
        (xc,) = ctx.saved_tensors
        dx = torch.empty_like(xc)
        _n.call("spcl_l2norm_rows_backward", _n.ptr(xc), _n.ptr(dz.detach().contiguous().float()), xc.shape[0], xc.shape[1],
                _n.ptr(dx), _n.stream())
        return dx.to(ctx.in_dtype)


def l2norm_rows(x):
    assert x.dim() == 2, x.shape
    return _L2NormRowsFn.apply(x)


class _PixelMlpFn(torch.autograd.Function):
    """The dense projector's 1x1-conv MLP on every pixel as matrix products over the N*H*W pixel rows (csrc/rows_mlp.hip:
    exact-f32 MFMA; forward, input gradient, weight gradient with a fixed-order fold).  The feature map is read in place
    (channels-last rows of pitch ``cs``), the hidden pre-activation is the only tensor kept for backward."""

    @staticmethod
    def forward(ctx, feat, w1, b1, w2, b2):
        _n.require_gpu(feat, w1, b1, w2, b2)
        x, cs = as_nhwc(feat.detach())
        N, H, W, _ = x.shape
        C, M, dev = feat.shape[1], N * H * W, feat.device
        mlp = w2 is not None
        w1c, b1c = w1.detach().reshape(w1.shape[0], -1).contiguous().float(), b1.detach().contiguous().float()
        first = torch.empty(M, w1c.shape[0], dtype=torch.float32, device=dev)  # pre-activation (mlp) or the output (linear)
        _n.call("spcl_rows_linear_forward", _n.ptr(x), _n.dtype_code(x.dtype), cs, 0, _n.ptr(w1c), _n.ptr(b1c), M, C,
                w1c.shape[0], _n.ptr(first), _n.stream())
        w2c = None
        out = first
        if mlp:
            w2c, b2c = w2.detach().reshape(w2.shape[0], -1).contiguous().float(), b2.detach().contiguous().float()
            out = torch.empty(M, w2c.shape[0], dtype=torch.float32, device=dev)
            _n.call("spcl_rows_linear_forward", _n.ptr(first), _n.dtype_code(torch.float32), w1c.shape[0], 1, _n.ptr(w2c),
                    _n.ptr(b2c), M, w1c.shape[0], w2c.shape[0], _n.ptr(out), _n.stream())
        ctx.save_for_backward(x, w1c, w2c, first if mlp else None)
        ctx.meta = (N, H, W, C, cs, x.dtype, feat.dtype)
        ctx.params = (w1, b1, w2, b2)
        return out.view(N, H, W, out.shape[1]).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dout):
        x, w1c, w2c, pre = ctx.saved_tensors
        N, H, W, C, cs, xdt, fdt = ctx.meta
        M, dev = N * H * W, dout.device
        mlp = w2c is not None
        g = _class_map_storage(dout.detach())  # [N, H, W, O] f32, contiguous
        g = g.view(M, g.shape[3])
        ng = ctx.needs_input_grad
        sk = tuple(take_grad_sink(p, ng[i + 1]) for i, p in enumerate(ctx.params))
        hid = w1c.shape[0]
        dw1 = _grad_buffer(sk[0], (hid, C), dev)
        db1 = _grad_buffer(sk[1], (hid,), dev)
        dw2 = db2 = None

        def wgrad(gm, xin, xdtype, ldx, leaky, n_out, k_in, dw, db):
            ws = torch.empty(_n.call("spcl_rows_linear_backward_weight_workspace_bytes", M, n_out, k_in) // 4 + 1,
                             dtype=torch.float32, device=dev)
            _n.call("spcl_rows_linear_backward_weight", _n.ptr(gm), _n.dtype_code(gm.dtype), _n.ptr(xin), _n.dtype_code(xdtype), ldx,
                    int(leaky), M, n_out, k_in, _n.ptr(ws), ws.numel() * 4, _n.ptr(dw), _n.ptr(db), _n.stream())

        if mlp:
            O = w2c.shape[0]
            dw2 = _grad_buffer(sk[2], (O, hid), dev)
            db2 = _grad_buffer(sk[3], (O,), dev)
            wgrad(g, pre, torch.float32, hid, True, O, hid, dw2, db2)
            dpre = torch.empty(M, hid, dtype=torch.float32, device=dev)
            _n.call("spcl_rows_linear_backward_input", _n.ptr(g), _n.dtype_code(g.dtype), _n.ptr(w2c), _n.ptr(pre), M, O, hid,
                    _n.ptr(dpre), _n.dtype_code(torch.float32), hid, _n.stream())
            g = dpre
        wgrad(g, x, xdt, cs, False, hid, C, dw1, db1)
        gfeat = None
        if ng[0]:
            dfeat = (torch.zeros if cs != C else torch.empty)(N, H, W, cs, dtype=xdt, device=dev)
            _n.call("spcl_rows_linear_backward_input", _n.ptr(g), _n.dtype_code(g.dtype), _n.ptr(w1c), None, M, hid, C, _n.ptr(dfeat),
                    _n.dtype_code(xdt), cs, _n.stream())
            gfeat = nhwc_to_logical(dfeat, C)
            if gfeat.dtype != fdt:
                gfeat = gfeat.to(fdt)
        return gfeat, dw1.view(ctx.params[0].shape), db1, None if dw2 is None else dw2.view(ctx.params[2].shape), db2


class _PixelMlpPooledFn(torch.autograd.Function):
    """``adaptive_avg_pool(conv2(leaky(conv1(x))))`` of the dense projector computed as ``conv2(adaptive_avg_pool(leaky(conv1(x))))``:
    the second 1x1 convolution is linear (bias included: an average of a constant is the constant), so it commutes with the
    average pooling and runs on the N * oh * ow pooled rows instead of the N * H * W pixels -- 31x fewer rows for a 56^2 map
    pooled to 10^2, 125x for 112^2; the products of the wide layer (hid x out) and its full-size output disappear.  Same
    function; the sums are associated differently (differences at the 1e-7 level, tests/test_gpu_round2_heads.py)."""

    @staticmethod
    def forward(ctx, feat, w1, b1, w2, b2, out_hw):
        _n.require_gpu(feat, w1, b1, w2, b2)
        x, cs = as_nhwc(feat.detach())
        N, H, W, _ = x.shape
        C, M, dev = feat.shape[1], N * H * W, feat.device
        oh, ow = out_hw
        f32 = _n.dtype_code(torch.float32)
        w1c, b1c = w1.detach().reshape(w1.shape[0], -1).contiguous().float(), b1.detach().contiguous().float()
        w2c, b2c = w2.detach().reshape(w2.shape[0], -1).contiguous().float(), b2.detach().contiguous().float()
        hid, O = w1c.shape[0], w2c.shape[0]
        # LeakyReLU(conv1(x)): the one full-size tensor kept -- in the feature map's own dtype (3.1 GB as f32 for 60 maps of
        # 224^2: the head's launches are streams of this tensor)
        h = torch.empty(M, hid, dtype=x.dtype, device=dev)
        _n.call("spcl_rows_linear_forward_act", _n.ptr(x), _n.dtype_code(x.dtype), cs, _n.ptr(w1c), _n.ptr(b1c), M, C, hid,
                _n.ptr(h), _n.dtype_code(h.dtype), _n.stream())
        hp = torch.empty(N * oh * ow, hid, dtype=torch.float32, device=dev)
        _n.call("spcl_adaptive_pool2d_forward", _n.ptr(h), _n.dtype_code(h.dtype), N, H, W, hid, hid, oh, ow, 0, _n.ptr(hp), None,
                _n.stream())
        out = torch.empty(N * oh * ow, O, dtype=torch.float32, device=dev)
        _n.call("spcl_rows_linear_forward", _n.ptr(hp), f32, hid, 0, _n.ptr(w2c), _n.ptr(b2c), N * oh * ow, hid, O, _n.ptr(out),
                _n.stream())
        ctx.save_for_backward(x, h, hp, w1c, w2c)
        ctx.meta = (N, H, W, C, cs, oh, ow, x.dtype, feat.dtype)
        ctx.params = (w1, b1, w2, b2)
        return out.view(N, oh, ow, O).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dout):
        x, h, hp, w1c, w2c = ctx.saved_tensors
        N, H, W, C, cs, oh, ow, xdt, fdt = ctx.meta
        M, Mp, dev = N * H * W, N * oh * ow, dout.device
        hid, O = w1c.shape[0], w2c.shape[0]
        f32 = _n.dtype_code(torch.float32)
        g = _class_map_storage(dout.detach()).view(Mp, O)
        ng = ctx.needs_input_grad
        sk = tuple(take_grad_sink(p, ng[i + 1]) for i, p in enumerate(ctx.params))
        dw1, db1 = _grad_buffer(sk[0], (hid, C), dev), _grad_buffer(sk[1], (hid,), dev)
        dw2, db2 = _grad_buffer(sk[2], (O, hid), dev), _grad_buffer(sk[3], (O,), dev)

        def wgrad(gm, rows, xin, xdtype, ldx, n_out, k_in, dw, db):
            ws = torch.empty(_n.call("spcl_rows_linear_backward_weight_workspace_bytes", rows, n_out, k_in) // 4 + 1,
                             dtype=torch.float32, device=dev)
            _n.call("spcl_rows_linear_backward_weight", _n.ptr(gm), _n.dtype_code(gm.dtype), _n.ptr(xin), _n.dtype_code(xdtype), ldx, 0,
                    rows, n_out, k_in, _n.ptr(ws), ws.numel() * 4, _n.ptr(dw), _n.ptr(db), _n.stream())

        wgrad(g, Mp, hp, torch.float32, hid, O, hid, dw2, db2)
        dhp = torch.empty(Mp, hid, dtype=torch.float32, device=dev)
        _n.call("spcl_rows_linear_backward_input", _n.ptr(g), f32, _n.ptr(w2c), None, Mp, O, hid, _n.ptr(dhp), f32, hid, _n.stream())
        dpre = torch.empty(M, hid, dtype=h.dtype, device=dev)  # un-pooled, through the LeakyReLU (h carries its sign)
        _n.call("spcl_adaptive_avgpool2d_backward_act", _n.ptr(dhp), _n.ptr(h), _n.dtype_code(h.dtype), N, H, W, hid, oh, ow,
                _n.ptr(dpre), _n.stream())
        wgrad(dpre, M, x, xdt, cs, hid, C, dw1, db1)
        gfeat = None
        if ng[0]:
            dfeat = (torch.zeros if cs != C else torch.empty)(N, H, W, cs, dtype=xdt, device=dev)
            _n.call("spcl_rows_linear_backward_input", _n.ptr(dpre), _n.dtype_code(dpre.dtype), _n.ptr(w1c), None, M, hid, C,
                    _n.ptr(dfeat), _n.dtype_code(xdt), cs, _n.stream())
            gfeat = nhwc_to_logical(dfeat, C)
            if gfeat.dtype != fdt:
                gfeat = gfeat.to(fdt)
        return gfeat, dw1.view(ctx.params[0].shape), db1, dw2.view(ctx.params[2].shape), db2, None


class _GroupedLeakyLinearFn(torch.autograd.Function):
    """The second layers of S ``mlp`` cluster subheads on the column slices of their stacked pre-activation: ``out[:, s*K + k]
    = b2[s][k] + sum_h W2[s][k][h] LeakyReLU(pre[:, s*Hd + h])``.  S calls of the rows product (csrc/rows_mlp.hip), each reading
    its slice of ``pre`` through the row pitch with the activation applied as it is read; no block-diagonal weight is built.
    Backward: per subhead the weight gradient (same pitch and activation) and the unmasked input gradient written into its slice
    through the output pitch, then one pass applies LeakyReLU' to the whole [M, S*Hd] gradient.  The rows product takes output
    counts that are multiples of 4: another K is padded with zero rows (and zero gradient columns), forward and backward."""

    @staticmethod
    def forward(ctx, pre, w2, b2):
        _n.require_gpu(pre, w2, b2)
        ps = _class_map_storage(pre.detach())
        N, H, W, ld = ps.shape
        S, K, hid = w2.shape
        M, dev, f32 = N * H * W, ps.device, _n.dtype_code(torch.float32)
        if ld != S * hid or hid % 4:
            raise ValueError(f"grouped second layers: {S} subheads of {hid} hidden units (a multiple of 4) on {ld} columns")
        w2c, b2c = w2.detach().contiguous().float(), b2.detach().contiguous().float()
        Kp = (K + 3) // 4 * 4  # (the rows product takes output counts that are multiples of 4: zero rows behind K)
        wp, bp = w2c, b2c
        if Kp != K:
            wp, bp = w2c.new_zeros(S, Kp, hid), b2c.new_zeros(S, Kp)
            wp[:, :K], bp[:, :K] = w2c, b2c
        out = torch.empty(M, S * K, dtype=torch.float32, device=dev)
        ys = torch.empty(M, Kp, dtype=torch.float32, device=dev)
        for s in range(S):
            _n.call("spcl_rows_linear_forward", ctypes.c_void_p(ps.data_ptr() + 4 * s * hid), f32, ld, 1, _n.ptr(wp[s]),
                    _n.ptr(bp[s]), M, hid, Kp, _n.ptr(ys), _n.stream())
            out[:, s * K:(s + 1) * K] = ys[:, :K]
        ctx.save_for_backward(ps, w2c)
        ctx.params = (w2, b2)
        return out.view(N, H, W, S * K).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dout):
        ps, w2c = ctx.saved_tensors
        N, H, W, ld = ps.shape
        S, K, hid = w2c.shape
        M, dev, f32 = N * H * W, ps.device, _n.dtype_code(torch.float32)
        Kp = (K + 3) // 4 * 4
        g = _class_map_storage(dout.detach()).view(M, S * K)
        ng = ctx.needs_input_grad
        sk = tuple(take_grad_sink(p, ng[i + 1]) for i, p in enumerate(ctx.params))
        dw2, db2 = _grad_buffer(sk[0], (S, K, hid), dev), _grad_buffer(sk[1], (S, K), dev)
        gs = torch.zeros(M, Kp, dtype=torch.float32, device=dev)
        wp = torch.zeros(Kp, hid, dtype=torch.float32, device=dev)
        dwp, dbp = torch.empty(Kp, hid, dtype=torch.float32, device=dev), torch.empty(Kp, dtype=torch.float32, device=dev)
        dact = torch.empty(M, ld, dtype=torch.float32, device=dev)
        ws = torch.empty(_n.call("spcl_rows_linear_backward_weight_workspace_bytes", M, Kp, hid) // 4 + 1, dtype=torch.float32,
                         device=dev)
        for s in range(S):
            gs[:, :K] = g[:, s * K:(s + 1) * K]
            wp[:K] = w2c[s]
            slice_ptr = ctypes.c_void_p(ps.data_ptr() + 4 * s * hid)
            _n.call("spcl_rows_linear_backward_weight", _n.ptr(gs), f32, slice_ptr, f32, ld, 1, M, Kp, hid, _n.ptr(ws),
                    ws.numel() * 4, _n.ptr(dwp), _n.ptr(dbp), _n.stream())
            dw2[s] = dwp[:K]
            db2[s] = dbp[:K]
            _n.call("spcl_rows_linear_backward_input", _n.ptr(gs), f32, _n.ptr(wp), None, M, Kp, hid,
                    ctypes.c_void_p(dact.data_ptr() + 4 * s * hid), f32, ld, _n.stream())
        dpre = None
        if ng[0]:
            # LeakyReLU'(pre) on every row at once: the masked un-pooling with one pixel a window is the identity times the mask
            dpre = torch.empty_like(ps)
            _n.call("spcl_adaptive_avgpool2d_backward_act", _n.ptr(dact), _n.ptr(ps), f32, M, 1, 1, ld, 1, 1, _n.ptr(dpre),
                    _n.stream())
            dpre = dpre.permute(0, 3, 1, 2)
        return dpre, dw2, db2


def cluster_mlp_logits(feat, w1, b1, w2, b2):
    """the logits of S ``mlp`` cluster subheads on a logical [N, C, H, W] map (contrastyou/projectors/heads.py:42-75 without
    the pooling, ``Normalize`` and softmax): ``w1`` [S*Hd, C(,1,1)] / ``b1`` [S*Hd] the stacked first layers -- one product --,
    LeakyReLU(0.01), ``w2`` [S, K, Hd] / ``b2`` [S, K] the second layers (``_GroupedLeakyLinearFn``) -> f32 logical
    [N, S*K, H, W]"""
    pre = pixelwise_mlp(feat, w1.reshape(w1.shape[0], -1, 1, 1), b1)
    return _GroupedLeakyLinearFn.apply(pre, w2, b2)


def pixelwise_mlp_pooled_supported(feat, w1, w2) -> bool:
    return bool(feat.is_cuda and w2 is not None and feat.shape[1] % 4 == 0 and w1.shape[0] % 4 == 0 and w2.shape[0] % 4 == 0)


def pixelwise_mlp_pooled(feat, w1, b1, w2, b2, out_hw):
    """``adaptive_avg_pool2d(pixelwise_mlp(feat, ...), out_hw)`` with the second layer applied AFTER the pooling (see
    ``_PixelMlpPooledFn``) -> f32 logical [N, O, oh, ow]"""
    return _PixelMlpPooledFn.apply(feat, w1, b1, w2, b2, tuple(int(v) for v in out_hw))


def pixelwise_mlp(feat, w1, b1, w2=None, b2=None):
    """1x1-conv MLP of ``get_contrastive_dense_projector`` (projectors/heads.py:28-39) on a logical [N,C,H,W] map:
    every pixel is a row (no pooling, no normalisation) -> f32 logical [N,O,H,W].
    ``w1`` [hid,C,1,1] (or [O,C,1,1] for the linear head), ``w2`` [O,hid,1,1].  Matrix products over the pixel rows
    (``_PixelMlpFn``) when the channel counts are multiples of 4 -- always, in the UNet --; else the rows go through the
    global projector's kernels (correct, and slow beyond a few thousand rows)."""
    dims = [feat.shape[1], w1.shape[0]] + ([w2.shape[0]] if w2 is not None else [])
    if feat.is_cuda and all(d % 4 == 0 for d in dims):
        return _PixelMlpFn.apply(feat, w1, b1, w2, b2)
    xs, cs = as_nhwc(feat)  # differentiable view ops only
    N, H, W, _ = xs.shape
    C = feat.shape[1]
    rows = torch.as_strided(xs, (N * H * W, C, 1, 1), (cs, 1, cs, cs), xs.storage_offset())
    o = projector(rows, w1.reshape(w1.shape[0], -1), b1, None if w2 is None else w2.reshape(w2.shape[0], -1), b2,
                  normalize=False)
    return o.view(N, H, W, o.shape[1]).permute(0, 3, 1, 2)


# --------------------------------------------------------------------------------------------- encoder blocks
def _ru16(c: int) -> int:
    return (c + 15) // 16 * 16


def to_nhwc_padded(x: torch.Tensor, dtype: torch.dtype):
    """logical NCHW -> contiguous [N,H,W,CS] storage of `dtype`, CS = C rounded up to 16 (pad channels = 0).
    Zero-copy when x already is such a view (what the fused blocks hand to each other)."""
    N, C, H, W = x.shape
    cs = _ru16(C)
    if x.dtype == dtype and cs == C:
        sN, sC, sH, sW = x.stride()
        if sC == 1 and sW == cs and sH == W * cs and sN == H * W * cs:
            return x.permute(0, 2, 3, 1)
    # (a channel count that is not a multiple of 16 is always re-padded: a narrow view cannot prove that the lanes
    # behind it hold zeros -- e.g. a channel slice of a concatenation's gradient)
    if cs == C:
        return x.to(dtype).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    out = torch.zeros(N, H, W, cs, dtype=dtype, device=x.device)
    out[..., :C] = x.permute(0, 2, 3, 1)
    return out


def nhwc_channel_slice(x, dtype):
    """``(view [N,H,W,C], S)`` when the logical NCHW tensor ``x`` is a 16-byte-aligned CHANNEL SLICE of a dense NHWC tensor of
    ``dtype`` with S > C channels per pixel (one half of a decoder concatenation's gradient, ``_VirtualCatFn``) -- what the
    ``_strided`` BatchNorm entry points read in place; else None (the caller re-packs)."""
    if x is None or x.dim() != 4 or x.dtype != dtype:
        return None
    N, C, H, W = x.shape
    sN, sC, sH, sW = x.stride()
    if sC != 1 or sW <= C or sW % 8 or C % 16 or sH != W * sW or sN != H * W * sW:
        return None
    if (x.storage_offset() * x.element_size()) % 16:
        return None
    return x.permute(0, 2, 3, 1), sW


def _bnrelu_fwd(y, dt_code, N, H, W, cs, scale, shift, act, pool):
    """BN-apply + ReLU (+ 2x2 max-pool) writer; ``act`` may be a channel slice of a wider NHWC tensor (pixel stride > cs)"""
    if act is not None and act.stride(2) != cs:
        _n.call("spcl_bnrelu_pool_forward_strided", _n.ptr(y), dt_code, N, H, W, cs, _n.ptr(scale), _n.ptr(shift),
                _n.ptr(act), int(act.stride(2)), _n.ptr(pool), _n.stream())
    else:
        _n.call("spcl_bnrelu_pool_forward", _n.ptr(y), dt_code, N, H, W, cs, _n.ptr(scale), _n.ptr(shift), _n.ptr(act),
                _n.ptr(pool), _n.stream())


def _act_buffer(cfg, N, H, W, cs, dtype, dev):
    """the block's activation output: the caller's destination (``cfg.act_dst``: its half of a concatenation buffer) when it
    fits, else a fresh dense tensor"""
    dst = getattr(cfg, "act_dst", None)
    if (dst is not None and tuple(dst.shape) == (N, H, W, cs) and dst.dtype == dtype and dst.device == dev
            and dst.stride(3) == 1 and dst.stride(2) % 8 == 0 and dst.stride(1) == W * dst.stride(2)
            and dst.stride(0) == H * W * dst.stride(2) and (dst.storage_offset() * dst.element_size()) % 16 == 0):
        return dst
    return torch.empty(N, H, W, cs, dtype=dtype, device=dev)


class PoolLink:
    """What the NEXT block's backward needs to leave the BatchNorm-backward partial sums of THIS block's second conv in the
    epilogue of its own input-gradient kernel (spcl_conv3x3_dgrad_poolstats): this block's raw second-conv output and BN
    coefficients.  The next block fills ``rows`` / ``dx_ptr``; this block's backward uses them if the pooled gradient it
    receives IS that kernel's output (same storage: nothing else contributed to it), else runs its own reduction pass."""
    __slots__ = ("yb", "stb", "N", "H", "W", "cout_s", "rows", "dx_ptr", "holder", "version", "acc", "ymax")

    def __init__(self, yb, stb, N, H, W, cout_s, acc=None, ymax=None):
        self.yb, self.stb, self.N, self.H, self.W, self.cout_s = yb, stb, N, H, W, cout_s
        # ``ymax``: [N, H/2, W/2, cout_s], the raw ``yb`` at each pooling window's first maximum (the pooled forward's side
        # output, ``_pool_ymax_pays``): the next block's dgrad reads it instead of ``yb`` (spcl_conv3x3_dgrad_poolmax)
        self.ymax = ymax
        # ``acc``: a zeroed fixed-point accumulator block (bn_acc_block) the next block's dgrad may ADD the sums to instead of
        # writing per-tile rows; ``rows`` is then ``ACC_ROWS`` and the apply pass derives its coefficients from the block
        self.acc = acc
        # ``holder``: the gradient tensor ``dx_ptr`` is the address of, kept alive until the consumer has compared -- a freed
        # tensor's address is the first thing the allocator hands out again (to the re-layout copy of a foreign gradient, say)
        self.rows, self.dx_ptr, self.holder, self.version = None, 0, None, 0

    def fresh(self, ptr):
        """is the gradient at ``ptr`` exactly the tensor the producer left (same storage, never accumulated into in place)?"""
        return self.rows is not None and ptr == self.dx_ptr and self.holder is not None and self.holder._version == self.version


def _pool_ymax_pays(N, H, W, cout_s):
    """Does the pooled forward of a block with raw output [N, H, W, cout_s] leave the window-maximum tensor for the next block's
    dgrad?  It pays where the dgrad's saved reads (3/4 of ``yb``) outweigh the extra 1/4-size store of the pooled forward.
    Measured per launch inside the replayed pre-train step (N = 64 bf16, one MI355X, parent -> this form, us;
    profiles/poolmax_timeline_{parent,branch}.txt):

        yb [N, H, W, C]          bytes      pooled forward     next block's dgrad    net
        64 x 224 x 224 x  16   102.8 MB     21.9 -> 25.6        37.0 -> 26.7        -6.6
        64 x 112 x 112 x  32    51.4 MB     11.6 -> 14.0        28.2 -> 24.4        -1.4
        64 x  56 x  56 x  64    25.7 MB      8.2 ->  9.0        18.9 -> 15.0        -3.1
        64 x  28 x  28 x 128    12.8 MB      6.3 ->  6.8        17.5 -> 13.9        -3.1

    Every measured level gains, so the rule is their range: from the smallest measured tensor up.  Below it nothing was
    measured (a tensor of a few MB is still in cache when the dgrad reads it: there is little traffic to save) and the
    full-tensor form stays."""
    return N * H * W * cout_s * 2 >= 12 * 2 ** 20


class ActLink:
    """A block whose activation has ONE consumer that applies the block's last BatchNorm + ReLU itself (``BlockCfg.lazy_act``:
    the 1x1 head, ``conv1x1_bn``): the raw second-conv output and the BN coefficients the consumer needs, and -- filled by
    the consumer's backward -- the BatchNorm-backward partial sums it left next to the activation gradient."""
    __slots__ = ("yb", "stb", "N", "H", "W", "C", "cs", "rows", "dx_ptr", "holder", "version")

    def __init__(self, yb, stb, N, H, W, C, cs):
        self.yb, self.stb, self.N, self.H, self.W, self.C, self.cs = yb, stb, N, H, W, C, cs
        self.rows, self.dx_ptr, self.holder, self.version = None, 0, None, 0  # (holder / version: see PoolLink)

    fresh = PoolLink.fresh


class UpLink:
    """Between a block whose activation has ONE consumer -- an up-convolution reading it at half resolution
    (``BlockCfg.up_in``) -- and that consumer: the consumer's backward leaves the FINE input gradient here instead of summing
    its 2 x 2 windows, and returns a shared half-resolution tensor of ZEROS whose address the block recognises; the block's
    BatchNorm-backward reduction pass forms the sums on its way (spcl_bnrelu_backward_up2).  A gradient that arrives at the
    block with any other address means somebody else contributed to it (zeros + their gradient): the block then adds the
    2 x 2 sums itself with the ordinary kernels."""
    __slots__ = ("d_up", "dx_ptr", "holder", "version")

    def __init__(self):
        self.d_up, self.dx_ptr, self.holder, self.version = None, 0, None, 0


class BlockCfg:
    """Static configuration of one fused Conv-BN-ReLU(-Conv-BN-ReLU)(-MaxPool) block call."""
    __slots__ = ("dtype", "training", "momentum", "eps", "track", "need_act", "need_pool", "image_input", "buffers",
                 "link_in", "link_out", "act_dst", "up2", "lazy_act", "link_act", "x2_link", "bn_link", "x2_bn", "up_in", "up_link",
                 "gap", "want_gap", "grad_mode")

    def __init__(self, dtype, training, momentum, eps, track, need_act, need_pool, image_input, buffers):
        self.dtype, self.training, self.momentum, self.eps, self.track = dtype, training, momentum, eps, track
        self.need_act, self.need_pool, self.image_input, self.buffers = need_act, need_pool, image_input, buffers
        self.link_in = None   # PoolLink of the block whose pooled output is this block's input (set by the caller)
        self.link_out = None  # PoolLink this call offers to the next block (set by the forward)
        self.act_dst = None   # [N,H,W,cout_s] view (pixel stride >= cout_s) the activation is written to: one half of a
                              # decoder concatenation buffer (UNet.forward), so that torch.cat needs no copy
        self.lazy_act = False  # the activation's only consumer applies BN + ReLU itself: return the RAW output, offer link_act
        self.link_act = None
        self.x2_link = None    # ActLink of the producer of ``x2`` when that tensor is its RAW output (conv_block(..., x2=...))
        self.up_in = False     # conv_bn_relu: the input is nn.Upsample(x2) of the HALF-resolution tensor passed in (read in place)
        self.up_link = None    # UpLink shared by that conv_bn_relu call and the block that produced its input
        self.bn_link = None    # conv_bn_relu: its (raw output, BN coefficients) offered to the consumer of its activation ...
        self.x2_bn = None      # ... conv_block(..., x2=that activation): its dgrad leaves that BatchNorm's backward sums there
        self.gap = None       # set by the forward: [N, C] f32 global average of the activation it wrote (small maps), see conv_block
        self.want_gap = False  # the caller has a consumer for it (the block's output is tapped by a forward hook: semi_seg/arch/hook.py)
        self.grad_mode = True  # set by conv_block: was autograd recording at the call?  (``needs_input_grad`` alone says "yes" under
                               # torch.no_grad() too; side outputs that only a backward reads are not written then)
        self.up2 = False      # the activation's only consumer is nn.Upsample(scale_factor=2): write it 2x2-replicated, return
                              # the [N, C, 2H, 2W] tensor (spcl_bnrelu_up2_forward); backward sums the 2x2 gradients first


def _pack(w, kind, dt_code, dtype):
    co, ci = w.shape[0], w.shape[1]
    n = _n.call("spcl_conv_packed_elems", ci, co, kind, dt_code)
    buf = torch.empty(n, dtype=dtype, device=w.device)
    wc = w.detach().contiguous().float()
    _n.call("spcl_conv_pack_weights", _n.ptr(wc), ci, co, kind, dt_code, _n.ptr(buf), _n.stream())
    return buf


def _pack_both(w, dt_code, dtype):
    """forward and dgrad fragment layouts in one launch -> (packed_fwd, packed_dgrad)."""
    co, ci = w.shape[0], w.shape[1]
    n0 = _n.call("spcl_conv_packed_elems", ci, co, 0, dt_code)
    n1 = _n.call("spcl_conv_packed_elems", ci, co, 1, dt_code)
    buf = torch.empty(n0 + n1, dtype=dtype, device=w.device)
    wc = w.detach().contiguous().float()
    p0, p1 = buf[:n0], buf[n0:]
    _n.call("spcl_conv_pack_weights_both", _n.ptr(wc), ci, co, dt_code, _n.ptr(p0), _n.ptr(p1), _n.stream())
    return p0, p1


def _pack_block(wa, wb, dt_code, dtype, H=0, W=0):
    """both convolutions of a block, forward and dgrad layouts, one launch -> ((a_fwd, a_dgrad), (b_fwd, b_dgrad)).
    ``H, W``: the image size they are used at (the band-GEMM layout is only written where that kernel runs)."""
    sizes = []
    for w in (wa, wb):
        co, ci = w.shape[0], w.shape[1]
        sizes += [_n.call("spcl_conv_packed_elems", ci, co, 0, dt_code), _n.call("spcl_conv_packed_elems", ci, co, 1, dt_code)]
    buf = torch.empty(sum(sizes), dtype=dtype, device=wa.device)
    parts, off = [], 0
    for n_ in sizes:
        parts.append(buf[off:off + n_])
        off += n_
    wac, wbc = wa.detach().contiguous().float(), wb.detach().contiguous().float()
    _n.call("spcl_conv_pack_weights_block_at", _n.ptr(wac), wa.shape[1], wa.shape[0], _n.ptr(parts[0]), _n.ptr(parts[1]),
            _n.ptr(wbc), wb.shape[1], wb.shape[0], _n.ptr(parts[2]), _n.ptr(parts[3]), dt_code, int(H), int(W), _n.stream())
    return (parts[0], parts[1]), (parts[2], parts[3])


# ---- weights of several layers packed ahead of their use, in ONE launch (UNet.forward announces the layers it is about to
# run: one pack launch per forward pass instead of one per block).  Entries are consumed by the block that uses them.
_PREPACKED = {}
_PREPACK = os.environ.get("SPCL_PREPACK", "1") != "0"  # A/B switch: 0 = every block packs right before its convolutions


_PREPACKED_ACORR = {}


def take_prepacked_acorr(image):
    return _PREPACKED_ACORR.pop((image.data_ptr(), image._version), None)


_EVAL_AFFINE = {}


def clear_prepacked():
    """drop what a forward pass announced and did not consume (UNet.forward calls it on every exit)"""
    _PREPACKED.clear()
    _PREPACKED_ACORR.clear()
    _EVAL_AFFINE.clear()


def prepare_eval_affines(bns):
    """``bns``: the BatchNorm2d modules an EVAL-mode forward pass is about to apply: mean / invstd / scale / shift of all of
    them from their running statistics in ONE launch (spcl_bn_eval_affine_multi), handed to ``_bn_stats`` through
    ``_EVAL_AFFINE`` (keyed by the running mean's storage).  One launch per layer was 22 launches of ~5 us in a validation
    batch of the full UNet: a quarter of its GPU time."""
    _EVAL_AFFINE.clear()
    bns = [bn for bn in bns if bn.running_mean is not None and bn.running_mean.is_cuda and bn.weight is not None]
    for i in range(0, len(bns), _n.BN_EVAL_MAX):
        part = bns[i:i + _n.BN_EVAL_MAX]
        dev = part[0].running_mean.device
        sizes = [_ru16(bn.num_features) for bn in part]
        buf = torch.empty(4 * sum(sizes), dtype=torch.float32, device=dev)
        items, keep, off = [], [], 0
        for bn, cs in zip(part, sizes):
            g, b = bn.weight.detach().contiguous().float(), bn.bias.detach().contiguous().float()
            st = buf[off:off + 4 * cs].view(4, cs)
            off += 4 * cs
            items.append(_n.BnEvalItem(g.data_ptr(), b.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                                       st.data_ptr(), bn.num_features, cs, float(bn.eps)))
            keep.append((g, b))
            _EVAL_AFFINE[(bn.running_mean.data_ptr(), cs)] = st
        arr = (_n.BnEvalItem * len(items))(*items)
        _n.call("spcl_bn_eval_affine_multi", arr, len(items), _n.stream())


def prepack_weights(layers, dtype, image=None):
    """``layers``: list of (weight [Cout, Cin, 3, 3], H, W) about to be used at image size H x W with storage ``dtype``:
    forward and dgrad layouts of all of them in one launch (spcl_conv_pack_weights_multi), handed to the blocks through
    ``take_prepacked``.  Anything left over from an earlier, unfinished forward is dropped.
    ``image`` [N, H, W] (or [N, H, W, 1]) f32: the same launch also computes its autocorrelation rows (``_image_autocorr``,
    the image3 path of the first block), handed over through ``take_prepacked_acorr``."""
    _PREPACKED.clear()
    _PREPACKED_ACORR.clear()
    if not _PREPACK or not layers:
        return
    dtc = _n.dtype_code(dtype)
    dev = layers[0][0].device
    sizes = []
    for w, H, W in layers:
        co, ci = w.shape[0], w.shape[1]
        sizes.append((_n.call("spcl_conv_packed_elems", ci, co, 0, dtc), _n.call("spcl_conv_packed_elems", ci, co, 1, dtc)))
    for i in range(0, len(layers), _n.PACK_MULTI_MAX):
        part, psz = layers[i:i + _n.PACK_MULTI_MAX], sizes[i:i + _n.PACK_MULTI_MAX]
        buf = torch.empty(sum(a + b for a, b in psz), dtype=dtype, device=dev)
        items, keep, off = [], [], 0
        for (w, H, W), (n0, n1) in zip(part, psz):
            wc = w.detach().contiguous().float()
            p0, p1 = buf[off:off + n0], buf[off + n0:off + n0 + n1]
            off += n0 + n1
            items.append(_n.PackItem(wc.data_ptr(), p0.data_ptr(), p1.data_ptr(), w.shape[1], w.shape[0],
                                     int(H) if _PACK_AT else 0, int(W) if _PACK_AT else 0))
            keep.append(wc)
            _PREPACKED[(w.data_ptr(), w._version, dtc, int(H), int(W))] = (p0, p1)  # (_version: an in-place update since)
        arr = (_n.PackItem * len(items))(*items)
        if image is not None and i == 0 and _acorr_in_conv_rows(dtc, *[int(v) for v in image.shape[:3]]) > 0:
            image = None  # (the image convolution leaves the autocorrelation rows itself: _conv_image_acorr)
        # (the pass's BatchNorm accumulator arena is zeroed by this launch -- the first of the pass -- instead of a fill launch)
        zero = _acc_arena_take_dirty(dev) if i == 0 else None
        zbytes = ctypes.c_size_t(zero.numel() * 8 if zero is not None else 0)
        if image is not None and i == 0:
            N, H, W = int(image.shape[0]), int(image.shape[1]), int(image.shape[2])
            acorr = torch.empty(_n.call("spcl_image_autocorr_rows", N, H, W), 64, dtype=torch.float32, device=dev)
            _n.call("spcl_conv_pack_weights_multi_zero", arr, len(items), dtc, _n.ptr(image), N, H, W, _n.ptr(acorr),
                    _n.ptr(zero), zbytes, _n.stream())
            _PREPACKED_ACORR[(image.data_ptr(), image._version)] = acorr
        else:
            _n.call("spcl_conv_pack_weights_multi_zero", arr, len(items), dtc, None, 0, 0, 0, None, _n.ptr(zero), zbytes,
                    _n.stream())


def _acorr_in_conv_rows(dt_code, N, H, W, cin=1, cout_s=16):
    """rows ([rows][64] f32) the image block's first convolution leaves as the image's autocorrelation partials when it
    runs as spcl_conv3x3_forward_image_acorr; 0: that form does not take the shape (the rows come from their own pass)"""
    return _n.call("spcl_conv3x3_forward_image_acorr_rows", dt_code, N, H, W, cin, cout_s)


def _conv_image_acorr(x_store, dt_code, dtype, N, H, W, cin_s, cout_s, wp, want_stats, rows, store=True):
    """the one-channel image convolution + the image's autocorrelation rows in ONE launch
    (spcl_conv3x3_forward_image_acorr) -> (y, stats, acorr [rows][64]); ``store=False``: the statistics-only form, y is None
    (the same rows bit for bit; the block's other launches form y again per tile: ``_BLOCK1_RECOMPUTE``)"""
    dev = x_store.device
    y = torch.empty(N, H, W, cout_s, dtype=dtype, device=dev) if store else None
    stats = None
    if want_stats:
        nt = _n.call("spcl_conv_stat_rows", dt_code, N, H, W, 16, cout_s)
        stats = torch.empty(_n.call("spcl_bn_stats_elems", nt, cout_s), dtype=torch.float32, device=dev)
        stats.ntiles = nt
    acorr = torch.empty(rows, 64, dtype=torch.float32, device=dev)
    _n.call("spcl_conv3x3_forward_image_acorr", _n.ptr(x_store), dt_code, N, H, W, cin_s, cout_s, _n.ptr(wp), _n.ptr(y),
            _n.ptr(stats), _n.ptr(acorr), _n.stream())
    return y, stats, acorr


# A/B switch: 0 = the image block stores its first convolution's raw output (103 MB at 64 x 224^2: written once, read by the
# second convolution's forward and by its backward) instead of forming it again per tile from the image in those two launches
_BLOCK1_RECOMPUTE = os.environ.get("SPCL_BLOCK1_RECOMPUTE", "1") != "0"
# A/B switch: 0 = the image block's backward materialises the gradient behind Conv1.b's BatchNorm + ReLU + max-pool (103 MB at
# 64 x 224^2: written by the BatchNorm apply pass, read back once by the one-pass backward of Conv1.b, its only reader) instead
# of that kernel forming it per tile from Conv1.b's raw output and the pooled gradient (spcl_conv16_bwd_fused_image_pooled)
_BLOCK1_POOLED_BWD = os.environ.get("SPCL_BLOCK1_POOLED_BWD", "1") != "0"


def _conv_from_image(image, y_image, dt_code, dtype, N, H, W, cout_s, wp_image, scale, shift, wp, want_stats):
    """the image block's second convolution with its input relu(scale y1a + shift) formed per tile from the f32 image and the
    first convolution's packed weights (spcl_conv3x3_forward_from_image; ``y_image``: the stored y1a is read instead, on the
    same 14 x 14 tiles) -> (y, stats), one statistics row set per 14 x 14 tile"""
    dev = image.device
    y = torch.empty(N, H, W, cout_s, dtype=dtype, device=dev)
    stats = None
    if want_stats:
        nt = N * (H // 14) * (W // 14)
        stats = torch.empty(_n.call("spcl_bn_stats_elems", nt, cout_s), dtype=torch.float32, device=dev)
        stats.ntiles = nt
    _n.call("spcl_conv3x3_forward_from_image", _n.ptr(image), _n.ptr(y_image), dt_code, N, H, W, cout_s, _n.ptr(wp_image),
            _n.ptr(scale), _n.ptr(shift), _n.ptr(wp), _n.ptr(y), _n.ptr(stats), _n.stream())
    return y, stats


def take_prepacked(w, dtc, H, W):
    return _PREPACKED.pop((w.data_ptr(), w._version, dtc, int(H), int(W)), None)


def _conv(x_store, dt_code, dtype, N, H, W, cin_s, cin_k, cout_s, wp, in_mode, scale, shift, want_stats):
    dev = x_store.device
    y = torch.empty(N, H, W, cout_s, dtype=dtype, device=dev)
    stats = None
    if want_stats:
        # rows [tile][3][cout_s] of Chan partials (+ the finalize kernel's scratch rows), see include/spcl_hip.h
        nt = _n.call("spcl_conv_stat_rows", dt_code, N, H, W, cin_k, cout_s)
        stats = torch.empty(_n.call("spcl_bn_stats_elems", nt, cout_s), dtype=torch.float32, device=dev)
        stats.ntiles = nt
    _n.call("spcl_conv3x3_forward", _n.ptr(x_store), dt_code, N, H, W, cin_s, cin_k, cout_s, _n.ptr(wp), in_mode,
            _n.ptr(scale), _n.ptr(shift), _n.ptr(y), _n.ptr(stats), _n.stream())
    return y, stats


def _conv_cat(xa, xb, dt_code, dtype, N, H, W, chalf, cout_s, wp, want_stats, xb_scale=None, xb_shift=None):
    """the convolution of ``torch.cat((xa, xb), channel)`` read from the two tensors (spcl_conv3x3_forward_cat);
    ``xb_scale`` / ``xb_shift``: ``xb`` is a raw convolution output, the concatenation holds relu(scale xb + shift)"""
    dev = xa.device
    y = torch.empty(N, H, W, cout_s, dtype=dtype, device=dev)
    stats = None
    if want_stats:
        nt = _n.call("spcl_conv_stat_rows", dt_code, N, H, W, 2 * chalf, cout_s)
        stats = torch.empty(_n.call("spcl_bn_stats_elems", nt, cout_s), dtype=torch.float32, device=dev)
        stats.ntiles = nt
    _n.call("spcl_conv3x3_forward_cat", _n.ptr(xa), _n.ptr(xb), dt_code, N, H, W, chalf, cout_s, _n.ptr(wp),
            _n.ptr(xb_scale), _n.ptr(xb_shift), _n.ptr(y), _n.ptr(stats), _n.stream())
    return y, stats


# ---- BatchNorm sums as fixed-point accumulator blocks (csrc/bn_acc.hpp): the producing kernel's epilogue ADDS its tile's sums
# (exact integer atomics: order-free, bit-for-bit deterministic), the next launch derives the coefficients in its prologue -- no
# finalize launch between them.  A block must be ZERO before its producer runs: all blocks of a forward pass (and of the
# backward that follows it) are slices of ONE zero-filled arena, i.e. one fill launch per step.
_BN_ACC = os.environ.get("SPCL_BN_ACC", "1") != "0"  # A/B switch: 0 keeps the per-tile rows + finalize launches everywhere
_ACC_ARENA = {"buf": None, "off": 0, "used": 0, "need": 0, "dirty": False}


def bn_acc_arena_begin(device):
    """a new forward pass starts (UNet.forward): an arena of what the previous pass used, zeroed by the pass's weight-pack
    launch (``prepack_weights``) or, failing that, by a fill of its own at the first block taken; blocks beyond it (the first
    pass, a changed shape) come from on-demand zero-filled chunks"""
    a = _ACC_ARENA
    a["need"], a["used"], a["off"] = a["used"], 0, 0
    a["buf"] = torch.empty(a["need"], dtype=torch.int64, device=device) if (a["need"] > 0 and _BN_ACC) else None
    a["dirty"] = a["buf"] is not None


def _acc_arena_take_dirty(device):
    """the arena still to be zeroed, for a launch that can do it on its way (-> tensor or None); the caller MUST zero it"""
    a = _ACC_ARENA
    if a["dirty"] and a["buf"] is not None and a["buf"].device == device:
        a["dirty"] = False
        return a["buf"]
    return None


def bn_acc_block(cs, device):
    """a zeroed accumulator block for a BatchNorm of ``cs`` (padded) channels -> int64 tensor [spcl_bn_acc_elems(cs)]"""
    words = _n.call("spcl_bn_acc_elems", int(cs))
    a = _ACC_ARENA
    buf = a["buf"]
    if buf is not None and a["dirty"]:  # nobody zeroed it on the way (no weight-pack launch in this pass)
        buf.zero_()
        a["dirty"] = False
    if buf is None or buf.device != device or a["off"] + words > buf.numel():
        buf = a["buf"] = torch.zeros(max(words, 1 << 15), dtype=torch.int64, device=device)
        a["off"] = 0
    blk = buf[a["off"]:a["off"] + words]
    a["off"] += words
    a["used"] += words
    return blk


def _bn_acc_desc(acc, cfg: "BlockCfg", C, cs, gamma, beta, which, count, st, keep):
    """the ``spcl_bn_acc`` of one BatchNorm (native.BnAcc); ``keep`` collects the tensors its pointers borrow"""
    g, b = gamma.detach().contiguous().float(), beta.detach().contiguous().float()
    rm, rv, nbt = cfg.buffers[which]
    upd = cfg.track[which]
    keep.extend([g, b])
    return _n.BnAcc(acc.data_ptr(), g.data_ptr(), b.data_ptr(), rm.data_ptr() if upd else None,
                    rv.data_ptr() if upd else None, nbt.data_ptr() if (upd and nbt is not None) else None, st.data_ptr(),
                    float(cfg.momentum), float(cfg.eps), float(count), int(C), int(cs))


def _conv_acc(x_store, dt_code, dtype, N, H, W, cin_k, cout_s, wp, in_bn, in_scale, in_shift, stats_acc, want_rows):
    """spcl_conv3x3_forward_acc: the input's BatchNorm + ReLU from a block (``in_bn``: native.BnAcc) or from scale / shift
    arrays or none; the output's statistics into ``stats_acc`` or, ``want_rows``, per-tile rows -> (y, rows or None)"""
    dev = x_store.device
    y = torch.empty(N, H, W, cout_s, dtype=dtype, device=dev)
    rows = None
    if want_rows and stats_acc is None:
        nt = _n.call("spcl_conv_stat_rows", dt_code, N, H, W, cin_k, cout_s)
        rows = torch.empty(_n.call("spcl_bn_stats_elems", nt, cout_s), dtype=torch.float32, device=dev)
        rows.ntiles = nt
    _n.call("spcl_conv3x3_forward_acc", _n.ptr(x_store), dt_code, N, H, W, cin_k, cout_s, _n.ptr(wp),
            ctypes.byref(in_bn) if in_bn is not None else None, _n.ptr(in_scale), _n.ptr(in_shift), _n.ptr(y),
            _n.ptr(stats_acc), _n.ptr(rows), _n.stream())
    return y, rows


def _bn_stats(stats, cfg: BlockCfg, C, cs, gamma, beta, which, dev):
    """-> tensor [4, cs]: mean, invstd, scale, shift."""
    st = torch.empty(4, cs, dtype=torch.float32, device=dev)
    g, b = gamma.detach().contiguous().float(), beta.detach().contiguous().float()
    rm, rv, nbt = cfg.buffers[which]
    if cfg.training:
        upd = cfg.track[which]
        _n.call("spcl_bn_finalize", _n.ptr(stats), stats.ntiles, C, cs, _n.ptr(g), _n.ptr(b), c_float(cfg.momentum),
                c_float(cfg.eps), _n.ptr(rm if upd else None), _n.ptr(rv if upd else None),
                _n.ptr(nbt if upd else None), _n.ptr(st[0]), _n.ptr(st[1]), _n.ptr(st[2]), _n.ptr(st[3]), _n.stream())
    else:
        pre = _EVAL_AFFINE.pop((rm.data_ptr(), cs), None) if rm.dtype == torch.float32 else None
        if pre is not None:  # computed with the pass's other layers in one launch (prepare_eval_affines)
            return pre
        _n.call("spcl_bn_eval_affine", C, cs, _n.ptr(g), _n.ptr(b), _n.ptr(rm), _n.ptr(rv), c_float(cfg.eps),
                _n.ptr(st[0]), _n.ptr(st[1]), _n.ptr(st[2]), _n.ptr(st[3]), _n.stream())
    return st


class DeferredWgrads:
    """Weight gradients of the wide (channel counts multiples of 64) bf16 layers, queued during backward and computed by
    ONE batched launch (csrc/wgrad_gemm.hip: the split-K partials are then written once per CU for all layers together
    instead of once per CU and layer).

    Only gradients that go STRAIGHT INTO A FLAT GRADIENT BUCKET are deferred (the parameter's armed sink, see
    ``take_grad_sink``), and autograd never sees them: the backward returns ``None`` for that parameter and the batched
    launch writes the bucket slice when the queue is flushed.  ``ddp.GradBucket.arm_sinks`` opens the queue, ``gather``
    flushes it before anything reads the bucket, adds what autograd accumulated from OTHER uses of the same parameter in
    that step (they do not get the sink) and points ``param.grad`` at the slice."""

    def __init__(self):
        self.items, self.keep, self.targets = [], [], set()
        self.tails = []

    def add(self, x_store, dy, scale, shift, sink, N, H, W, cin, cin_s, cout, cout_s, in_mode, x2=None, x_up2=False):
        it = _n.WgradItem(x_store.data_ptr(), dy.data_ptr(), scale.data_ptr() if scale is not None else None,
                          shift.data_ptr() if shift is not None else None, sink.data_ptr(), N, H, W, cin, cin_s, cout,
                          cout_s, in_mode, x2.data_ptr() if x2 is not None else None, 1 if x_up2 else 0)
        self.items.append(it)
        self.keep.append((x_store, dy, scale, shift, x2))  # operands stay alive until the launch
        self.targets.add(sink.data_ptr())
        if len(self.items) == _QUEUE_MAX[0]:
            self.flush()

    def capture_tail(self, sink, keep, launch):
        """Run ``launch()`` -- one of the narrow layers' weight-gradient producers writing to ``sink`` -- with a tail
        capture armed (``spcl_wgrad_tail_capture``): its few-microsecond final reduction launch is skipped and rides in
        the batched launch's reduction kernel at the next flush.  ``keep``: the buffers the pending sum reads.  Returns
        True when the producer left a tail (the gradient then reaches ``sink`` at the flush, like a deferred item)."""
        tail = _n.WgradTail()
        _n.call("spcl_wgrad_tail_capture", ctypes.byref(tail))
        try:
            launch()
        finally:
            _n.call("spcl_wgrad_tail_capture", None)
        if tail.kind < 0:
            return False
        self.tails.append(tail)
        self.keep.append(keep)
        self.targets.add(sink.data_ptr())
        if len(self.tails) == _QUEUE_MAX[1]:
            self.flush()
        return True

    def flush(self):
        if not self.items and not self.tails:
            return
        wgrad_batched(self.items, accumulate=False, device=self.keep[0][1].device, tails=self.tails)
        self.items, self.keep, self.tails = [], [], []


# items / tails a queue holds before it flushes by itself (A/B switch SPCL_WGRAD_QUEUE_MAX; the library's limits by default:
# the whole UNet's eleven wide layers and ten narrow ones then leave in ONE batched launch at the gather)
_QUEUE_MAX = (min(_n.WGRAD_BATCH_MAX, int(os.environ.get("SPCL_WGRAD_QUEUE_MAX", _n.WGRAD_BATCH_MAX))),
              min(_n.WGRAD_TAILS_MAX, int(os.environ.get("SPCL_WGRAD_QUEUE_MAX", _n.WGRAD_TAILS_MAX))))
_CONV_UP2 = os.environ.get("SPCL_CONV_UP2", "1") != "0"  # A/B switch: 0 writes the x2-upsampled activations (BlockCfg.up2)
_UP2_BWD_FUSED = os.environ.get("SPCL_UP2_BWD_FUSED", "1") != "0"  # A/B switch: 0 sums the 2x2 gradients in a launch of its own
_CONV_SPLIT = os.environ.get("SPCL_CONV_SPLIT", "1") != "0"  # A/B switch: 0 leaves that level's gradient as one interleaved tensor
_CONV_CAT = os.environ.get("SPCL_CONV_CAT", "1") != "0"  # A/B switch: 0 materialises the 16-channel decoder concatenation
_PACK_AT = os.environ.get("SPCL_PACK_AT", "1") != "0"  # A/B switch: 0 packs the band-GEMM layout whether or not it is used
_ACC_FILL = os.environ.get("SPCL_ACC_FILL", "1") != "0"  # A/B switch: 0 keeps the finalize launch of the generic BatchNorm backward
_GAP = os.environ.get("SPCL_GAP", "1") != "0"  # A/B switch: 0 leaves the global average to the projector's own pooling launch
_TAILS = os.environ.get("SPCL_WGRAD_TAILS", "1") != "0"  # A/B switch: 0 keeps every layer's own final reduction launch


def sink_queue(sink):
    """the deferred weight-gradient queue of the bucket that armed ``sink`` (``ddp.GradBucket.arm_sinks`` hangs it on the
    bucket's views), or None: every bucket owns its queue, so two buckets armed in one step never see each other's items
    and a step that was aborted between arming and gathering leaves nothing behind for the next one"""
    return getattr(sink, "_spcl_queue", None) if sink is not None else None


def wgrad_batched(items, accumulate, device, tails=()):
    """one launch for ``items`` (list of native.WgradItem, at most native.WGRAD_BATCH_MAX) and the captured ``tails``
    (native.WgradTail, at most native.WGRAD_TAILS_MAX)"""
    arr, ws = None, None
    if items:
        arr = (_n.WgradItem * len(items))(*items)
        nbytes = _n.call("spcl_conv_wgrad_batched_workspace_bytes", arr, len(items))
        if nbytes == 0:
            raise RuntimeError("wgrad_batched: unsupported item (bf16 NHWC, channel counts multiples of 64, in_mode 0/1)")
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    tarr = (_n.WgradTail * len(tails))(*tails) if tails else None
    _n.call("spcl_conv3x3_wgrad_batched_tails", arr, len(items), tarr, len(tails), int(bool(accumulate)), _n.ptr(ws),
            _n.stream())


def _wgrad(x_store, dy, dt_code, N, H, W, cin, cin_s, cin_k, cout, cout_s, in_mode, scale, shift, sink=None):
    dev = dy.device
    queue = sink_queue(sink)
    if (queue is not None and cin_s == cin_k
            and _n.call("spcl_conv_wgrad_batched_supported", dt_code, cin, cin_s, cout, cout_s, in_mode)):
        queue.add(x_store, dy, scale, shift, sink, N, H, W, cin, cin_s, cout, cout_s, in_mode)
        return None  # written into the bucket slice when the queue is flushed; autograd gets no gradient from this use
    nbytes = _n.call("spcl_conv_wgrad_workspace_bytes", N, H, W, cin_k, cout_s)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    dw = _grad_buffer(sink, (cout, cin, 3, 3), dev)

    def launch():
        _n.call("spcl_conv3x3_wgrad", _n.ptr(x_store), _n.ptr(dy), dt_code, N, H, W, cin, cin_s, cin_k, cout, cout_s,
                in_mode, _n.ptr(scale), _n.ptr(shift), _n.ptr(ws), _n.ptr(dw), _n.stream())

    if queue is not None and _TAILS:
        # narrow layer straight into a bucket slice: its final sum joins the batched launch (no separate reduce launch)
        if queue.capture_tail(sink, (ws, dy, x_store, scale, shift), launch):
            return None
        return dw
    launch()
    return dw


def _wgrad_up2(x_half, dy, dt_code, N, H, W, cin, cout, cout_s, sink=None):
    """weight gradient of the up-convolution, its input ``nn.Upsample(x2)(x_half)`` read from the half-resolution tensor
    (spcl_conv3x3_wgrad_up2 / spcl_wgrad_item::x_up2); H x W = the convolution's size"""
    dev = dy.device
    queue = sink_queue(sink)
    if queue is not None and _n.call("spcl_conv_wgrad_batched_supported", dt_code, cin, cin, cout, cout_s, 0):
        queue.add(x_half, dy, None, None, sink, N, H, W, cin, cin, cout, cout_s, 0, x_up2=True)
        return None
    nbytes = _n.call("spcl_conv_wgrad_workspace_bytes", N, H, W, cin, cout_s)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    dw = _grad_buffer(sink, (cout, cin, 3, 3), dev)

    def launch():
        _n.call("spcl_conv3x3_wgrad_up2", _n.ptr(x_half), _n.ptr(dy), dt_code, N, H, W, cin, cout, cout_s, _n.ptr(ws),
                _n.ptr(dw), _n.stream())

    if queue is not None and _TAILS:
        if queue.capture_tail(sink, (ws, dy, x_half), launch):
            return None
        return dw
    launch()
    return dw


def up_in_shape_ok(N, cin, H, W, cout, dtype):
    """can ``conv_bn_relu`` read ``nn.Upsample(x2)`` of a dense [N, cin, H/2, W/2] tensor in its loaders (H x W the
    convolution's size)?  (spcl_conv_up2_supported: bf16, sizes the specialised kernels tile)"""
    return bool(_CONV_UP2 and dtype == torch.bfloat16 and cin % 16 == 0
                and _n.call("spcl_conv_up2_supported", _n.dtype_code(dtype), N, H, W, cin, _ru16(cout)))


def _wgrad_cat(xa, xb, dy, dt_code, N, H, W, chalf, cout, cout_s, sink=None, xb_scale=None, xb_shift=None):
    """weight gradient of the convolution of ``cat((xa, xb), channel)``, the input read from the two tensors
    (spcl_conv3x3_wgrad_cat); the final sum rides in the batched launch when ``sink`` belongs to a bucket, as in ``_wgrad``"""
    dev = dy.device
    queue = sink_queue(sink)
    if (queue is not None and xb_scale is None
            and _n.call("spcl_conv_wgrad_batched_supported", dt_code, 2 * chalf, 2 * chalf, cout, cout_s, 0)):
        # a wide layer: one item of the batched launch, its 64-channel input blocks read from the tensor that holds them
        queue.add(xa, dy, None, None, sink, N, H, W, 2 * chalf, 2 * chalf, cout, cout_s, 0, x2=xb)
        return None
    nbytes = _n.call("spcl_conv_wgrad_workspace_bytes", N, H, W, 2 * chalf, cout_s)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    dw = _grad_buffer(sink, (cout, 2 * chalf, 3, 3), dev)

    def launch():
        _n.call("spcl_conv3x3_wgrad_cat", _n.ptr(xa), _n.ptr(xb), _n.ptr(dy), dt_code, N, H, W, chalf, cout, cout_s,
                _n.ptr(xb_scale), _n.ptr(xb_shift), _n.ptr(ws), _n.ptr(dw), _n.stream())

    if queue is not None and _TAILS:
        if queue.capture_tail(sink, (ws, dy, xa, xb, xb_scale, xb_shift), launch):
            return None
        return dw
    launch()
    return dw


_BCAST = os.environ.get("SPCL_POOL_BCAST", "1") != "0"  # A/B switch: 0 materialises the average pool's gradient


def broadcast_rows(g, dtype):
    """``g`` [N, C, H, W] whose every pixel of an (image, channel) holds the same value through stride-0 dimensions (what
    the projector's backward hands over for a global average pool: ``[N, C] .view(N, C, 1, 1).expand(N, C, H, W)``) ->
    the contiguous [N, C] tensor behind it, else None"""
    if (g is None or g.dim() != 4 or g.dtype != dtype or g.shape[1] % 16 or g.shape[2] * g.shape[3] <= 1
            or g.stride(2) != 0 or g.stride(3) != 0 or g.stride(1) != 1 or g.stride(0) != g.shape[1]):
        return None
    return torch.as_strided(g, (g.shape[0], g.shape[1]), (g.shape[1], 1), g.storage_offset())


def _bnrelu_bwd_bcast(y, g_nc, dt_code, dtype, N, H, W, C, cs, st, training, sinks=(None, None)):
    """_bnrelu_bwd for a gradient that is one value per (image, channel) (spcl_bnrelu_backward_bcast)"""
    dev = y.device
    ws = torch.empty(_n.call("spcl_bnrelu_bwd_workspace_bytes", N, H, W, cs) // 4, dtype=torch.float32, device=dev)
    dgamma = _grad_buffer(sinks[0], (C,), dev)
    dbeta = _grad_buffer(sinks[1], (C,), dev)
    dy = torch.empty(N, H, W, cs, dtype=dtype, device=dev)
    _n.call("spcl_bnrelu_backward_bcast", _n.ptr(y), _n.ptr(g_nc), dt_code, N, H, W, C, cs, _n.ptr(st[0]), _n.ptr(st[1]),
            _n.ptr(st[2]), _n.ptr(st[3]), int(training), _n.ptr(ws), _n.ptr(dgamma), _n.ptr(dbeta), _n.ptr(dy), _n.stream())
    return dy, dgamma, dbeta


def _bnrelu_bwd(y, dact, dpool, dt_code, dtype, N, H, W, C, cs, st, training, sinks=(None, None), dact_stride=0, d_up=None):
    """``dact_stride`` > 0: ``dact`` is a channel slice of a wider NHWC tensor with that many elements per pixel.
    ``d_up``: the gradient arrives at twice the resolution ([N, 2H, 2W, cs]: the activation went through nn.Upsample(x2));
    its 2 x 2 sums are formed inside the reduction pass (spcl_bnrelu_backward_up2), ``dact`` is not given"""
    dev = y.device
    ws = torch.empty(_n.call("spcl_bnrelu_bwd_workspace_bytes", N, H, W, cs) // 4, dtype=torch.float32, device=dev)
    dgamma = _grad_buffer(sinks[0], (C,), dev)
    dbeta = _grad_buffer(sinks[1], (C,), dev)
    dy = torch.empty(N, H, W, cs, dtype=dtype, device=dev)
    if d_up is not None:
        assert dact is None and dpool is None
        gsum = torch.empty(N, H, W, cs, dtype=dtype, device=dev)  # (the summed gradient, for the apply pass)
        _n.call("spcl_bnrelu_backward_up2", _n.ptr(y), _n.ptr(d_up), _n.ptr(gsum), dt_code, N, H, W, C, cs, _n.ptr(st[0]),
                _n.ptr(st[1]), _n.ptr(st[2]), _n.ptr(st[3]), int(training), _n.ptr(ws), _n.ptr(dgamma), _n.ptr(dbeta),
                _n.ptr(dy), _n.stream())
    elif dact_stride and dact is not None:
        _n.call("spcl_bnrelu_pool_backward_strided", _n.ptr(y), _n.ptr(dact), int(dact_stride), _n.ptr(dpool), dt_code, N, H,
                W, C, cs, _n.ptr(st[0]), _n.ptr(st[1]), _n.ptr(st[2]), _n.ptr(st[3]), int(training), _n.ptr(ws),
                _n.ptr(dgamma), _n.ptr(dbeta), _n.ptr(dy), _n.stream())
    else:
        _n.call("spcl_bnrelu_pool_backward", _n.ptr(y), _n.ptr(dact), _n.ptr(dpool), dt_code, N, H, W, C, cs,
                _n.ptr(st[0]), _n.ptr(st[1]), _n.ptr(st[2]), _n.ptr(st[3]), int(training), _n.ptr(ws), _n.ptr(dgamma),
                _n.ptr(dbeta), _n.ptr(dy), _n.stream())
    return dy, dgamma, dbeta


def _bnrelu_bwd_image_wgrad(y, dact, image, dt_code, N, H, W, C, cs, st, training, sinks=(None, None, None)):
    """BN+ReLU backward of a one-channel image block's first conv fused with its weight gradient (no dy tensor)."""
    dev = y.device
    nbytes = _n.call("spcl_bnrelu_image_wgrad_workspace_bytes", N, H, W, cs)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    dw = _grad_buffer(sinks[0], (C, 1, 3, 3), dev)
    dgamma = _grad_buffer(sinks[1], (C,), dev)
    dbeta = _grad_buffer(sinks[2], (C,), dev)

    def launch():
        _n.call("spcl_bnrelu_backward_image_wgrad", _n.ptr(y), _n.ptr(dact), _n.ptr(image), dt_code, N, H, W, C, cs,
                _n.ptr(st[0]), _n.ptr(st[1]), _n.ptr(st[2]), _n.ptr(st[3]), int(training), _n.ptr(ws), _n.ptr(dgamma),
                _n.ptr(dbeta), _n.ptr(dw), _n.stream())

    queue = sink_queue(sinks[0])
    if queue is not None and _TAILS:
        if queue.capture_tail(sinks[0], (ws, dact), launch):
            dw = None  # reaches the bucket slice when the queue is flushed
    else:
        launch()
    return dw, dgamma, dbeta


def _image_wgrad_fusable(cfg, cin, cout_s):
    return cfg.image_input and cin == 1 and cout_s <= 256 and cout_s & (cout_s - 1) == 0


def _dgrad_bnstats(dy, wp_t, y2, st2, dt_code, dtype, N, H, W, cin_k, cout_s):
    """input gradient of a block's second conv + the per-tile partial sums of the first conv's BN backward (one kernel)
    -> (g, rows) or None where no specialised kernel exists (the caller then runs the separate reduction pass)."""
    if not _n.call("spcl_conv_dgrad_bnstats_supported", dt_code, N, H, W, cin_k, cout_s):
        return None
    dev = dy.device
    nt = _n.call("spcl_conv_stat_rows", dt_code, N, H, W, cin_k, cout_s)
    g = torch.empty(N, H, W, cout_s, dtype=dtype, device=dev)
    rows = torch.empty(nt * 2 * cout_s, dtype=torch.float32, device=dev)
    _n.call("spcl_conv3x3_dgrad_bnstats", _n.ptr(dy), dt_code, N, H, W, cin_k, cout_s, _n.ptr(wp_t), _n.ptr(g),
            _n.ptr(y2), _n.ptr(st2[2]), _n.ptr(st2[3]), _n.ptr(st2[0]), _n.ptr(rows), _n.stream())
    rows.ntiles = nt
    return g, rows


def _bnrelu_bwd_rows(y, dact, image, rows, dt_code, dtype, N, H, W, C, cs, st, training, sinks):
    """BN+ReLU backward finished from the dgrad's per-tile rows -> (dy or dW, dgamma, dbeta)."""
    dev = y.device
    nbytes = _n.call("spcl_bnrelu_image_wgrad_workspace_bytes" if image is not None else
                     "spcl_bnrelu_bwd_workspace_bytes", N, H, W, cs)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    if image is not None:
        first = _grad_buffer(sinks[0], (C, 1, 3, 3), dev)
        dgamma, dbeta = _grad_buffer(sinks[1], (C,), dev), _grad_buffer(sinks[2], (C,), dev)
        dy, dw = None, first
    else:
        first = torch.empty(N, H, W, cs, dtype=dtype, device=dev)
        dgamma, dbeta = _grad_buffer(sinks[0], (C,), dev), _grad_buffer(sinks[1], (C,), dev)
        dy, dw = first, None
    def launch():
        _n.call("spcl_bnrelu_backward_rows", _n.ptr(y), _n.ptr(dact), _n.ptr(image), _n.ptr(rows), rows.ntiles, dt_code,
                N, H, W, C, cs, _n.ptr(st[0]), _n.ptr(st[1]), _n.ptr(st[2]), _n.ptr(st[3]), int(training), _n.ptr(ws),
                _n.ptr(dgamma), _n.ptr(dbeta), _n.ptr(dy), _n.ptr(dw), _n.stream())

    queue = sink_queue(sinks[0]) if image is not None else None
    if queue is not None and _TAILS:
        if queue.capture_tail(sinks[0], (ws, dact), launch):
            first = None  # the weight gradient reaches the bucket slice when the queue is flushed
    else:
        launch()
    return first, dgamma, dbeta


_IMAGE3 = os.environ.get("SPCL_IMAGE3", "1") != "0"  # A/B switch: 0 keeps the fused BN-backward + weight-gradient pass


def _image3_supported(cfg, cin, dt_code, N, H, W, cout_s):
    """the first conv of a one-channel-image block can get its BN backward and weight gradient WITHOUT a pass over its
    output (csrc/bn.hip image3: dgrad epilogue sums + image autocorrelation)"""
    return bool(_IMAGE3 and cfg.image_input and cin == 1 and cfg.dtype == torch.bfloat16 and W <= 256 and
                _n.call("spcl_conv_dgrad_bnstats_image_supported", dt_code, N, H, W, cout_s, cout_s))


def _image_autocorr(image, N, H, W):
    """partial rows of the 9 x 9 autocorrelation (45 sums) and the 9 shifted sums of the zero-padded f32 image batch"""
    rows = _n.call("spcl_image_autocorr_rows", N, H, W)
    out = torch.empty(rows, 64, dtype=torch.float32, device=image.device)
    _n.call("spcl_image_autocorr", _n.ptr(image), N, H, W, _n.ptr(out), _n.stream())
    return out


def _dgrad_bnstats_image(dy, wp_t, y2, st2, image, dt_code, dtype, N, H, W, cs, want_g=False):
    """_dgrad_bnstats for the image block: the per-tile rows carry nine more sub-rows, sum dz * image[p + tap].  The
    gradient g itself is only written on request: with image3 nothing downstream reads it (103 MB at 64 x 224^2)."""
    dev = dy.device
    nt = _n.call("spcl_conv_stat_rows", dt_code, N, H, W, cs, cs)
    g = torch.empty(N, H, W, cs, dtype=dtype, device=dev) if want_g else None
    rows = torch.empty(nt * 11 * cs, dtype=torch.float32, device=dev)
    _n.call("spcl_conv3x3_dgrad_bnstats_image", _n.ptr(dy), dt_code, N, H, W, cs, cs, _n.ptr(wp_t), _n.ptr(g), _n.ptr(y2),
            _n.ptr(st2[2]), _n.ptr(st2[3]), _n.ptr(st2[0]), _n.ptr(image), _n.ptr(rows), _n.stream())
    rows.ntiles = nt
    return g, rows


_CONV16_FUSED = os.environ.get("SPCL_CONV16_FUSED", "1") != "0"  # A/B switch: 0 = separate wgrad and dgrad launches
_CONV16_WGROWS = os.environ.get("SPCL_CONV16_WGROWS", "1") != "0"  # A/B switch: 0 = per-tile rows + the folding launch


def _conv16_bwd_fused(dy, wp_t, y2, st2, image, dt_code, N, H, W, cin, cout, cs, sink, acorr=None, wp_image=None, pooled=None):
    """the image block's second conv, whole backward in one launch (csrc/conv16_bwd.hip): -> (dW or None when it went into
    a bucket slice, rows of the first conv's BatchNorm backward / weight gradient).  With ``acorr`` (the autocorrelation's
    partial rows) the rows come as ONE set per workgroup in the final kernel's layout (``rows.wg``) and the same launch
    folds ``acorr`` to 16 rows (``rows.acorr16``): no per-tile rows, no folding launch; else per tile ([tiles][11][cs]).
    ``y2`` None: the first conv's output was never stored -- the kernel forms it from ``image`` and ``wp_image``, that conv's
    packed forward weights (spcl_conv16_bwd_fused_image).  ``pooled`` (with ``dy`` and ``y2`` None): ``dy`` was never stored
    either -- (y, dpool, rows, st, acc, dgamma, dbeta, training) of this convolution's BatchNorm + ReLU + max-pool, from which
    the kernel's loader forms it (spcl_conv16_bwd_fused_image_pooled, which also adds ``rows`` to the zeroed block ``acc`` and
    leaves dgamma / dbeta)."""
    dev = image.device
    if y2 is None and wp_image is None:
        raise RuntimeError("conv16 backward: neither the first convolution's output nor its packed weights")
    if (dy is None) != (pooled is not None) or (pooled is not None and y2 is not None):
        raise RuntimeError("conv16 backward: exactly one of the gradient and the tensors it is formed from")
    nsplit = _n.call("spcl_conv16_bwd_fused_splits", N, H, W)
    if acorr is not None:
        rows = torch.empty(11 * cs * nsplit, dtype=torch.float32, device=dev)
        rows.wg, rows.acorr16 = nsplit, torch.empty(16, 64, dtype=torch.float32, device=dev)
    else:
        nt = _n.call("spcl_conv_stat_rows", dt_code, N, H, W, cs, cs)
        rows = torch.empty(nt * 11 * cs, dtype=torch.float32, device=dev)
        rows.ntiles, rows.wg = nt, 0
    ws = torch.empty(nsplit * 9 * 256, dtype=torch.float32, device=dev)
    dw = _grad_buffer(sink, (cout, cin, 3, 3), dev)

    def launch():
        if pooled is not None:
            yb, dpool, prow, stb, acc, dgamma, dbeta, training = pooled
            _n.call("spcl_conv16_bwd_fused_image_pooled", _n.ptr(yb), _n.ptr(dpool), _n.ptr(prow), prow.ntiles, dt_code, N, H, W,
                    _n.ptr(stb), int(training), _n.ptr(acc), _n.ptr(dgamma), _n.ptr(dbeta), _n.ptr(wp_t), _n.ptr(wp_image),
                    _n.ptr(st2[2]), _n.ptr(st2[3]), _n.ptr(st2[0]), _n.ptr(image), _n.ptr(rows) if not rows.wg else None,
                    _n.ptr(ws), _n.ptr(dw), cin, cout, _n.ptr(rows) if rows.wg else None, _n.ptr(acorr),
                    0 if acorr is None else acorr.shape[0], _n.ptr(rows.acorr16) if rows.wg else None, _n.stream())
            return
        _n.call("spcl_conv16_bwd_fused" if y2 is not None else "spcl_conv16_bwd_fused_image", _n.ptr(dy), dt_code, N, H, W,
                _n.ptr(wp_t), _n.ptr(y2 if y2 is not None else wp_image), _n.ptr(st2[2]),
                _n.ptr(st2[3]), _n.ptr(st2[0]), _n.ptr(image), _n.ptr(rows) if not rows.wg else None, _n.ptr(ws), _n.ptr(dw),
                cin, cout, _n.ptr(rows) if rows.wg else None, _n.ptr(acorr), 0 if acorr is None else acorr.shape[0],
                _n.ptr(rows.acorr16) if rows.wg else None, _n.stream())

    queue = sink_queue(sink)
    if queue is not None and _TAILS:
        # (kept alive until the flush; the queue takes its device from element 1: a tensor, never the absent dy)
        if queue.capture_tail(sink, (ws, image, dy, y2, rows, wp_image, pooled), launch):
            return None, rows
        return dw, rows
    launch()
    return dw, rows


def _bnrelu_bwd_rows_image3(rows, acorr, w, N, H, W, C, cs, st, training, sinks):
    """BN + ReLU backward of the image block's first conv and its weight gradient from the rows and the autocorrelation
    -> (dW, dgamma, dbeta); dW goes straight into its sink (no tail: the final kernel writes it)"""
    dev = rows.device
    ws = torch.empty(_n.call("spcl_bnrelu_image3_workspace_bytes", cs) // 4, dtype=torch.float32, device=dev)
    dw = _grad_buffer(sinks[0], (C, 1, 3, 3), dev)
    dgamma, dbeta = _grad_buffer(sinks[1], (C,), dev), _grad_buffer(sinks[2], (C,), dev)
    wc = w.detach().contiguous().float()
    if getattr(rows, "wg", 0):  # one row set per workgroup of the one-pass kernel, autocorrelation already folded
        _n.call("spcl_bnrelu_backward_wgrows_image3", _n.ptr(rows), rows.wg, _n.ptr(rows.acorr16), 16, _n.ptr(wc), N, H, W, C,
                cs, _n.ptr(st[0]), _n.ptr(st[1]), _n.ptr(st[2]), int(training), _n.ptr(ws), _n.ptr(dgamma), _n.ptr(dbeta),
                _n.ptr(dw), _n.stream())
        return dw, dgamma, dbeta
    _n.call("spcl_bnrelu_backward_rows_image3", _n.ptr(rows), rows.ntiles, _n.ptr(acorr), acorr.shape[0], _n.ptr(wc), N, H,
            W, C, cs, _n.ptr(st[0]), _n.ptr(st[1]), _n.ptr(st[2]), int(training), _n.ptr(ws), _n.ptr(dgamma), _n.ptr(dbeta),
            _n.ptr(dw), _n.stream())
    return dw, dgamma, dbeta


def _bnrelu_pool_bwd_rows(y, dpool, rows, dt_code, dtype, N, H, W, C, cs, st, training, sinks):
    """BN + ReLU + max-pool backward finished from the rows the next block's dgrad left -> (dy, dgamma, dbeta)."""
    dev = y.device
    ws = torch.empty(_n.call("spcl_bnrelu_bwd_workspace_bytes", N, H, W, cs) // 4, dtype=torch.float32, device=dev)
    dgamma = _grad_buffer(sinks[0], (C,), dev)
    dbeta = _grad_buffer(sinks[1], (C,), dev)
    dy = torch.empty(N, H, W, cs, dtype=dtype, device=dev)
    _n.call("spcl_bnrelu_pool_backward_rows", _n.ptr(y), _n.ptr(dpool), _n.ptr(rows), rows.ntiles, dt_code, N, H, W, C, cs,
            _n.ptr(st[0]), _n.ptr(st[1]), _n.ptr(st[2]), _n.ptr(st[3]), int(training), _n.ptr(ws), _n.ptr(dgamma),
            _n.ptr(dbeta), _n.ptr(dy), _n.stream())
    return dy, dgamma, dbeta


ACC_ROWS = object()  # ``PoolLink.rows`` / a dgrad's ``rows`` when the sums went into a fixed-point accumulator block instead


def _bnrelu_bwd_fill(y, dact, dpool, dt_code, dtype, N, H, W, C, cs, st, training, sinks, acc, dact_stride=0, d_up=None):
    """``_bnrelu_bwd`` whose reduction pass ADDS its sums to the zeroed block ``acc`` and whose apply pass derives the
    coefficients from it (spcl_bnrelu_backward_fill_acc): two launches, no finalize launch -> (dy, dgamma, dbeta)"""
    dev = y.device
    dgamma = _grad_buffer(sinks[0], (C,), dev)
    dbeta = _grad_buffer(sinks[1], (C,), dev)
    dy = torch.empty(N, H, W, cs, dtype=dtype, device=dev)
    if d_up is not None:
        assert dact is None and dpool is None
        dact = torch.empty(N, H, W, cs, dtype=dtype, device=dev)  # (the summed gradient, for the apply pass)
    _n.call("spcl_bnrelu_backward_fill_acc", _n.ptr(y), _n.ptr(dact), int(dact_stride), _n.ptr(dpool), _n.ptr(d_up), dt_code,
            N, H, W, C, cs, _n.ptr(st), int(training), _n.ptr(acc), _n.ptr(dgamma), _n.ptr(dbeta), _n.ptr(dy), _n.stream())
    return dy, dgamma, dbeta


def _bnrelu_bwd_rows_acc(y, dact, dpool, rows, dt_code, dtype, N, H, W, C, cs, st, training, sinks, acc):
    """``_bnrelu_bwd_rows`` / ``_bnrelu_pool_bwd_rows`` with the rows added to the zeroed block ``acc`` by one small launch and
    the apply pass deriving its coefficients from it (spcl_bnrelu_backward_rows_acc): no finalize launch -> (dy, dgamma, dbeta)"""
    dev = y.device
    dgamma = _grad_buffer(sinks[0], (C,), dev)
    dbeta = _grad_buffer(sinks[1], (C,), dev)
    dy = torch.empty(N, H, W, cs, dtype=dtype, device=dev)
    _n.call("spcl_bnrelu_backward_rows_acc", _n.ptr(y), _n.ptr(dact), _n.ptr(dpool), _n.ptr(rows), rows.ntiles, dt_code, N, H, W,
            C, cs, _n.ptr(st), int(training), _n.ptr(acc), _n.ptr(dgamma), _n.ptr(dbeta), _n.ptr(dy), _n.stream())
    return dy, dgamma, dbeta


def _take_acc(ctx, name):
    """the backward accumulator block ``ctx.<name>`` -- ONCE: a block is zero only for the first backward after its forward
    (a second backward through the same graph finds None and takes the rows + finalize path)"""
    acc = getattr(ctx, name, None)
    setattr(ctx, name, None)
    return acc


def _dgrad_bnstats_acc(dy, wp_t, y2, st2, dt_code, dtype, N, H, W, cin_k, cout_s, acc):
    """``_dgrad_bnstats`` with the sums ADDED to the block ``acc`` (spcl_conv3x3_dgrad_bnstats_acc) -> g"""
    g = torch.empty(N, H, W, cout_s, dtype=dtype, device=dy.device)
    _n.call("spcl_conv3x3_dgrad_bnstats_acc", _n.ptr(dy), dt_code, N, H, W, cin_k, cout_s, _n.ptr(wp_t), _n.ptr(g), _n.ptr(y2),
            _n.ptr(st2[2]), _n.ptr(st2[3]), _n.ptr(st2[0]), _n.ptr(acc), _n.stream())
    return g


def _bnrelu_bwd_acc(y, dact, dpool, dact_nc, dt_code, dtype, N, H, W, C, cs, st, training, sinks, acc):
    """BN + ReLU (+ max-pool) backward's apply pass with its coefficients derived from the block ``acc``
    (spcl_bnrelu_backward_acc): exactly one of dact / dpool (block already filled by the dgrad that produced the gradient) or
    dact_nc [N, cs] (this call's reduction pass fills it) -> (dy, dgamma, dbeta)"""
    dev = y.device
    dgamma = _grad_buffer(sinks[0], (C,), dev)
    dbeta = _grad_buffer(sinks[1], (C,), dev)
    dy = torch.empty(N, H, W, cs, dtype=dtype, device=dev)
    assert st.is_contiguous() and tuple(st.shape) == (4, cs)
    _n.call("spcl_bnrelu_backward_acc", _n.ptr(y), _n.ptr(dact), _n.ptr(dpool), _n.ptr(dact_nc), dt_code, N, H, W, C, cs,
            _n.ptr(st), int(training), _n.ptr(acc), _n.ptr(dgamma), _n.ptr(dbeta), _n.ptr(dy), _n.stream())
    return dy, dgamma, dbeta


class _ConvBlockFn(torch.autograd.Function):
    """[conv3x3 -> BN -> ReLU] x2 (+ 2x2 max-pool), semi_seg/arch/unet.py:67-82 + :118-121, as HIP kernels.

    Only the raw conv outputs are kept for backward; BN-apply+ReLU of the first conv is fused into the second conv's
    loader, the second's into the (optional) activation / pooled writers."""

    @staticmethod
    def forward(ctx, x, wa, ga, ba, wb, gb, bb, cfg: BlockCfg, x2=None):
        """``x2``: the block's input is ``torch.cat((x, x2), 1)`` (the decoder's skip concatenation, unet.py:194-224), read
        from the two tensors in place (``cat_pair_supported`` must have said yes): no concatenated tensor in the forward,
        ONE gradient tensor in the backward whose channel halves are returned as views."""
        _n.require_gpu(x, wa, wb)
        dtype, dev = cfg.dtype, x.device
        dtc = _n.dtype_code(dtype)
        N, cin, H, W = x.shape
        cout = wa.shape[0]
        cout_s = _ru16(cout)
        x2s = None
        if x2 is not None:
            xs, x2s = to_nhwc_padded(x.detach(), dtype), to_nhwc_padded(x2.detach(), dtype)
            assert not cfg.image_input and x2.shape == x.shape and xs.shape[3] == cin and x2s.shape[3] == cin \
                and wa.shape[1] == 2 * cin, (tuple(x.shape), tuple(x2.shape), tuple(wa.shape))
            chalf, cin = cin, 2 * cin
            cin_s = cin_k = cin
            mode_a = 0
            xl = getattr(cfg, "x2_link", None)
            if xl is not None:  # x2 is the up-convolution's raw output: its BatchNorm + ReLU happens in the loaders
                assert xl.yb.data_ptr() == x2s.data_ptr() and xl.cs == chalf, "x2 is not the linked producer's output"
            ctx.x2_coef = (xl.stb[2], xl.stb[3]) if xl is not None else (None, None)
        elif cfg.image_input:
            if cin > 16:
                raise NotImplementedError("image-input block supports input_dim <= 16")
            xs = x.detach().float().permute(0, 2, 3, 1).contiguous()  # [N,H,W,cin] f32 (a view when cin == 1)
            cin_s, cin_k, mode_a = cin, 16, 2
        else:
            xs = to_nhwc_padded(x.detach(), dtype)
            cin_s = cin_k = xs.shape[3]
            mode_a = 0
        need_bwd = any(ctx.needs_input_grad)
        ctx.acorr = None
        acorr_rows = 0
        if (need_bwd and ctx.needs_input_grad[1] and not ctx.needs_input_grad[0]
                and _image3_supported(cfg, cin, dtc, N, H, W, cout_s)):
            # of the input image only: usually it came with the forward pass's weight-pack launch (UNet._prepack), else now
            ctx.acorr = take_prepacked_acorr(xs)
            acorr_rows = _acorr_in_conv_rows(dtc, N, H, W, cin, cout_s) if (ctx.acorr is None and x2s is None) else 0
            if ctx.acorr is None and acorr_rows == 0:
                ctx.acorr = _image_autocorr(xs, N, H, W)
        pre_a, pre_b = take_prepacked(wa, dtc, H, W), take_prepacked(wb, dtc, H, W)
        if pre_a is not None and pre_b is not None:  # packed with the other layers at the start of the forward pass
            (wpa, wpa_t), (wpb, wpb_t) = pre_a, pre_b
        elif need_bwd:  # the dgrad layouts are packed alongside (same launch) and kept for backward
            (wpa, wpa_t), (wpb, wpb_t) = _pack_block(wa, wb, dtc, dtype, *((H, W) if _PACK_AT else (0, 0)))
        else:
            wpa, wpb, wpa_t, wpb_t = _pack(wa, 0, dtc, dtype), _pack(wb, 0, dtc, dtype), None, None
        ctx.up2 = bool(getattr(cfg, "up2", False)) and cfg.need_act and not cfg.need_pool
        lazy = (bool(getattr(cfg, "lazy_act", False)) and cfg.need_act and not cfg.need_pool and not ctx.up2
                and getattr(cfg, "act_dst", None) is None)
        # BatchNorm sums through fixed-point accumulator blocks where the layer's kernels offer it (bf16, the specialised
        # convolution kernels, few enough tiles: Conv3 .. Conv5 of the 224^2 step): no finalize launch on either BatchNorm
        count = float(N) * H * W
        acc_ok = _BN_ACC and cfg.training and dtype == torch.bfloat16 and cout_s <= 256 and cout == cout_s
        sup = lambda ci, co, kind, out: bool(_n.call("spcl_conv_bn_acc_supported", dtc, N, H, W, ci, co, kind, out))  # noqa: E731
        use_a = (acc_ok and x2s is None and acorr_rows == 0 and mode_a == 0 and sup(cin_k, cout_s, 0, 1)
                 and sup(cout_s, cout_s, 1, 0))
        use_b = (acc_ok and not lazy and not ctx.up2 and getattr(cfg, "act_dst", None) is None
                 and sup(cout_s, cout_s, 1 if use_a else 2, 1))
        keep = []
        recompute = False
        ctx.acc_bwd_a = ctx.acc_bwd_b = ctx.acc_rows_a = None
        if use_a:
            acc_a = bn_acc_block(cout_s, dev)
            ya, _ = _conv_acc(xs, dtc, dtype, N, H, W, cin_k, cout_s, wpa, None, None, None, acc_a, False)
            sta = torch.empty(4, cout_s, dtype=torch.float32, device=dev)  # written by the second convolution's first workgroup
            bn_a = _bn_acc_desc(acc_a, cfg, cout, cout_s, ga, ba, 0, count, sta, keep)
        else:
            if x2s is not None:
                ya, sa = _conv_cat(xs, x2s, dtc, dtype, N, H, W, chalf, cout_s, wpa, cfg.training, *ctx.x2_coef)
            elif acorr_rows > 0:  # the image convolution leaves the autocorrelation rows of the image3 backward itself
                # ... and, where the second convolution and the block's backward can form its output again from the image,
                # nothing else: ya is never stored.  That needs the rows form of BOTH BatchNorms and the one-pass backward:
                # where Conv1.b's statistics go through an accumulator block (``use_b``: at most 4 096 tiles, N <= 16 at
                # 224^2) the tensor is still stored, whatever spcl_block1_recompute_supported says about the kernels
                recompute = (_BLOCK1_RECOMPUTE and _CONV16_FUSED and cfg.training and not use_b and cin == 1
                             and cout == cout_s and ctx.needs_input_grad[4]
                             and bool(_n.call("spcl_block1_recompute_supported", dtc, N, H, W, cin_s, cout_s)))
                ya, sa, ctx.acorr = _conv_image_acorr(xs, dtc, dtype, N, H, W, cin_s, cout_s, wpa, cfg.training, acorr_rows,
                                                      store=not recompute)
            else:
                ya, sa = _conv(xs, dtc, dtype, N, H, W, cin_s, cin_k, cout_s, wpa, mode_a, None, None, cfg.training)
            sta = _bn_stats(sa, cfg, cout, cout_s, ga, ba, 0, dev)
        if use_a or use_b:
            acc_b = bn_acc_block(cout_s, dev) if use_b else None
            yb, sb = _conv_acc(ya, dtc, dtype, N, H, W, cout_s, cout_s, wpb, bn_a if use_a else None,
                               None if use_a else sta[2], None if use_a else sta[3], acc_b, cfg.training)
        elif recompute:
            yb, sb = _conv_from_image(xs, None, dtc, dtype, N, H, W, cout_s, wpa, sta[2], sta[3], wpb, cfg.training)
        else:
            yb, sb = _conv(ya, dtc, dtype, N, H, W, cout_s, cout_s, cout_s, wpb, 1, sta[2], sta[3], cfg.training)
        ctx.wpa_fwd = wpa if recompute else None  # (the backward forms ya from the image with them)
        if use_b:
            stb = torch.empty(4, cout_s, dtype=torch.float32, device=dev)  # written by the activation writer's first workgroup
            bn_b = _bn_acc_desc(acc_b, cfg, cout, cout_s, gb, bb, 1, count, stb, keep)
        else:
            stb = _bn_stats(sb, cfg, cout, cout_s, gb, bb, 1, dev)
        if acc_ok and any(ctx.needs_input_grad):
            # the backward's blocks are zeroed with the forward's (one fill per step): sum dz / sum dz (y - mean) of both
            # BatchNorms, added by whichever kernel produces the incoming gradient
            if not cfg.image_input and _n.call("spcl_conv_dgrad_bnstats_acc_supported", dtc, N, H, W, cout_s, cout_s):
                ctx.acc_bwd_a = bn_acc_block(cout_s, dev)
            elif not cfg.image_input and _ACC_FILL:
                ctx.acc_rows_a = bn_acc_block(cout_s, dev)  # (more tiles than a block takes adds from: the dgrad's ROWS go in)
            ctx.acc_bwd_b = bn_acc_block(cout_s, dev)
        # small maps whose activation is the block's only product (the encoder's last block under a feature tap): the writer
        # also leaves the activation's global average per (image, channel) -- the projector's AdaptiveAvgPool2d((1, 1)) then
        # has nothing to read back (conv_block hangs it on the returned tensor, _ProjectorFn looks for it)
        cfg.gap = None
        want_gap = (_GAP and getattr(cfg, "want_gap", False) and cfg.need_act and not cfg.need_pool and not lazy
                    and not ctx.up2 and cfg.act_dst is None
                    and H * W <= 1024 and _n.call("spcl_bnrelu_gap_supported", dtc, H, W, cout, cout_s))
        # a training block whose ONLY product is the pooled activation offers the next block a PoolLink (below): its writer then also
        # leaves the window maxima's raw values where that pays (training with a backward only: eval / inference write nothing)
        offers_link = need_bwd and cfg.need_pool and not cfg.need_act and cfg.training and dtype == torch.bfloat16
        want_ymax = (offers_link and cfg.grad_mode and not want_gap and not lazy and not ctx.up2 and H >= 2 and W >= 2
                     and _pool_ymax_pays(N, H, W, cout_s))
        ymax = None
        if want_gap:
            act, pool = torch.empty(N, H, W, cout_s, dtype=dtype, device=dev), None
            cfg.gap = torch.empty(N, cout, dtype=torch.float32, device=dev)
            _n.call("spcl_bnrelu_gap_forward", _n.ptr(yb), dtc, N, H, W, cout, cout_s, None if use_b else _n.ptr(stb[2]),
                    None if use_b else _n.ptr(stb[3]), ctypes.byref(bn_b) if use_b else None, _n.ptr(act), _n.ptr(cfg.gap),
                    _n.stream())
        elif use_b:
            act = torch.empty(N, H, W, cout_s, dtype=dtype, device=dev) if cfg.need_act else None
            pool = torch.empty(N, H // 2, W // 2, cout_s, dtype=dtype, device=dev) if cfg.need_pool else None
            if want_ymax:
                ymax = torch.empty_like(pool)
                _n.call("spcl_bnrelu_pool_forward_ymax", _n.ptr(yb), dtc, N, H, W, cout_s, None, None, ctypes.byref(bn_b),
                        None, _n.ptr(pool), _n.ptr(ymax), _n.stream())
            else:
                _n.call("spcl_bnrelu_pool_forward_acc", _n.ptr(yb), dtc, N, H, W, cout_s, ctypes.byref(bn_b), _n.ptr(act),
                        _n.ptr(pool), _n.stream())
        elif lazy:
            # no activation tensor: the consumer (conv1x1_bn) reads yb and applies scale / shift / ReLU in its loader
            act, pool = yb, None
            cfg.link_act = ActLink(yb, stb, N, H, W, cout, cout_s)
        elif ctx.up2:
            act = torch.empty(N, 2 * H, 2 * W, cout_s, dtype=dtype, device=dev)
            pool = None
            _n.call("spcl_bnrelu_up2_forward", _n.ptr(yb), dtc, N, H, W, cout_s, _n.ptr(stb[2]), _n.ptr(stb[3]), _n.ptr(act),
                    _n.stream())
        else:
            act = _act_buffer(cfg, N, H, W, cout_s, dtype, dev) if cfg.need_act else None
            pool = torch.empty(N, H // 2, W // 2, cout_s, dtype=dtype, device=dev) if cfg.need_pool else None
            if want_ymax:
                ymax = torch.empty_like(pool)
                _n.call("spcl_bnrelu_pool_forward_ymax", _n.ptr(yb), dtc, N, H, W, cout_s, _n.ptr(stb[2]), _n.ptr(stb[3]), None,
                        None, _n.ptr(pool), _n.ptr(ymax), _n.stream())
            else:
                _bnrelu_fwd(yb, dtc, N, H, W, cout_s, stb[2], stb[3], act, pool)
        ctx.save_for_backward(xs, ya, yb, sta, stb, wa, wb)
        ctx.x2s = x2s  # (not an input of this Function as a tensor object: a detached re-layout, kept directly)
        ctx.params = (wa, ga, ba, wb, gb, bb)
        ctx.packed_t = (wpa_t, wpb_t)
        ctx.cfg = cfg
        if need_bwd and pool is not None and act is None and cfg.training and dtype == torch.bfloat16:
            cfg.link_out = PoolLink(yb, stb, N, H, W, cout_s, ctx.acc_bwd_b, ymax)  # the pooled output is this block's only product
        ctx.meta = (N, cin, H, W, cout, cout_s, cin_s, cin_k, mode_a, x.dtype)
        outs = []
        outs.append(nhwc_to_logical(act, cout) if act is not None else None)
        outs.append(nhwc_to_logical(pool, cout) if pool is not None else None)
        return tuple(outs)

    @staticmethod
    def backward(ctx, d_act, d_pool):
        xs, ya, yb, sta, stb, wa, wb = ctx.saved_tensors
        cfg = ctx.cfg
        N, cin, H, W, cout, cout_s, cin_s, cin_k, mode_a, xdt = ctx.meta
        dtype = cfg.dtype
        dtc = _n.dtype_code(dtype)
        g_nc = broadcast_rows(d_act, dtype) if (_BCAST and d_pool is None and d_act is not None and not ctx.up2
                                                  and d_act.shape[1] == cout_s) else None
        d_up = None
        ul = getattr(cfg, "up_link", None)
        if ul is not None and ul.d_up is not None:
            # the consuming up-convolution left its FINE input gradient in the link (UpLink) and sent an unwritten tensor
            # (compared while the link still holds the unwritten tensor: released first, its address is the first thing the
            # allocator hands out again -- to the very re-layout copy a foreign gradient would need)
            du, holder = ul.d_up, ul.holder
            same = (d_act is not None and d_pool is None and d_act.data_ptr() == ul.dx_ptr and d_act.dtype == holder.dtype
                    and holder._version == ul.version and nhwc_channel_slice(d_act, dtype) is None
                    and to_nhwc_padded(d_act, dtype).data_ptr() == ul.dx_ptr)
            dirty = holder._version != ul.version  # (somebody wrote INTO the shared zeros: what they hold now is that gradient)
            ul.d_up, ul.dx_ptr, ul.holder = None, 0, None
            if same:
                d_up, d_act = du, None
            else:
                # somebody else contributed to this activation's gradient: what arrived is THEIR part (the link's tensor
                # holds zeros), the 2 x 2 sums of the up-convolution's fine gradient are added here -- the ordinary kernels
                gs = torch.empty(N, H, W, cout_s, dtype=dtype, device=du.device)
                _n.call("spcl_upsample2x_backward", _n.ptr(du), _n.ptr(gs), dtc, N, H, W, cout_s, _n.stream())
                gl = nhwc_to_logical(gs, cout)
                d_act = gl if d_act is None else d_act.to(gl.dtype) + gl
                if dirty:
                    holder.zero_()  # (restore the shared tensor for its next use)
        elif ctx.up2 and d_act is not None:
            # the forward returned the x2-upsampled activation: its gradient is summed over the 2x2 replicas first -- inside
            # the BatchNorm-backward reduction pass (spcl_bnrelu_backward_up2), or by its own launch
            du = to_nhwc_padded(d_act, dtype)
            if _UP2_BWD_FUSED and d_pool is None:
                d_up, d_act = du, None
            else:
                dsum = torch.empty(N, H, W, cout_s, dtype=dtype, device=du.device)
                _n.call("spcl_upsample2x_backward", _n.ptr(du), _n.ptr(dsum), dtc, N, H, W, cout_s, _n.stream())
                d_act = nhwc_to_logical(dsum, cout)
        da_stride = 0
        da_sl = nhwc_channel_slice(d_act, dtype) if (d_act is not None and g_nc is None) else None
        if da_sl is not None:  # the skip half of a concatenation's gradient, read in place (spcl_bnrelu_pool_backward_strided)
            da_s, da_stride = da_sl
        else:
            da_s = to_nhwc_padded(d_act, dtype) if (d_act is not None and g_nc is None) else None
        dp_s = to_nhwc_padded(d_pool, dtype) if d_pool is not None else None
        if da_s is None and dp_s is None and g_nc is None and d_up is None:
            return (None,) * 9
        x2s = ctx.x2s
        # ---- second conv
        ng = ctx.needs_input_grad
        sk = tuple(take_grad_sink(p, ng[i + 1]) for i, p in enumerate(ctx.params))  # (wa, ga, ba, wb, gb, bb)
        lk = cfg.link_out
        la = getattr(cfg, "link_act", None)
        pooled = None  # (set where dyb is not materialised: ``_BLOCK1_POOLED_BWD``)
        if la is not None and da_s is not None and dp_s is None and da_stride == 0 and la.fresh(da_s.data_ptr()):
            # the consumer's backward (the 1x1 head) left this BatchNorm's partial sums next to the activation gradient
            dyb, dgb, dbb = _bnrelu_bwd_rows(yb, da_s, None, la.rows, dtc, dtype, N, H, W, cout, cout_s, stb, cfg.training,
                                             sk[4:6])
        elif g_nc is not None:
            # the block's output fed a global average pool only: its gradient is one value per (image, channel)
            acc = _take_acc(ctx, "acc_bwd_b")
            if acc is not None:  # (reduction pass adds into the block, the apply pass derives its coefficients: no finalize)
                dyb, dgb, dbb = _bnrelu_bwd_acc(yb, None, None, g_nc, dtc, dtype, N, H, W, cout, cout_s, stb, cfg.training,
                                                sk[4:6], acc)
            else:
                dyb, dgb, dbb = _bnrelu_bwd_bcast(yb, g_nc, dtc, dtype, N, H, W, cout, cout_s, stb, cfg.training, sk[4:6])
        elif lk is not None and da_s is None and dp_s is not None and lk.fresh(dp_s.data_ptr()):
            # the next block's input-gradient kernel left this BatchNorm's partial sums next to the gradient itself
            if lk.rows is ACC_ROWS:  # ... in this block's accumulator block
                dyb, dgb, dbb = _bnrelu_bwd_acc(yb, None, dp_s, None, dtc, dtype, N, H, W, cout, cout_s, stb, cfg.training,
                                                sk[4:6], _take_acc(ctx, "acc_bwd_b"))
            else:
                acc = _take_acc(ctx, "acc_bwd_b") if (_ACC_FILL and H % 2 == 0 and W % 2 == 0 and cout_s <= 256) else None
                if (acc is not None and _BLOCK1_POOLED_BWD and ya is None and ctx.acorr is not None and ctx.wpa_fwd is not None
                        and ctx.needs_input_grad[4] and cout == cout_s and dtype == torch.bfloat16
                        and _n.call("spcl_conv16_bwd_fused_image_pooled_supported", dtc, N, H, W, cout_s, cout_s,
                                    int(cfg.training))):
                    # the image block with its first convolution recomputed: this gradient's ONE reader is the one-pass
                    # backward of Conv1.b below, which forms it per tile from yb and the pooled gradient -- no tensor, no
                    # apply launch; that call adds the rows to the block and leaves dgamma / dbeta
                    dyb = None
                    dgb, dbb = _grad_buffer(sk[4], (cout,), yb.device), _grad_buffer(sk[5], (cout,), yb.device)
                    # (views of their own for the call: ``pooled`` stays alive in the weight-gradient queue until its flush,
                    # and a gradient somebody else still holds is CLONED by autograd instead of adopted as ``param.grad`` --
                    # two copies and, the sink then unclaimed, an addition into the bucket per step)
                    pooled = (yb, dp_s, lk.rows, stb, acc, dgb.view(cout), dbb.view(cout), cfg.training)
                elif acc is not None:  # (the rows go into this block's own, untouched, accumulator block: no finalize launch)
                    dyb, dgb, dbb = _bnrelu_bwd_rows_acc(yb, None, dp_s, lk.rows, dtc, dtype, N, H, W, cout, cout_s, stb,
                                                         cfg.training, sk[4:6], acc)
                else:
                    dyb, dgb, dbb = _bnrelu_pool_bwd_rows(yb, dp_s, lk.rows, dtc, dtype, N, H, W, cout, cout_s, stb,
                                                          cfg.training, sk[4:6])
        else:
            acc = _take_acc(ctx, "acc_bwd_b") if _ACC_FILL else None
            if acc is not None and lk is not None and lk.rows is ACC_ROWS:
                # the next block's input-gradient kernel ADDED its sums to this block already -- of a gradient that then got
                # company (a second consumer of the pooled tensor): the block is not zero any more, and its content is not
                # this gradient's
                acc = None
            if acc is not None:
                # a gradient that did not come with its sums (several consumers: the decoder's skip connections): the reduction
                # pass adds them to the block, the apply pass derives its coefficients -- no finalize launch
                dyb, dgb, dbb = _bnrelu_bwd_fill(yb, da_s, dp_s, dtc, dtype, N, H, W, cout, cout_s, stb, cfg.training, sk[4:6],
                                                 acc, dact_stride=da_stride, d_up=d_up)
            else:
                dyb, dgb, dbb = _bnrelu_bwd(yb, da_s, dp_s, dtc, dtype, N, H, W, cout, cout_s, stb, cfg.training, sk[4:6],
                                            dact_stride=da_stride, d_up=d_up)
        if lk is not None:
            lk.rows, lk.dx_ptr, lk.holder = None, 0, None
        if la is not None:
            la.rows, la.dx_ptr, la.holder = None, 0, None
        wpa_t, wpb_t = ctx.packed_t
        if wpb_t is None:
            wpb_t = _pack(wb, 1, dtc, dtype)
        image3 = ctx.acorr is not None
        # image block: this conv's weight gradient AND the sums the first conv's backward needs in one pass over dyb / ya
        one_pass = (image3 and (_CONV16_FUSED or ya is None) and ctx.needs_input_grad[4] and cout == cout_s
                    and _n.call("spcl_conv16_bwd_fused_supported", dtc, N, H, W, cout_s, cout_s))
        if ya is None and not one_pass:  # (the forward offered the recomputation where this holds: never a silent fallback)
            raise RuntimeError("image block backward: the first convolution's output was not stored and the one-pass kernel "
                               "that forms it again is not available")
        if pooled is not None and not one_pass:  # (taken only where the one-pass kernel runs: never a silent fallback)
            raise RuntimeError("image block backward: the gradient behind the max-pool was not materialised and the one-pass "
                               "kernel that forms it is not available")
        if one_pass:
            dwb, rows16 = _conv16_bwd_fused(dyb, wpb_t, ya, sta, xs, dtc, N, H, W, cout, cout, cout_s, sk[3],
                                            acorr=ctx.acorr if _CONV16_WGROWS else None, wp_image=ctx.wpa_fwd, pooled=pooled)
        else:
            dwb = _wgrad(ya, dyb, dtc, N, H, W, cout, cout_s, cout_s, cout, cout_s, 1, sta[2], sta[3], sk[3]) \
                if ctx.needs_input_grad[4] else None
        # the dgrad's output is d loss / d relu(bn_a(ya)): where a specialised kernel exists its epilogue also leaves the
        # per-tile partial sums of bn_a's backward (no separate reduction pass over ya and the gradient)
        if one_pass:
            fused = (None, rows16)
        elif image3:
            fused = _dgrad_bnstats_image(dyb, wpb_t, ya, sta, xs, dtc, dtype, N, H, W, cout_s)
        else:
            acc = _take_acc(ctx, "acc_bwd_a")
            if acc is not None:  # the sums go into the block, the apply pass below derives its coefficients from it
                fused = (_dgrad_bnstats_acc(dyb, wpb_t, ya, sta, dtc, dtype, N, H, W, cout_s, cout_s, acc), (ACC_ROWS, acc))
            else:
                fused = _dgrad_bnstats(dyb, wpb_t, ya, sta, dtc, dtype, N, H, W, cout_s, cout_s) \
                    if dtype == torch.bfloat16 else None
        if fused is not None:
            daa, rows = fused
        else:
            daa, _ = _conv(dyb, dtc, dtype, N, H, W, cout_s, cout_s, cout_s, wpb_t, 0, None, None, False)
        # ---- first conv
        image_fused = ctx.needs_input_grad[1] and not ctx.needs_input_grad[0] and _image_wgrad_fusable(cfg, cin, cout_s)
        if image3:
            dya = None  # no pass over ya / the gradient at all: rows + image autocorrelation -> dW, dgamma, dbeta
            dwa, dga, dba = _bnrelu_bwd_rows_image3(rows, ctx.acorr, wa, N, H, W, cout, cout_s, sta, cfg.training, sk[0:3])
        elif image_fused:
            dya = None  # dy of this layer feeds only dW: one fused pass, nothing written
            if fused is not None:
                dwa, dga, dba = _bnrelu_bwd_rows(ya, daa, xs, rows, dtc, dtype, N, H, W, cout, cout_s, sta, cfg.training,
                                                 sk[0:3])
            else:
                dwa, dga, dba = _bnrelu_bwd_image_wgrad(ya, daa, xs, dtc, N, H, W, cout, cout_s, sta, cfg.training,
                                                        sk[0:3])
        else:
            if fused is not None and isinstance(rows, tuple) and rows[0] is ACC_ROWS:
                dya, dga, dba = _bnrelu_bwd_acc(ya, daa, None, None, dtc, dtype, N, H, W, cout, cout_s, sta, cfg.training,
                                                sk[1:3], rows[1])
            elif fused is not None:
                acc = _take_acc(ctx, "acc_rows_a")
                if acc is not None:
                    dya, dga, dba = _bnrelu_bwd_rows_acc(ya, daa, None, rows, dtc, dtype, N, H, W, cout, cout_s, sta,
                                                         cfg.training, sk[1:3], acc)
                else:
                    dya, dga, dba = _bnrelu_bwd_rows(ya, daa, None, rows, dtc, dtype, N, H, W, cout, cout_s, sta,
                                                     cfg.training, sk[1:3])
            else:
                dya, dga, dba = _bnrelu_bwd(ya, daa, None, dtc, dtype, N, H, W, cout, cout_s, sta, cfg.training,
                                            sk[1:3])
            if not ctx.needs_input_grad[1]:
                dwa = None
            elif x2s is not None:
                dwa = _wgrad_cat(xs, x2s, dya, dtc, N, H, W, cin // 2, cout, cout_s, sk[0], *ctx.x2_coef)
            else:
                dwa = _wgrad(xs, dya, dtc, N, H, W, cin, cin_s, cin_k, cout, cout_s, mode_a, None, None, sk[0])
        dx = dx2 = None
        if ctx.needs_input_grad[0] or (x2s is not None and ctx.needs_input_grad[8]):
            if cfg.image_input:
                raise NotImplementedError("gradient w.r.t. the input image is not on the hot path")
            if wpa_t is None:
                wpa_t = _pack(wa, 1, dtc, dtype)
            li = cfg.link_in
            dxs = None
            if (li is not None and dtype == torch.bfloat16 and li.cout_s == cin_s and li.N == N
                    and _n.call("spcl_conv_dgrad_poolstats_supported", dtc, N, H, W, cout_s, cin_s, li.H, li.W)):
                dxs = torch.empty(N, H, W, cin_s, dtype=dtype, device=dya.device)
                # the producer's pooled forward left the window maxima (``_pool_ymax_pays``): the epilogue reads that tensor, a
                # quarter of ``li.yb``'s bytes, and leaves the same bits (spcl_conv3x3_dgrad_poolmax)
                ym = li.ymax if (li.ymax is not None and tuple(li.ymax.shape) == (N, H, W, cin_s)) else None
                if (li.acc is not None and _n.call("spcl_conv_dgrad_poolstats_acc_supported", dtc, N, H, W, cout_s, cin_s,
                                                   li.H, li.W)):
                    # ... added to the producing block's accumulator block (zeroed with its forward): no rows, no finalize.
                    # Taken ONCE, like ``_take_acc``: the block is zero only for the first backward after its forward; a second
                    # backward through the same graph (retain_graph=True) finds None here and writes rows
                    acc_in, li.acc = li.acc, None
                    if ym is not None and _n.call("spcl_conv_dgrad_poolmax_acc_supported", dtc, N, H, W, cout_s, cin_s):
                        _n.call("spcl_conv3x3_dgrad_poolmax_acc", _n.ptr(dya), dtc, N, H, W, cout_s, cin_s, _n.ptr(wpa_t),
                                _n.ptr(dxs), _n.ptr(ym), _n.ptr(li.stb[2]), _n.ptr(li.stb[3]), _n.ptr(li.stb[0]),
                                _n.ptr(acc_in), _n.stream())
                    else:
                        _n.call("spcl_conv3x3_dgrad_poolstats_acc", _n.ptr(dya), dtc, N, H, W, cout_s, cin_s, _n.ptr(wpa_t),
                                _n.ptr(dxs), _n.ptr(li.yb), li.H, li.W, _n.ptr(li.stb[2]), _n.ptr(li.stb[3]),
                                _n.ptr(li.stb[0]), _n.ptr(acc_in), _n.stream())
                    rows = ACC_ROWS
                else:
                    nt = _n.call("spcl_conv_stat_rows", dtc, N, H, W, cout_s, cin_s)
                    rows = torch.empty(nt * 2 * cin_s, dtype=torch.float32, device=dya.device)
                    if ym is not None and _n.call("spcl_conv_dgrad_poolmax_supported", dtc, N, H, W, cout_s, cin_s):
                        _n.call("spcl_conv3x3_dgrad_poolmax", _n.ptr(dya), dtc, N, H, W, cout_s, cin_s, _n.ptr(wpa_t),
                                _n.ptr(dxs), _n.ptr(ym), _n.ptr(li.stb[2]), _n.ptr(li.stb[3]), _n.ptr(li.stb[0]),
                                _n.ptr(rows), _n.stream())
                    else:
                        _n.call("spcl_conv3x3_dgrad_poolstats", _n.ptr(dya), dtc, N, H, W, cout_s, cin_s, _n.ptr(wpa_t),
                                _n.ptr(dxs), _n.ptr(li.yb), li.H, li.W, _n.ptr(li.stb[2]), _n.ptr(li.stb[3]),
                                _n.ptr(li.stb[0]), _n.ptr(rows), _n.stream())
                    rows.ntiles = nt
                li.rows, li.dx_ptr, li.holder, li.version = rows, dxs.data_ptr(), dxs, dxs._version
                li.ymax = None  # (its one reader has run: a second backward through the graph reads ``li.yb``, same bits)
            split = None
            if (dxs is None and x2s is not None and _CONV_SPLIT
                    and _n.call("spcl_conv_split_supported", dtc, N, H, W, cout_s, cin_s)):
                # the concatenation's gradient as the two dense gradients of its parts (one launch, no interleaved tensor)
                split = (torch.empty(N, H, W, cin_s // 2, dtype=dtype, device=dya.device),
                         torch.empty(N, H, W, cin_s // 2, dtype=dtype, device=dya.device))
                xb = getattr(cfg, "x2_bn", None)
                if (xb is not None and xb.cs == cin_s // 2 and (xb.N, xb.H, xb.W) == (N, H, W) and cfg.training
                        and _n.call("spcl_conv_split_bnstats_supported", dtc, N, H, W, cout_s, cin_s)):
                    # ... and the up-convolution's BatchNorm-backward sums in the same epilogue (its reduction pass disappears)
                    nt = _n.call("spcl_conv_stat_rows", dtc, N, H, W, cout_s, cin_s)
                    rows = torch.empty(nt * 2 * (cin_s // 2), dtype=torch.float32, device=dya.device)
                    rows.ntiles = nt
                    _n.call("spcl_conv3x3_dgrad_split_bnstats", _n.ptr(dya), dtc, N, H, W, cout_s, cin_s, _n.ptr(wpa_t),
                            _n.ptr(split[0]), _n.ptr(split[1]), _n.ptr(xb.yb), _n.ptr(xb.stb[2]), _n.ptr(xb.stb[3]),
                            _n.ptr(xb.stb[0]), _n.ptr(rows), _n.stream())
                    xb.rows, xb.dx_ptr, xb.holder, xb.version = rows, split[1].data_ptr(), split[1], split[1]._version
                else:
                    _n.call("spcl_conv3x3_forward_split", _n.ptr(dya), dtc, N, H, W, cout_s, cin_s, _n.ptr(wpa_t),
                            _n.ptr(split[0]), _n.ptr(split[1]), _n.stream())
            elif dxs is None:
                dxs, _ = _conv(dya, dtc, dtype, N, H, W, cout_s, cout_s, cin_s, wpa_t, 0, None, None, False)
            if x2s is not None:
                if split is not None:
                    dx, dx2 = nhwc_to_logical(split[0], cin // 2), nhwc_to_logical(split[1], cin // 2)
                else:
                    # one gradient tensor for the concatenation; each producer's backward reads its channel half in place
                    # (nhwc_channel_slice -> the _strided BatchNorm entry points)
                    full = dxs.permute(0, 3, 1, 2)
                    dx, dx2 = full[:, :cin // 2], full[:, cin // 2:]
                if dx.dtype != xdt:
                    dx, dx2 = dx.to(xdt), dx2.to(xdt)
                if not ctx.needs_input_grad[0]:
                    dx = None
                if not ctx.needs_input_grad[8]:
                    dx2 = None
            else:
                dx = nhwc_to_logical(dxs, cin)
                if dx.dtype != xdt:
                    dx = dx.to(xdt)
        ng = ctx.needs_input_grad
        return (dx, dwa, dga if ng[2] else None, dba if ng[3] else None, dwb, dgb if ng[5] else None,
                dbb if ng[6] else None, None, dx2)


def conv_block(x, wa, ga, ba, wb, gb, bb, cfg: BlockCfg, x2=None):
    """-> (act or None, pooled or None), logical NCHW views over NHWC storage.  ``x2``: see ``_ConvBlockFn.forward``."""
    cfg.grad_mode = torch.is_grad_enabled()
    act, pool = _ConvBlockFn.apply(x, wa, ga, ba, wb, gb, bb, cfg, x2)
    gap = getattr(cfg, "gap", None)
    if gap is not None and act is not None:
        # the activation's global average, left by its writer: valid while the tensor is not written in place (its version
        # counter says so); a slice / copy of the tensor simply does not carry it and is pooled the ordinary way
        act._spcl_gap = (gap, act._version)
        cfg.gap = None
    return act, pool


def _gap_of(feat, N, C):
    """the [N, C] global average the producer of ``feat`` left on it (``conv_block``), if still valid, else None"""
    gap = getattr(feat, "_spcl_gap", None)
    if (gap is None or gap[1] != feat._version or tuple(gap[0].shape) != (N, C) or gap[0].device != feat.device
            or tuple(feat.shape[:2]) != (N, C)):
        return None
    return gap[0]


def cat_pair_shape_ok(N, C, H, W, cout, dtype):
    """``cat_pair_supported`` for two dense NHWC tensors of this shape that do not exist yet (UNet.forward plans with it)"""
    return bool(_CONV_CAT and dtype == torch.bfloat16
                and _n.call("spcl_conv_cat_supported", _n.dtype_code(dtype), N, H, W, C, _ru16(cout)))


def cat_pair_supported(a, b, cout, dtype):
    """can ``conv_block(a, ..., x2=b)`` stand for ``conv_block(torch.cat((a, b), 1), ...)``?  (two dense bf16 NHWC tensors of
    16 or 32 channels each at a size the specialised convolution kernels tile: spcl_conv_cat_supported)"""
    if not (_CONV_CAT and a.is_cuda and b.is_cuda and a.shape == b.shape and a.dim() == 4 and dtype == torch.bfloat16
            and a.dtype == dtype and b.dtype == dtype):
        return False
    N, C, H, W = a.shape
    for t in (a, b):
        st, cs = as_nhwc(t)
        if cs != C or (st.data_ptr() % 16):
            return False
    return bool(_n.call("spcl_conv_cat_supported", _n.dtype_code(dtype), N, H, W, C, _ru16(cout)))


# --------------------------------------------------------------------------------------------- decoder / head (N1)
class _ConvBNReLUFn(torch.autograd.Function):
    """conv3x3 -> BN -> ReLU, ONCE (the conv of ``_UpConv``, semi_seg/arch/unet.py:85-97, after its nearest upsample),
    from the same kernels as the two-conv block: conv with statistics epilogue, finalize, BN-apply+ReLU writer;
    backward = BN-ReLU backward (2 passes), wgrad, dgrad."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, cfg: BlockCfg):
        _n.require_gpu(x, w)
        dtype, dev = cfg.dtype, x.device
        dtc = _n.dtype_code(dtype)
        N, cin, H, W = x.shape
        up_in = bool(getattr(cfg, "up_in", False))
        if up_in:
            H, W = 2 * H, 2 * W  # the convolution's size: x is the half-resolution tensor, upsampled by the loaders
        cout = w.shape[0]
        cout_s = _ru16(cout)
        xs = to_nhwc_padded(x.detach(), dtype)
        cin_s = xs.shape[3]
        need_bwd = any(ctx.needs_input_grad)
        pre = take_prepacked(w, dtc, H, W)
        if pre is not None:
            wp, wp_t = pre
        elif need_bwd:
            wp, wp_t = _pack_both(w, dtc, dtype)
        else:
            wp, wp_t = _pack(w, 0, dtc, dtype), None
        if up_in:
            assert cin_s == cin, "the in-place upsample needs an unpadded channel count"
            y = torch.empty(N, H, W, cout_s, dtype=dtype, device=dev)
            s = None
            if cfg.training:
                nt = _n.call("spcl_conv_stat_rows", dtc, N, H, W, cin_s, cout_s)
                s = torch.empty(_n.call("spcl_bn_stats_elems", nt, cout_s), dtype=torch.float32, device=dev)
                s.ntiles = nt
            _n.call("spcl_conv3x3_forward_up2", _n.ptr(xs), dtc, N, H, W, cin_s, cout_s, _n.ptr(wp), _n.ptr(y), _n.ptr(s),
                    _n.stream())
        else:
            y, s = _conv(xs, dtc, dtype, N, H, W, cin_s, cin_s, cout_s, wp, 0, None, None, cfg.training)
        st = _bn_stats(s, cfg, cout, cout_s, gamma, beta, 0, dev)
        if bool(getattr(cfg, "lazy_act", False)) and getattr(cfg, "act_dst", None) is None and cout == cout_s:
            # the only consumer (the next block's two-tensor convolution) applies this BatchNorm + ReLU in its loaders
            act = y
            cfg.link_act = ActLink(y, st, N, H, W, cout, cout_s)
        else:
            act = _act_buffer(cfg, N, H, W, cout_s, dtype, dev)
            _bnrelu_fwd(y, dtc, N, H, W, cout_s, st[2], st[3], act, None)
        ctx.save_for_backward(xs, y, st, w)
        ctx.params = (w, gamma, beta)
        ctx.packed_t = wp_t
        ctx.cfg = cfg
        # a block of the step's (zeroed) accumulator arena for the backward's sums: reduction pass adds, apply pass derives
        ctx.acc_bwd = (bn_acc_block(cout_s, dev) if (_BN_ACC and _ACC_FILL and need_bwd and cfg.training and cout_s <= 256
                                                     and dtype == torch.bfloat16) else None)
        cfg.bn_link = ActLink(y, st, N, H, W, cout, cout_s) if (need_bwd and cout == cout_s) else None
        ctx.meta = (N, cin, H, W, cout, cout_s, cin_s, x.dtype)
        ctx.up_in = up_in
        return nhwc_to_logical(act, cout)

    @staticmethod
    def backward(ctx, d_act):
        xs, y, st, w = ctx.saved_tensors
        cfg = ctx.cfg
        N, cin, H, W, cout, cout_s, cin_s, xdt = ctx.meta
        up_in = ctx.up_in
        dtype = cfg.dtype
        dtc = _n.dtype_code(dtype)
        da_sl = nhwc_channel_slice(d_act, dtype)
        da_s, da_stride = da_sl if da_sl is not None else (to_nhwc_padded(d_act, dtype), 0)
        ng = ctx.needs_input_grad
        sk = tuple(take_grad_sink(p, ng[i + 1]) for i, p in enumerate(ctx.params))
        bl = getattr(cfg, "bn_link", None)
        if bl is not None and da_stride == 0 and bl.fresh(da_s.data_ptr()):
            # the consumer's input-gradient kernel left this BatchNorm's backward sums next to the gradient itself
            dy, dg, db = _bnrelu_bwd_rows(y, da_s, None, bl.rows, dtc, dtype, N, H, W, cout, cout_s, st, cfg.training, sk[1:3])
        else:
            acc = _take_acc(ctx, "acc_bwd")
            if acc is not None:
                dy, dg, db = _bnrelu_bwd_fill(y, da_s, None, dtc, dtype, N, H, W, cout, cout_s, st, cfg.training, sk[1:3], acc,
                                              dact_stride=da_stride)
            else:
                dy, dg, db = _bnrelu_bwd(y, da_s, None, dtc, dtype, N, H, W, cout, cout_s, st, cfg.training, sk[1:3],
                                         dact_stride=da_stride)
        if bl is not None:
            bl.rows, bl.dx_ptr, bl.holder = None, 0, None
        if not ctx.needs_input_grad[1]:
            dw = None
        elif up_in:
            dw = _wgrad_up2(xs, dy, dtc, N, H, W, cin, cout, cout_s, sk[0])
        else:
            dw = _wgrad(xs, dy, dtc, N, H, W, cin, cin_s, cin_s, cout, cout_s, 0, None, None, sk[0])
        dx = None
        if ctx.needs_input_grad[0]:
            wp_t = ctx.packed_t if ctx.packed_t is not None else _pack(w, 1, dtc, dtype)
            dxs, _ = _conv(dy, dtc, dtype, N, H, W, cout_s, cout_s, cin_s, wp_t, 0, None, None, False)
            if up_in:  # the gradient w.r.t. the half-resolution input: the 2 x 2 sums of the fine gradient
                ul = getattr(cfg, "up_link", None)
                if ul is not None and _UP2_BWD_FUSED and cfg.training:
                    # the producing block forms the sums (UpLink); what travels through autograd in their place is a shared
                    # tensor of ZEROS (one per shape, never written: the cache's reference keeps autograd from accumulating
                    # into it in place) -- a second consumer of the activation then adds its gradient to zeros, and the block,
                    # which sees a tensor that is not this one, adds the sums to that (it used to be unwritten
                    # memory, and the block could only refuse)
                    dsum = _up_zeros(N, H // 2, W // 2, cin_s, dtype, dxs.device)
                    ul.d_up, ul.dx_ptr, ul.holder, ul.version = dxs, dsum.data_ptr(), dsum, dsum._version
                else:
                    dsum = torch.empty(N, H // 2, W // 2, cin_s, dtype=dtype, device=dxs.device)
                    _n.call("spcl_upsample2x_backward", _n.ptr(dxs), _n.ptr(dsum), dtc, N, H // 2, W // 2, cin_s, _n.stream())
                dxs = dsum
            dx = nhwc_to_logical(dxs, cin)
            if dx.dtype != xdt:
                dx = dx.to(xdt)
        ng = ctx.needs_input_grad
        return dx, dw, dg if ng[2] else None, db if ng[3] else None, None


_UP_ZEROS = {}


def _up_zeros(N, H, W, cs, dtype, device):
    """the shared all-zero [N, H, W, cs] tensor an UpLink sends through autograd in place of the gradient sums it hands over"""
    key = (N, H, W, cs, dtype, device.type, device.index)
    t = _UP_ZEROS.get(key)
    if t is None:
        t = _UP_ZEROS[key] = torch.zeros(N, H, W, cs, dtype=dtype, device=device)
    return t


def conv_bn_relu(x, w, gamma, beta, cfg: BlockCfg):
    return _ConvBNReLUFn.apply(x, w, gamma, beta, cfg)


def _class_map_storage(t: torch.Tensor):
    """logical [N,K,H,W] f32 -> contiguous [N,H,W,K] storage (zero-copy for the channels-last views these ops return)."""
    assert t.dim() == 4
    if t.dtype != torch.float32:
        t = t.float()
    s = t.permute(0, 2, 3, 1)
    return s if s.is_contiguous() else s.contiguous()


class _Conv1x1Fn(torch.autograd.Function):
    """nn.Conv2d(C, K, 1) with bias (``_Deconv_1x1``, unet.py:147,229) -> f32 class map, logical [N,K,H,W]."""

    @staticmethod
    def forward(ctx, x, w, b, dtype):
        _n.require_gpu(x, w, b)
        N, C, H, W = x.shape
        K = w.shape[0]
        if K > 16 or C > 256:
            raise NotImplementedError("conv1x1 head: at most 16 classes / 256 input channels")
        xs = to_nhwc_padded(x.detach(), dtype)
        cs = xs.shape[3]
        wc, bc = w.detach().reshape(K, C).contiguous().float(), b.detach().contiguous().float()
        out = torch.empty(N, H, W, K, dtype=torch.float32, device=x.device)
        _n.call("spcl_conv1x1_forward", _n.ptr(xs), _n.dtype_code(dtype), N * H * W, C, cs, K, _n.ptr(wc), _n.ptr(bc),
                _n.ptr(out), _n.stream())
        ctx.save_for_backward(xs, wc)
        ctx.params = (w, b)
        ctx.meta = (N, C, H, W, K, cs, dtype, x.dtype, tuple(w.shape))
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dout):
        xs, wc = ctx.saved_tensors
        N, C, H, W, K, cs, dtype, xdt, wshape = ctx.meta
        do = _class_map_storage(dout)
        dev = do.device
        dxs = torch.empty(N, H, W, cs, dtype=dtype, device=dev)
        sinks = (take_grad_sink(ctx.params[0], ctx.needs_input_grad[1]),
                 take_grad_sink(ctx.params[1], ctx.needs_input_grad[2]))
        dw = _grad_buffer(sinks[0], (K, C), dev)
        db = _grad_buffer(sinks[1], (K,), dev)
        ws = torch.empty(_n.call("spcl_conv1x1_bwd_workspace_bytes", C, K) // 4, dtype=torch.float32, device=dev)
        _n.call("spcl_conv1x1_backward", _n.ptr(xs), _n.ptr(do), _n.dtype_code(dtype), N * H * W, C, cs, K, _n.ptr(wc),
                _n.ptr(dxs), _n.ptr(dw), _n.ptr(db), _n.ptr(ws), _n.stream())
        dx = nhwc_to_logical(dxs, C)
        if dx.dtype != xdt:
            dx = dx.to(xdt)
        return dx, dw.reshape(wshape), db, None


def conv1x1(x, w, b, dtype):
    return _Conv1x1Fn.apply(x, w, b, dtype)


class _Conv1x1BnFn(torch.autograd.Function):
    """``_Deconv_1x1(relu(bn(y)))`` for the block that returned its RAW second-conv output ``y`` (``BlockCfg.lazy_act``,
    ``link``: its ``ActLink``): BN + ReLU in the loader of the 1x1 convolution (spcl_conv1x1_forward_bn); the backward
    returns the gradient w.r.t. the ACTIVATION -- what the block's backward expects -- and leaves the BatchNorm-backward
    partial sums in the link (spcl_conv1x1_backward_bn)."""

    @staticmethod
    def forward(ctx, y, w, b, link: ActLink):
        _n.require_gpu(y, w, b)
        N, C, H, W = y.shape
        K = w.shape[0]
        if K > 16 or C > 256:
            raise NotImplementedError("conv1x1 head: at most 16 classes / 256 input channels")
        ys = link.yb
        assert (N, H, W, C) == (link.N, link.H, link.W, link.C) and ys.data_ptr() == y.data_ptr(), "not the linked block's output"
        cs, dtype = link.cs, ys.dtype
        wc, bc = w.detach().reshape(K, C).contiguous().float(), b.detach().contiguous().float()
        out = torch.empty(N, H, W, K, dtype=torch.float32, device=y.device)
        _n.call("spcl_conv1x1_forward_bn", _n.ptr(ys), _n.dtype_code(dtype), N * H * W, C, cs, K, _n.ptr(link.stb[2]),
                _n.ptr(link.stb[3]), _n.ptr(wc), _n.ptr(bc), _n.ptr(out), _n.stream())
        ctx.save_for_backward(wc)
        ctx.link = link
        ctx.params = (w, b)
        ctx.meta = (N, C, H, W, K, cs, dtype, y.dtype, tuple(w.shape))
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dout):
        (wc,) = ctx.saved_tensors
        link = ctx.link
        N, C, H, W, K, cs, dtype, ydt, wshape = ctx.meta
        do = _class_map_storage(dout)
        dev = do.device
        dact = torch.empty(N, H, W, cs, dtype=dtype, device=dev)
        sinks = (take_grad_sink(ctx.params[0], ctx.needs_input_grad[1]),
                 take_grad_sink(ctx.params[1], ctx.needs_input_grad[2]))
        dw = _grad_buffer(sinks[0], (K, C), dev)
        db = _grad_buffer(sinks[1], (K,), dev)
        ws = torch.empty(_n.call("spcl_conv1x1_bwd_workspace_bytes", C, K) // 4, dtype=torch.float32, device=dev)
        nrows = _n.call("spcl_conv1x1_bwd_rows", N * H * W)
        rows = torch.empty(nrows * 2 * cs, dtype=torch.float32, device=dev)
        rows.ntiles = nrows
        st = link.stb
        _n.call("spcl_conv1x1_backward_bn", _n.ptr(link.yb), _n.ptr(do), _n.dtype_code(dtype), N * H * W, C, cs, K,
                _n.ptr(st[2]), _n.ptr(st[3]), _n.ptr(st[0]), _n.ptr(wc), _n.ptr(dact), _n.ptr(dw), _n.ptr(db), _n.ptr(ws),
                _n.ptr(rows), _n.stream())
        link.rows, link.dx_ptr, link.holder, link.version = rows, dact.data_ptr(), dact, dact._version
        dx = nhwc_to_logical(dact, C)
        if dx.dtype != ydt:
            dx = dx.to(ydt)
        return dx, dw.reshape(wshape), db, None


def conv1x1_bn(y, w, b, link: ActLink):
    return _Conv1x1BnFn.apply(y, w, b, link)


class _SoftmaxFn(torch.autograd.Function):
    """``logits.softmax(1)`` on a logical [N,K,H,W] class map (new_epocher.py:86,271)."""

    @staticmethod
    def forward(ctx, logits):
        _n.require_gpu(logits)
        ls = _class_map_storage(logits.detach())
        N, H, W, K = ls.shape
        prob = torch.empty_like(ls)
        _n.call("spcl_softmax_forward", _n.ptr(ls), N * H * W, K, _n.ptr(prob), _n.stream())
        ctx.save_for_backward(prob)
        return prob.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dprob):
        (prob,) = ctx.saved_tensors
        N, H, W, K = prob.shape
        dp = _class_map_storage(dprob)
        dl = torch.empty_like(prob)
        _n.call("spcl_softmax_backward", _n.ptr(prob), _n.ptr(dp), N * H * W, K, _n.ptr(dl), _n.stream())
        return dl.permute(0, 3, 1, 2)


def softmax_classes(logits):
    return _SoftmaxFn.apply(logits)


class _KLDivFn(torch.autograd.Function):
    """deepclustering2.loss.KL_div(reduction='mean')(prob, target): mean over positions of
    sum_c -target log((prob+eps)/(target+eps)); gradient w.r.t. ``prob`` only (as the reference uses it)."""

    @staticmethod
    def forward(ctx, prob, target, eps):
        _n.require_gpu(prob, target)
        ps, ts = _class_map_storage(prob.detach()), _class_map_storage(target.detach())
        N, H, W, K = ps.shape
        dev = ps.device
        ws = torch.empty(_n.call("spcl_kl_workspace_bytes") // 4, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _n.call("spcl_kl_div_forward", _n.ptr(ps), _n.ptr(ts), N * H * W, K, c_float(eps), _n.ptr(ws), _n.ptr(loss),
                _n.stream())
        ctx.save_for_backward(ps, ts)
        ctx.eps = eps
        return loss

    @staticmethod
    def backward(ctx, g):
        ps, ts = ctx.saved_tensors
        N, H, W, K = ps.shape
        gs = g.detach().reshape(1).float().contiguous()
        dp = torch.empty_like(ps)
        _n.call("spcl_kl_div_backward", _n.ptr(ps), _n.ptr(ts), N * H * W, K, c_float(ctx.eps), _n.ptr(gs), _n.ptr(dp),
                _n.stream())
        return dp.permute(0, 3, 1, 2), None, None


def kl_div(prob, target, eps=1e-16):
    return _KLDivFn.apply(prob, target, eps)


class _SupLossFn(torch.autograd.Function):
    """``KL_div(logits.softmax(1), class2one_hot(target, C))`` + the Dice counts of ``logits.max(1)[1]`` against ``target``
    (semi_seg/epochers/new_epocher.py:268-282) in ONE launch over the class map; the gradient w.r.t. the logits for a unit
    upstream gradient is written by the same launch and scaled in backward.  ``counts`` receives (inter, union) [B, C]."""

    @staticmethod
    def forward(ctx, logits, labels, eps, counts):
        _n.require_gpu(logits, labels)
        ls = _class_map_storage(logits.detach())
        N, H, W, K = ls.shape
        lab = labels.detach().long().contiguous()
        if tuple(lab.shape) != (N, H, W):
            raise AssertionError(f"labels {tuple(lab.shape)} do not match the class map {(N, H, W)}")
        dev = ls.device
        ws = torch.empty(_n.call("spcl_kl_workspace_bytes") // 4, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        dl = torch.empty_like(ls)
        both = torch.empty(2, N, K, dtype=torch.int64, device=dev)  # (written by the launch; a caller that keeps them clones ``inter._base`` once)
        inter, union = both[0], both[1]
        _n.call("spcl_sup_loss_forward", _n.ptr(ls), _n.ptr(lab), N, H * W, K, c_float(eps), _n.ptr(ws), _n.ptr(loss),
                _n.ptr(dl), _n.ptr(inter), _n.ptr(union), _n.stream())
        counts.append((inter, union))
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        if is_unit_gradient(g):  # the epocher's own ``backward(gradient=ones)``: x * 1.0 is x, the pass over the class map is skipped
            return dl.permute(0, 3, 1, 2), None, None, None
        return (dl * g.detach().float()).permute(0, 3, 1, 2), None, None, None


_UNIT_GRADIENTS = {}  # data_ptr -> weakref of a 0-dim tensor its owner promises to keep at exactly 1.0


def register_unit_gradient(t: torch.Tensor):
    """``t`` (0-dim, value 1.0, never written again by its owner) is what ``loss.backward(gradient=t)`` will be called with:
    a backward that recognises it by its storage skips the multiplication by it.  Held weakly."""
    import weakref
    assert t.numel() == 1
    _UNIT_GRADIENTS[t.data_ptr()] = (weakref.ref(t), t._version)
    return t


def is_unit_gradient(g: torch.Tensor) -> bool:
    ent = _UNIT_GRADIENTS.get(g.data_ptr()) if g.numel() == 1 else None
    if ent is None:
        return False
    ref, version = ent
    t = ref()
    if t is None or t.data_ptr() != g.data_ptr() or t.dtype != g.dtype:
        _UNIT_GRADIENTS.pop(g.data_ptr(), None)  # (the registered tensor is gone: its address may belong to anything now)
        return False
    if t._version != version:
        # written in place since it was registered (a caller scaling the loss through it): no longer known to hold 1.0 -- the
        # promise is broken for good, the backward multiplies by whatever it holds now
        _UNIT_GRADIENTS.pop(g.data_ptr(), None)
        return False
    return True


def sup_loss_kl_onehot(logits, labels, eps=1e-16):
    """-> (loss, (inter, union)): the fine-tune criterion and the training batch's Dice counts, fused (``_SupLossFn``)"""
    counts = []
    loss = _SupLossFn.apply(logits, labels, eps, counts)
    return loss, counts[0]


_SUP_DICE_WS = {}  # (device, stream, N, C, H, W) -> workspace; the calls of one stream on one shape reuse it, in order


class _SupDiceFn(torch.autograd.Function):
    """``dice_weight * soft-Dice + kl_weight * class-weighted KL`` on one-hot targets (csrc/sup_dice.hip,
    contrastyou/losses/dice.py) + the Dice counts of the arg-max map.  Forward is ONE streaming pass (the sums of every group
    and class, reduced in a fixed order); the gradient needs those sums, so it is a second pass, launched by ``backward`` --
    under ``no_grad`` it never runs and nothing is kept.  ``cfg`` = (dice_weight, kl_weight, include_background, per_sample,
    smooth, eps); ``out`` receives ((inter, union) [N, C] int64, parts [2] = (L_kl, L_dice))."""

    @staticmethod
    def forward(ctx, logits, labels, weight, cfg, out):
        _n.require_gpu(logits, labels, weight)
        ls = _class_map_storage(logits.detach())
        N, H, W, C = ls.shape
        lab = labels.detach().long().contiguous()
        if tuple(lab.shape) != (N, H, W):
            raise AssertionError(f"labels {tuple(lab.shape)} do not match the class map {(N, H, W)}")
        dice_weight, kl_weight, include_background, per_sample, smooth, eps = cfg
        dev = ls.device
        key = (dev, torch.cuda.current_stream(dev).cuda_stream, N, C, H, W)
        ws = _SUP_DICE_WS.get(key)
        if ws is None:  # zeroed once: a call leaves the ticket in its first bytes at zero
            ws = _SUP_DICE_WS[key] = torch.zeros(max(_n.call("spcl_sup_dice_workspace_bytes", N, C, H, W), 64),
                                                 dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        parts = torch.empty(2, dtype=torch.float32, device=dev)  # L_kl, L_dice
        both = torch.empty(2, N, C, dtype=torch.int64, device=dev)
        coef = torch.empty(N if per_sample else 1, C, 2, dtype=torch.float32, device=dev)
        _n.call("spcl_sup_dice_forward", _n.ptr(ls), _n.ptr(lab), _n.ptr(weight), N, C, H, W, c_float(dice_weight),
                c_float(kl_weight), int(bool(include_background)), int(bool(per_sample)), c_float(smooth), c_float(eps),
                _n.ptr(loss), _n.ptr(parts), _n.ptr(both[0]), _n.ptr(both[1]), _n.ptr(coef), _n.ptr(ws), ws.numel(),
                _n.stream())
        out.append(((both[0], both[1]), parts))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(ls, lab, weight, coef)
            ctx.cfg = cfg
        return loss

    @staticmethod
    def backward(ctx, g):
        ls, lab, weight, coef = ctx.saved_tensors
        N, H, W, C = ls.shape
        dice_weight, kl_weight, _, per_sample, _, eps = ctx.cfg
        gs = None if is_unit_gradient(g) else g.detach().reshape(1).float().contiguous()  # (scaled inside the one pass)
        dl = torch.empty_like(ls)
        _n.call("spcl_sup_dice_backward", _n.ptr(ls), _n.ptr(lab), _n.ptr(weight), _n.ptr(coef), N, C, H, W,
                c_float(dice_weight), c_float(kl_weight), int(bool(per_sample)), c_float(eps), _n.ptr(gs), _n.ptr(dl),
                _n.stream())
        return dl.permute(0, 3, 1, 2), None, None, None, None


def sup_dice_kl_onehot(logits, labels, weight, *, dice_weight=1.0, kl_weight=1.0, include_background=True, per_sample=False,
                       smooth=1e-5, eps=1e-16):
    """-> (loss, (inter, union), parts): soft-Dice + class-weighted KL of [N,C,H,W] logits against an [N,H,W] label map
    (``_SupDiceFn``); ``weight`` is a float32 device vector of C class weights, ``parts`` a device [2] tensor (L_kl, L_dice)"""
    out = []
    cfg = (float(dice_weight), float(kl_weight), bool(include_background), bool(per_sample), float(smooth), float(eps))
    loss = _SupDiceFn.apply(logits, labels, weight, cfg, out)
    counts, parts = out[0]
    return loss, counts, parts


_SDM_WS, _BOUNDARY_WS = {}, {}  # (device, stream, shape) -> workspace, as _SUP_DICE_WS


def _class_list(classes, what):
    cl = tuple(int(c) for c in classes)
    if not cl or len(cl) > 16 or len(set(cl)) != len(cl) or min(cl) < 0:
        raise ValueError(f"{what}: 1 to 16 distinct non-negative classes, given {cl}")
    return cl


def signed_distance_maps(labels: torch.Tensor, classes) -> torch.Tensor:
    """[N,H,W] integer labels -> logical [N, |classes|, H, W] f32 (channels-last storage) signed Euclidean distance maps
    (csrc/boundary.hip, INTEGRATION.md "Boundary loss"): +sqrt(d2) outside ``labels == c``, -(sqrt(d2) - 1) inside, 0 on a
    slice where the class is absent or fills it; unit pixel spacing.  Two launches, nothing read back, no gradient."""
    cl = _class_list(classes, "signed_distance_maps")
    _n.require_gpu(labels)
    if labels.dim() != 3:
        raise ValueError(f"labels [N,H,W], given {tuple(labels.shape)}")
    lab = labels.detach().long().contiguous()
    N, H, W = lab.shape
    if N > 1024 or H > 1024 or W > 1024 or min(N, H, W) < 1:
        raise ValueError(f"signed_distance_maps: 1 <= N, H, W <= 1024, given {(N, H, W)}")
    S, dev = len(cl), lab.device
    key = (dev, torch.cuda.current_stream(dev).cuda_stream, N, H, W, S)
    ws = _SDM_WS.get(key)
    if ws is None:
        ws = _SDM_WS[key] = torch.empty(_n.call("spcl_signed_distance_workspace_bytes", N, H, W, S), dtype=torch.uint8,
                                        device=dev)
    phi = torch.empty(N, H, W, S, dtype=torch.float32, device=dev)
    _n.call("spcl_signed_distance_maps", _n.ptr(lab), N, H, W, (ctypes.c_int * S)(*cl), S, _n.ptr(phi), _n.ptr(ws),
            ws.numel(), _n.stream())
    return phi.permute(0, 3, 1, 2)


class _BoundaryFn(torch.autograd.Function):
    """``alpha * L_B``, L_B = mean over (n, listed class, pixel) of softmax(logits) * phi (csrc/boundary.hip); ``alpha`` is a
    device scalar read by the kernels, so a captured call replays with what it holds then.  ``out`` receives L_B itself."""

    @staticmethod
    def forward(ctx, logits, phi, classes, alpha, out):
        _n.require_gpu(logits, phi, alpha)
        ls = _class_map_storage(logits.detach())
        ps = _class_map_storage(phi.detach())
        N, H, W, C = ls.shape
        S = len(classes)
        if tuple(ps.shape) != (N, H, W, S):
            raise AssertionError(f"distance maps {tuple(ps.shape)} do not match {(N, H, W, S)}")
        if alpha.dtype != torch.float32 or alpha.numel() != 1:
            raise AssertionError("alpha must be a float32 device scalar")
        dev = ls.device
        key = (dev, torch.cuda.current_stream(dev).cuda_stream, N, H, W)
        ws = _BOUNDARY_WS.get(key)
        if ws is None:
            ws = _BOUNDARY_WS[key] = torch.empty(max(_n.call("spcl_boundary_workspace_bytes", N, H, W), 8),
                                                 dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)  # alpha * L_B
        mean = torch.empty((), dtype=torch.float32, device=dev)  # L_B
        cl = (ctypes.c_int * S)(*classes)
        _n.call("spcl_boundary_forward", _n.ptr(ls), _n.ptr(ps), cl, S, N, C, H, W, _n.ptr(alpha), _n.ptr(loss),
                _n.ptr(mean), _n.ptr(ws), ws.numel(), _n.stream())
        out.append(mean)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(ls, ps, alpha)
            ctx.classes = classes
        return loss

    @staticmethod
    def backward(ctx, g):
        ls, ps, alpha = ctx.saved_tensors
        N, H, W, C = ls.shape
        S = len(ctx.classes)
        gs = None if is_unit_gradient(g) else g.detach().reshape(1).float().contiguous()
        dl = torch.empty_like(ls)
        _n.call("spcl_boundary_backward", _n.ptr(ls), _n.ptr(ps), (ctypes.c_int * S)(*ctx.classes), S, N, C, H, W,
                _n.ptr(alpha), _n.ptr(gs), _n.ptr(dl), _n.stream())
        return dl.permute(0, 3, 1, 2), None, None, None, None


def boundary_loss(logits, phi, classes, alpha, *, with_mean=False):
    """``alpha * L_B`` of [N,C,H,W] logits against the signed distance maps ``phi`` [N,|classes|,H,W] of ``classes`` (distinct,
    in [0, C)); ``alpha`` a float32 device scalar (``_BoundaryFn``).  ``with_mean=True`` -> (loss, L_B), L_B a device scalar
    without a gradient."""
    cl = _class_list(classes, "boundary_loss")
    _n.require_gpu(logits, phi, alpha)
    if logits.dim() != 4 or max(cl) >= logits.shape[1]:
        raise ValueError(f"boundary_loss: logits [N,C,H,W] and classes in [0, C), given {tuple(logits.shape)} and {cl}")
    out = []
    loss = _BoundaryFn.apply(logits, phi, cl, alpha, out)
    return (loss, out[0]) if with_mean else loss


def one_hot_classes(labels: torch.Tensor, K: int) -> torch.Tensor:
    """class2one_hot: [N,H,W] integer labels -> logical [N,K,H,W] f32 one-hot (NHWC storage)."""
    _n.require_gpu(labels)
    lab = labels.detach().long().contiguous()
    N, H, W = lab.shape
    out = torch.empty(N, H, W, K, dtype=torch.float32, device=lab.device)
    _n.call("spcl_one_hot", _n.ptr(lab), N * H * W, K, _n.ptr(out), _n.stream())
    return out.permute(0, 3, 1, 2)


def argmax_classes(logits: torch.Tensor) -> torch.Tensor:
    """``logits.max(1)[1]`` -> [N,H,W] int64 (first maximum)."""
    _n.require_gpu(logits)
    ls = _class_map_storage(logits.detach())
    N, H, W, K = ls.shape
    out = torch.empty(N, H, W, dtype=torch.int64, device=ls.device)
    _n.call("spcl_argmax_classes", _n.ptr(ls), N * H * W, K, _n.ptr(out), _n.stream())
    return out


def dice_counts(pred: torch.Tensor, target: torch.Tensor, C: int):
    """per sample and class: intersection and union counts of two class-coded maps -> two [B,C] int64 tensors."""
    _n.require_gpu(pred, target)
    if pred.shape != target.shape:
        raise AssertionError(f"incompatible shape of `pred` and `target`, given {pred.shape} and {target.shape}.")
    p, t = pred.detach().long().contiguous(), target.detach().long().contiguous()
    B = p.shape[0]
    inter = torch.zeros(B, C, dtype=torch.int64, device=p.device)
    union = torch.zeros(B, C, dtype=torch.int64, device=p.device)
    _n.call("spcl_dice_counts", _n.ptr(p), _n.ptr(t), B, p[0].numel(), C, _n.ptr(inter), _n.ptr(union), _n.stream())
    return inter, union


_SURFACE_WS = {}  # (device, B, H, W, n_report) -> workspace; every call on that shape reuses it (calls are stream-ordered)


def surface_distances(pred: torch.Tensor, target: torch.Tensor, C: int, report_axis=None, voxelspacing=None,
                      percentile: float = 95.0):
    """Hausdorff, percentile Hausdorff and average surface distance per (sample, reported class) of two class-coded [B,H,W]
    maps (``spcl_surface_distances``) -> ``(hd, mhd, asd, empty)``: three float64 [B, n_report] tensors and a uint8 flag that
    is set where the class is missing from ``pred`` or ``target`` (the three values are NaN there).  ``voxelspacing``: None
    (1, 1), one float for both axes, or ``(sy, sx)``.  Everything stays on the device."""
    _n.require_gpu(pred, target)
    if pred.shape != target.shape:
        raise AssertionError(f"incompatible shape of `pred` and `target`, given {pred.shape} and {target.shape}.")
    if pred.dim() != 3 or pred.is_floating_point() or target.is_floating_point():
        raise TypeError(f"surface_distances takes class-coded integer [B,H,W] maps, given {tuple(pred.shape)} {pred.dtype}")
    report = list(range(C)) if report_axis is None else [int(c) for c in report_axis]
    if voxelspacing is None:
        sy = sx = 1.0
    elif isinstance(voxelspacing, (int, float)):
        sy = sx = float(voxelspacing)
    else:
        sy, sx = (float(v) for v in voxelspacing)
    p, t = pred.detach().long().contiguous(), target.detach().long().contiguous()
    B, H, W = p.shape
    R, dev = len(report), p.device
    key = (dev, B, H, W, R)
    ws = _SURFACE_WS.get(key)
    if ws is None:
        nbytes = _n.call("spcl_surface_workspace_bytes", B, H, W, R)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None  # (0: the call below says why)
        if ws is not None:
            _SURFACE_WS[key] = ws
    vals = torch.empty((3, B, R), dtype=torch.float64, device=dev)
    empty = torch.empty((B, R), dtype=torch.uint8, device=dev)
    _n.call("spcl_surface_distances", _n.ptr(p), _n.ptr(t), B, H, W, int(C), (c_int * max(R, 1))(*report), R, sy, sx,
            float(percentile), _n.ptr(vals[0]), _n.ptr(vals[1]), _n.ptr(vals[2]), _n.ptr(empty), _n.ptr(ws),
            ws.numel() if ws is not None else 0, _n.stream())
    return vals[0], vals[1], vals[2], empty


_SURFACE3D_WS = {}  # (device, V, D, H, W, n_report) -> workspace, reused as _SURFACE_WS is


def surface_distances_3d(pred: torch.Tensor, target: torch.Tensor, C: int, report_axis=None, voxelspacing=None,
                         percentile: float = 95.0):
    """``surface_distances`` per VOLUME (``spcl_surface_distances_3d``): class-coded integer ``[D,H,W]`` (one volume) or
    ``[V,D,H,W]`` maps, 6-neighbour borders, exact 3-D Euclidean distances -> ``(hd, mhd, asd, empty)``, float64 / uint8
    ``[V, n_report]``.  ``voxelspacing``: None (1, 1, 1), one float for the three axes, or ``(sz, sy, sx)``.  Everything
    stays on the device."""
    if pred.shape != target.shape:
        raise AssertionError(f"incompatible shape of `pred` and `target`, given {pred.shape} and {target.shape}.")
    if pred.dim() not in (3, 4) or pred.is_floating_point() or target.is_floating_point():
        raise TypeError("surface_distances_3d takes class-coded integer [D,H,W] or [V,D,H,W] maps, given "
                        f"{tuple(pred.shape)} {pred.dtype}")
    _n.require_gpu(pred, target)
    report = list(range(C)) if report_axis is None else [int(c) for c in report_axis]
    if voxelspacing is None:
        sz = sy = sx = 1.0
    elif isinstance(voxelspacing, (int, float)):
        sz = sy = sx = float(voxelspacing)
    else:
        sz, sy, sx = (float(v) for v in voxelspacing)
    p, t = pred.detach().long().contiguous(), target.detach().long().contiguous()
    if p.dim() == 3:
        p, t = p.unsqueeze(0), t.unsqueeze(0)
    V, D, H, W = p.shape
    R, dev = len(report), p.device
    key = (dev, V, D, H, W, R)
    ws = _SURFACE3D_WS.get(key)
    if ws is None:
        nbytes = _n.call("spcl_surface_3d_workspace_bytes", V, D, H, W, R)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None  # (0: the call below says why)
        if ws is not None:
            _SURFACE3D_WS[key] = ws
    vals = torch.empty((3, V, R), dtype=torch.float64, device=dev)
    empty = torch.empty((V, R), dtype=torch.uint8, device=dev)
    _n.call("spcl_surface_distances_3d", _n.ptr(p), _n.ptr(t), V, D, H, W, int(C), (c_int * max(R, 1))(*report), R, sz, sy, sx,
            float(percentile), _n.ptr(vals[0]), _n.ptr(vals[1]), _n.ptr(vals[2]), _n.ptr(empty), _n.ptr(ws),
            ws.numel() if ws is not None else 0, _n.stream())
    return vals[0], vals[1], vals[2], empty


_LCC_WS = {}  # (device, V, D, H, W, n_classes) -> workspace, reused as _SURFACE_WS is


def largest_components(labels: torch.Tensor, num_classes: int, classes=None, volumetric: bool = True, out=None):
    """Keep the largest connected component of every listed foreground class (``spcl_largest_component``): ``labels`` is a
    class-coded integer ``[D,H,W]`` or ``[V,D,H,W]`` map; with ``volumetric=False`` a ``[B,H,W]`` map is ``B`` independent
    slices (4-neighbour components; a 4-D map is refused there), with ``volumetric=True`` it is ONE volume (6-neighbour), as
    ``surface_distances_3d`` reads it.  -> the processed int64 map in the shape of ``labels``: every voxel of a listed class outside that class's
    largest component becomes 0 (equal sizes: the component that starts first in raster order, as ``scipy.ndimage.label`` +
    ``argmax(bincount)`` decide), everything else is copied.  ``classes``: None = ``range(1, num_classes)``, else distinct
    classes in ``[1, num_classes)``, at most 15.  A list passed as ``out`` receives ``(kept_size, n_components)``: int64 / int32
    ``[V, n_classes]`` device tensors (as ``ucmt_softmax_mse(out=)`` hands over its extras).  Everything stays on the device."""
    if labels.dim() not in (3, 4) or labels.is_floating_point() or labels.dtype == torch.bool:
        raise TypeError("largest_components takes class-coded integer [D,H,W] or [V,D,H,W] maps, given "
                        f"{tuple(labels.shape)} {labels.dtype}")
    _n.require_gpu(labels)
    C = int(num_classes)
    cls = list(range(1, C)) if classes is None else [int(c) for c in classes]
    if C < 2 or not 1 <= len(cls) <= 15 or any(not 1 <= c < C for c in cls) or len(set(cls)) != len(cls):
        raise ValueError(f"largest_components: `classes` must be 1 to 15 distinct classes in [1, {C}) (0 is the fill value), "
                         f"given {cls}")
    lab = labels.detach().long().contiguous()
    shape = lab.shape
    if lab.dim() == 3:
        lab = lab.unsqueeze(0) if volumetric else lab.unsqueeze(1)
    elif not volumetric:
        raise ValueError("largest_components(volumetric=False) takes [B,H,W] slices")
    V, D, H, W = lab.shape
    R, dev = len(cls), lab.device
    key = (dev, V, D, H, W, R)
    ws = _LCC_WS.get(key)
    if ws is None:
        nbytes = _n.call("spcl_largest_component_workspace_bytes", V, D, H, W, R)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None  # (0: the call below says why)
        if ws is not None:
            _LCC_WS[key] = ws
    processed = torch.empty_like(lab)
    kept = torch.empty((V, R), dtype=torch.int64, device=dev)
    ncomp = torch.empty((V, R), dtype=torch.int32, device=dev)
    _n.call("spcl_largest_component", _n.ptr(lab), V, D, H, W, C, (c_int * R)(*cls), R, _n.ptr(processed), _n.ptr(kept),
            _n.ptr(ncomp), _n.ptr(ws), ws.numel() if ws is not None else 0, _n.stream())
    if out is not None:
        out.extend((kept, ncomp))
    return processed.view(shape)


# ------------------------------------------------------------------------------- test-time augmentation (csrc/tta.hip)
# The op byte of a view: bit 0 its input was flipped along H, bit 1 along W, bit 2 its H and W axes were swapped AFTER the
# flips.  "flips" is the group of the two mirrors, "dihedral" the eight symmetries of the square.
TTA_MODES = {"flips": (0, 1, 2, 3), "dihedral": (0, 1, 2, 3, 4, 5, 6, 7)}
TTA_VIEW_COUNTS = (1, 2, 4, 8)  # the merge's pairwise tree is balanced
_TTA_WS = {}  # (device, N, H, W) -> workspace, reused as _SURFACE_WS is
_TTA_FLAGS = {}  # (device, N, flip bits) -> uint8 [N] flags of ``flip_batch``, every sample the same


def _tta_ops(mode, H, W):
    """the op bytes of ``mode`` for an H x W image; host only.  An unknown mode and "dihedral" on a non-square image raise
    ``ValueError``."""
    if mode not in TTA_MODES:
        raise ValueError(f"tta mode must be one of {tuple(TTA_MODES)}, given {mode!r}")
    ops = TTA_MODES[mode]
    if any(op & 4 for op in ops) and H != W:
        raise ValueError(f"tta mode {mode!r} swaps the image axes and needs a square image, given {H} x {W}")
    return ops


def _tta_view(image, op):
    """view ``op`` of an [N, 1, H, W] batch: flipped along H (bit 0) and W (bit 1) by ``flip_batch``, then its axes swapped
    (bit 2).  Op 0 is ``image`` itself, not a copy."""
    view = image
    if op & 3:
        _n.require_gpu(image)
        key = (image.device, image.shape[0], op & 3)
        flags = _TTA_FLAGS.get(key)
        if flags is None:
            flags = _TTA_FLAGS[key] = torch.full((image.shape[0],), op & 3, dtype=torch.uint8, device=image.device)
        view = flip_batch(view, flags)
    if op & 4:
        view = view.transpose(-1, -2).contiguous()
    return view


def tta_views(image, mode):
    """``[(view_image, op), ...]`` of an [N, 1, H, W] batch for ``mode`` = "flips" (ops 0 - 3) or "dihedral" (ops 0 - 7, square
    images only: ``ValueError`` on the host before any device work).  View 0 is ``image`` itself."""
    if image.dim() != 4:
        raise ValueError(f"tta_views takes an [N, C, H, W] batch, given {tuple(image.shape)}")
    return [(_tta_view(image, op), op) for op in _tta_ops(mode, image.shape[-2], image.shape[-1])]


def tta_merge(view_logits, ops, eps=1e-16, want_entropy=True):
    """Merge the class logits of V views (``spcl_tta_merge``, one launch): ``view_logits[j]`` is the logical [N, C, H, W] map
    the network returned for the view with op byte ``ops[j]``, in THAT view's frame.  -> ``(prob, pred, entropy,
    mean_entropy)`` in the original frame: the mean over the views of their softmax (a logical [N, C, H, W] view of
    channels-last storage; the V rows are added in a balanced pairwise tree, so V exact copies merge to the bits of one),
    its first maximal class (int64 [N, H, W]), its normalised entropy ``-sum p log(p + eps) / log(C)`` (f32 [N, H, W]; None
    without ``want_entropy``) and the mean of that entropy (an f32 device scalar).  Everything stays on the device."""
    maps, ops = list(view_logits), [int(op) for op in ops]
    if len(maps) not in TTA_VIEW_COUNTS:
        raise ValueError(f"tta_merge: {len(maps)} views (1, 2, 4 or 8)")
    if len(ops) != len(maps):
        raise ValueError(f"tta_merge: {len(maps)} views and {len(ops)} ops")
    if any(not 0 <= op < 8 for op in ops):
        raise ValueError(f"tta_merge: every op must be in [0, 8), given {ops}")
    if any(t.dim() != 4 or tuple(t.shape) != tuple(maps[0].shape) or t.device != maps[0].device for t in maps):
        raise ValueError(f"tta_merge: the views' maps differ: {[tuple(t.shape) for t in maps]}")
    _n.require_gpu(*maps)
    stores = [_class_map_storage(t.detach()) for t in maps]
    N, H, W, C = stores[0].shape
    dev = stores[0].device
    key = (dev, N, H, W)
    ws = _TTA_WS.get(key)
    if ws is None:
        ws = _TTA_WS[key] = torch.empty(_n.call("spcl_tta_merge_workspace_bytes", N, H, W), dtype=torch.uint8, device=dev)
    prob = torch.empty((N, H, W, C), dtype=torch.float32, device=dev)
    pred = torch.empty((N, H, W), dtype=torch.int64, device=dev)
    entropy = torch.empty((N, H, W), dtype=torch.float32, device=dev) if want_entropy else None
    mean_entropy = torch.empty((), dtype=torch.float32, device=dev)
    _n.call("spcl_tta_merge", _n.ptr_array(stores), (ctypes.c_uint8 * len(ops))(*ops), len(ops), N, C, H, W,
            c_float(float(eps)), _n.ptr(prob), _n.ptr(pred), _n.ptr(entropy), _n.ptr(mean_entropy), _n.ptr(ws), ws.numel(),
            _n.stream())
    return prob.permute(0, 3, 1, 2), pred, entropy, mean_entropy


# ------------------------------------------------------------------------- pre-training monitor (csrc/embed_monitor.hip)
EMBED_MONITOR_MAX_N, EMBED_MONITOR_MAX_D, EMBED_MONITOR_MAX_K, EMBED_MONITOR_MAX_KINDS = 8192, 512, 32, 4
EMBED_MONITOR_MAX_LABEL = 65535
_EMON_WS = {}  # (device, N, d, k) -> workspace, kept and reused as _SURFACE_WS is (33 MB at the largest shape)

EmbeddingMonitorResult = collections.namedtuple(
    "EmbeddingMonitorResult", ["knn_idx", "knn_sim", "pred", "correct", "pair_rank", "scalars"])


def embedding_monitor(z, labels=None, pair=None, k=20, exclude_pair=True, check_labels=False, *, group=None):
    """Neighbour statistics of N embeddings in one sweep over their similarity matrix (``spcl_embed_monitor``, four launches,
    no [N, N] matrix).  ``z`` [N, d] f32 (2 <= N <= 8192, 1 <= d <= 512; rows of any length, normalised as ``F.normalize``);
    ``labels`` None, an integer [N] vector or [L, N] matrix (or a sequence of [N] vectors) of up to 4 label kinds with values
    in [0, 65535]; ``pair`` None or an integer [N] vector: the index of the row's other view, or -1; 1 <= ``k`` <= 32.  The
    candidates of row i are all j != i, with ``exclude_pair`` also j != pair[i]; a larger similarity wins, an equal one goes to
    the lower index.  -> ``EmbeddingMonitorResult`` of device tensors:

    ``knn_idx`` int32 / ``knn_sim`` f32 [N, k] (rank order; -1 / -inf where a row has fewer candidates), ``pred`` int32 [L, N]
    (the majority label of the neighbours, equal counts to the label whose best-ranked neighbour comes first, -1 without a
    neighbour), ``correct`` int32 [L], ``pair_rank`` int32 [N] (how many j outside {i, pair[i]} beat the pair; -1 without a
    pair) and ``scalars`` f64 [4]: alignment (NaN without a paired row), uniformity, the number of paired rows, the smallest
    row norm.  Bad arguments raise ``ValueError`` on the host before any device work.  The label range is the interface's
    contract only -- the kernel compares labels, it never indexes with them --, so it is checked (one read-back) only with
    ``check_labels=True``.  Nothing else is read back and the call can be captured, but the FIRST call at a shape
    (device, N, d, k) allocates that shape's workspace, which is kept for every later call: make it outside a capture, or
    the buffer comes from the graph's private pool.

    ``group`` (keyword only) None or an integer [N] vector on z's device: with ``group[i] >= 0`` the candidates of row i also
    leave out every j with ``group[j] == group[i]`` (``spcl_embed_monitor_grouped``; a negative id: ungrouped, nothing more is
    left out).  Groups enter ``knn_idx`` / ``knn_sim`` / ``pred`` / ``correct`` only.  ``group=None`` is the call it always was."""
    if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.dtype != torch.float32:
        raise ValueError("embedding_monitor takes an [N, d] float32 tensor, given "
                         f"{tuple(z.shape) if isinstance(z, torch.Tensor) else type(z).__name__} {getattr(z, 'dtype', '')}")
    N, d = z.shape
    if not 2 <= N <= EMBED_MONITOR_MAX_N or not 1 <= d <= EMBED_MONITOR_MAX_D:
        raise ValueError(f"embedding_monitor: N = {N} (2 .. {EMBED_MONITOR_MAX_N}), d = {d} (1 .. {EMBED_MONITOR_MAX_D})")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= EMBED_MONITOR_MAX_K:
        raise ValueError(f"embedding_monitor: k must be an integer in [1, {EMBED_MONITOR_MAX_K}], given {k!r}")
    if labels is not None and not isinstance(labels, torch.Tensor):
        labels = list(labels)
        if any(not isinstance(t, torch.Tensor) or t.dim() != 1 for t in labels):
            raise ValueError("embedding_monitor: a sequence of labels must hold [N] tensors")
        labels = torch.stack(labels) if labels else None
    if labels is not None:
        if labels.is_floating_point() or labels.dtype == torch.bool or labels.dim() not in (1, 2):
            raise ValueError(f"embedding_monitor: labels must be an integer [N] or [L, N] tensor, given {tuple(labels.shape)} "
                             f"{labels.dtype}")
        labels = labels.view(1, -1) if labels.dim() == 1 else labels
        if labels.shape[1] != N or labels.shape[0] > EMBED_MONITOR_MAX_KINDS or labels.device != z.device:
            raise ValueError(f"embedding_monitor: labels of shape {tuple(labels.shape)} on {labels.device} for {N} rows on "
                             f"{z.device} (at most {EMBED_MONITOR_MAX_KINDS} kinds)")
        if labels.shape[0] == 0:
            labels = None
    if labels is not None and check_labels:
        lo, hi = int(labels.min()), int(labels.max())
        if lo < 0 or hi > EMBED_MONITOR_MAX_LABEL:
            raise ValueError(f"embedding_monitor: labels must lie in [0, {EMBED_MONITOR_MAX_LABEL}], given [{lo}, {hi}]")
    if pair is not None:
        if not isinstance(pair, torch.Tensor) or pair.is_floating_point() or pair.dtype == torch.bool or \
                tuple(pair.shape) != (N,) or pair.device != z.device:
            raise ValueError(f"embedding_monitor: pair must be an integer [{N}] tensor on {z.device}")
    if group is not None:
        if not isinstance(group, torch.Tensor) or group.is_floating_point() or group.dtype == torch.bool or \
                tuple(group.shape) != (N,) or group.device != z.device:
            raise ValueError(f"embedding_monitor: group must be an integer [{N}] tensor on {z.device}")
    _n.require_gpu(z)
    z = z.detach()
    if z.stride(1) != 1 or z.stride(0) < d:
        z = z.contiguous()
    L = 0 if labels is None else labels.shape[0]
    lab = None if labels is None else labels.detach().to(torch.int32).contiguous()
    pr = None if pair is None else pair.detach().to(torch.int32).contiguous()
    dev = z.device
    key = (dev, N, d, k)
    ws = _EMON_WS.get(key)
    if ws is None:
        nbytes = _n.call("spcl_embed_monitor_workspace_bytes", N, d, k)
        ws = _EMON_WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    knn_idx = torch.empty((N, k), dtype=torch.int32, device=dev)
    knn_sim = torch.empty((N, k), dtype=torch.float32, device=dev)
    pred = torch.empty((L, N), dtype=torch.int32, device=dev)
    correct = torch.empty((L,), dtype=torch.int32, device=dev)
    pair_rank = torch.empty((N,), dtype=torch.int32, device=dev)
    scalars = torch.empty((4,), dtype=torch.float64, device=dev)
    outs = (_n.ptr(knn_idx), _n.ptr(knn_sim), _n.ptr(pred) if L else None, _n.ptr(correct) if L else None,
            _n.ptr(pair_rank), _n.ptr(scalars), _n.ptr(ws), ws.numel(), _n.stream())
    if group is None:
        _n.call("spcl_embed_monitor", _n.ptr(z), z.stride(0), _n.ptr(lab), L, _n.ptr(pr), N, d, k, 1 if exclude_pair else 0,
                *outs)
    else:
        gr = group.detach().to(torch.int32).contiguous()
        _n.call("spcl_embed_monitor_grouped", _n.ptr(z), z.stride(0), _n.ptr(lab), L, _n.ptr(pr), _n.ptr(gr), N, d, k,
                1 if exclude_pair else 0, *outs)
    return EmbeddingMonitorResult(knn_idx, knn_sim, pred, correct, pair_rank, scalars)


CELL_MAJORITY_MAX_C = 16


def cell_majority(labels, C, size, purity=True):
    """The label of every cell of an adaptive pool (``spcl_cell_majority``, one launch, integer counts): ``labels`` [N, H, W]
    (or [N, 1, H, W]) uint8 class codes below ``C`` (2 .. 16), ``size`` = (sh, sw) with 1 <= sh <= H, 1 <= sw <= W.  Cell
    (u, v) is the window of ``nn.AdaptiveAvgPool2d(size)``.  -> (``cell_label`` int32 [N, sh, sw]: the class with the largest
    count, equal counts to the lower class, -1 for a window of values >= C only; ``purity`` f32 [N, sh, sw]: count / window
    size, or None with ``purity=False``).  Bad arguments raise ``ValueError`` on the host; nothing is read back."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8:
        raise ValueError("cell_majority takes uint8 label maps, given "
                         f"{getattr(labels, 'dtype', type(labels).__name__)}")
    if labels.dim() == 4 and labels.shape[1] == 1:
        labels = labels[:, 0]
    if labels.dim() != 3 or min(labels.shape) < 1:
        raise ValueError(f"cell_majority: label maps must be [N, H, W] or [N, 1, H, W], given {tuple(labels.shape)}")
    if isinstance(C, bool) or not isinstance(C, int) or not 2 <= C <= CELL_MAJORITY_MAX_C:
        raise ValueError(f"cell_majority: C must be an integer in [2, {CELL_MAJORITY_MAX_C}], given {C!r}")
    size = (size, size) if isinstance(size, int) and not isinstance(size, bool) else tuple(size)
    N, H, W = labels.shape
    if len(size) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in size) or \
            not 1 <= size[0] <= H or not 1 <= size[1] <= W:
        raise ValueError(f"cell_majority: grid {size} for maps of {H} x {W} (1 <= sh <= H, 1 <= sw <= W)")
    sh, sw = size
    _n.require_gpu(labels)
    labels = labels.detach().contiguous()
    cell = torch.empty((N, sh, sw), dtype=torch.int32, device=labels.device)
    pur = torch.empty((N, sh, sw), dtype=torch.float32, device=labels.device) if purity else None
    _n.call("spcl_cell_majority", _n.ptr(labels), N, H, W, C, sh, sw, _n.ptr(cell), _n.ptr(pur), _n.stream())
    return cell, pur


class _Upsample2xFn(torch.autograd.Function):
    """nn.Upsample(scale_factor=2) (nearest) of ``_UpConv`` on NHWC storage; backward = 2x2 sum."""

    @staticmethod
    def forward(ctx, x, dtype):
        _n.require_gpu(x)
        N, C, H, W = x.shape
        xs = to_nhwc_padded(x.detach(), dtype)
        cs = xs.shape[3]
        y = torch.empty(N, 2 * H, 2 * W, cs, dtype=dtype, device=x.device)
        _n.call("spcl_upsample2x_forward", _n.ptr(xs), _n.ptr(y), _n.dtype_code(dtype), N, H, W, cs, _n.stream())
        ctx.meta = (N, C, H, W, cs, dtype, x.dtype)
        return nhwc_to_logical(y, C)

    @staticmethod
    def backward(ctx, dy):
        N, C, H, W, cs, dtype, xdt = ctx.meta
        dys = to_nhwc_padded(dy, dtype)
        dx = torch.empty(N, H, W, cs, dtype=dtype, device=dy.device)
        _n.call("spcl_upsample2x_backward", _n.ptr(dys), _n.ptr(dx), _n.dtype_code(dtype), N, H, W, cs, _n.stream())
        out = nhwc_to_logical(dx, C)
        return (out if out.dtype == xdt else out.to(xdt)), None


def upsample2x(x, dtype):
    return _Upsample2xFn.apply(x, dtype)


class _Concat2Fn(torch.autograd.Function):
    """torch.cat((a, b), dim=1) of two logical-NCHW tensors with NHWC storage (channel counts multiples of 16);
    backward = one split launch into two contiguous gradients."""

    @staticmethod
    def forward(ctx, a, b, dtype):
        _n.require_gpu(a, b)
        N, CA, H, W = a.shape
        CB = b.shape[1]
        sa, sb = to_nhwc_padded(a.detach(), dtype), to_nhwc_padded(b.detach(), dtype)
        out = torch.empty(N, H, W, CA + CB, dtype=dtype, device=a.device)
        _n.call("spcl_concat2_channels", _n.ptr(sa), _n.ptr(sb), _n.ptr(out), out.element_size(), N * H * W, CA, CB,
                _n.stream())
        ctx.meta = (N, CA, CB, H, W, dtype, a.dtype, b.dtype)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        N, CA, CB, H, W, dtype, adt, bdt = ctx.meta
        gs = to_nhwc_padded(g, dtype)
        ga = torch.empty(N, H, W, CA, dtype=dtype, device=g.device)
        gb = torch.empty(N, H, W, CB, dtype=dtype, device=g.device)
        _n.call("spcl_split2_channels", _n.ptr(gs), _n.ptr(ga), _n.ptr(gb), gs.element_size(), N * H * W, CA, CB,
                _n.stream())
        ga, gb = ga.permute(0, 3, 1, 2), gb.permute(0, 3, 1, 2)
        return (ga if ga.dtype == adt else ga.to(adt)), (gb if gb.dtype == bdt else gb.to(bdt)), None


class _VirtualCatFn(torch.autograd.Function):
    """``torch.cat((a, b), dim=1)`` (semi_seg/arch/unet.py:194-224) when a and b ALREADY are the two channel halves of one
    dense NHWC buffer -- their producers wrote them there (``BlockCfg.act_dst``): no launch forward, no launch backward (the
    gradient's halves are handed on as channel-slice views, which the BatchNorm-backward kernels read in place)."""

    @staticmethod
    def forward(ctx, a, b, holder):
        buf = holder[0]
        ctx.ca = a.shape[1]
        return buf.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        return g[:, :ctx.ca], g[:, ctx.ca:], None


def cat_buffer(N, H, W, ca, cb, dtype, device):
    """a dense [N,H,W,ca+cb] buffer and its two channel-slice views (destinations for the producers of a concatenation)"""
    buf = torch.empty(N, H, W, ca + cb, dtype=dtype, device=device)
    return buf, buf[..., :ca], buf[..., ca:]


def virtual_cat(a, b, buf):
    """cat((a, b), 1) without a copy when a and b are the two halves of ``buf`` (see ``cat_buffer``); else the copying kernel"""
    ca, cb = a.shape[1], b.shape[1]
    es = buf.element_size()
    ok = (a.dtype == b.dtype == buf.dtype and a.stride(1) == 1 and b.stride(1) == 1
          and a.data_ptr() == buf.data_ptr() and b.data_ptr() == buf.data_ptr() + ca * es
          and a.stride(3) == ca + cb == b.stride(3) and tuple(a.shape[2:]) == tuple(buf.shape[1:3]) == tuple(b.shape[2:])
          and a.shape[0] == buf.shape[0] == b.shape[0] and buf.shape[3] == ca + cb)
    if not ok:
        return concat_channels(a, b, buf.dtype)
    return _VirtualCatFn.apply(a, b, [buf])


def concat_channels(a, b, dtype):
    """cat((a, b), 1); channel counts that are not multiples of 16 (tiny test networks) go through torch.cat."""
    if a.shape[1] % 16 or b.shape[1] % 16:
        return torch.cat((a, b), dim=1)
    return _Concat2Fn.apply(a, b, dtype)


# --------------------------------------------------------------------------------------------- IIC / consistency (csrc/iic.hip)
IIC_DENSE, IIC_GLOBAL = 1, 0


def _flip_flags_arg(flags, N, dev):
    """per-sample flip flags as the kernels read them: a uint8 [N] tensor on the logits' device (the kernels index it
    by sample), or None"""
    if flags is None:
        return None
    _n.require_gpu(flags)
    if flags.device != dev or flags.dtype != torch.uint8 or flags.dim() != 1 or flags.numel() != N:
        raise ValueError(f"flip flags must be a uint8 [{N}] tensor on {dev}: got {flags.dtype} {tuple(flags.shape)} on "
                         f"{flags.device}")
    return flags.detach().contiguous()


class _IICLossFn(torch.autograd.Function):
    """The IIC criterion of S subheads in three launches: the joint of the grouped softmaxes of two logit maps (X read through
    its per-sample flips), the loss with dJ (one launch for all subheads), and -- in backward -- d(logits) of both maps.
    ``lx`` / ``ly``: logical [N, S*K, H, W] f32 logits (channels-last storage, as ``pixelwise_mlp`` returns them).
    Returns the loss; ``out`` receives (J f32 [S,T,T,K,K], nan flag int32 [1])."""

    @staticmethod
    def forward(ctx, lx, ly, flags, S, K, pad, dense, scale, out):
        _n.require_gpu(lx, ly)
        xs, ys = _class_map_storage(lx.detach()), _class_map_storage(ly.detach())
        if xs.shape != ys.shape or xs.shape[3] != S * K:
            raise AssertionError(f"logit maps {tuple(xs.shape)} / {tuple(ys.shape)} do not hold {S} x {K} clusters")
        N, H, W, ld = xs.shape
        T, dev = 2 * pad + 1, xs.device
        fl = _flip_flags_arg(flags, N, dev)
        jacc = torch.empty(_n.call("spcl_iic_joint_workspace_bytes", S, K, pad) // 8, dtype=torch.int64, device=dev)
        _n.call("spcl_iic_joint_forward", _n.ptr(xs), _n.ptr(ys), ld, N, H, W, S, K, pad, _n.ptr(fl), _n.ptr(jacc), _n.stream())
        jf = torch.empty(S, T, T, K, K, dtype=torch.float32, device=dev)
        dj = torch.empty_like(jf)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        flag = torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.empty(_n.call("spcl_iic_loss_workspace_bytes", S, T), dtype=torch.uint8, device=dev)
        _n.call("spcl_iic_loss", _n.ptr(jacc), None, S, K, T, int(dense), c_float(scale), _n.ptr(jf), _n.ptr(loss), _n.ptr(dj),
                _n.ptr(flag), _n.ptr(ws), ws.numel(), _n.stream())
        out.extend([jf, flag])
        ctx.save_for_backward(xs, ys, dj, fl)
        ctx.meta = (S, K, pad)
        return loss

    @staticmethod
    def backward(ctx, g):
        xs, ys, dj, fl = ctx.saved_tensors
        S, K, pad = ctx.meta
        N, H, W, ld = xs.shape
        gs = None if is_unit_gradient(g) else g.detach().float().reshape(1).contiguous()
        dlx, dly = torch.empty_like(xs), torch.empty_like(ys)
        _n.call("spcl_iic_joint_backward", _n.ptr(xs), _n.ptr(ys), ld, N, H, W, S, K, pad, _n.ptr(fl), _n.ptr(dj), _n.ptr(gs),
                _n.ptr(dlx), _n.ptr(dly), _n.stream())
        return dlx.permute(0, 3, 1, 2), dly.permute(0, 3, 1, 2), None, None, None, None, None, None, None


def iic_loss(lx, ly, *, num_subheads, num_clusters, padding=0, dense=True, scale=1.0, flags=None, out=None):
    """``scale * sum_s criterion(softmax(flip(lx)_s), softmax(ly_s))`` (IIDSegmentationLoss(padding) when ``dense``, IIDLoss
    otherwise) of logical [N, S*K, H, W] logits; differentiable w.r.t. both maps.  ``out`` (a list) receives (J, nan flag)."""
    return _IICLossFn.apply(lx, ly, flags, int(num_subheads), int(num_clusters), int(padding), bool(dense), float(scale),
                            [] if out is None else out)


def iic_loss_from_joint(j, *, dense=True, scale=1.0):
    """-> (loss, dJ, nan flag) of an f32 joint [S, T, T, K, K] (spcl_iic_loss on a given J; a check tool for the criterion)"""
    _n.require_gpu(j)
    jc = j.detach().float().contiguous()
    S, T, _, K, _ = jc.shape
    loss = torch.empty((), dtype=torch.float32, device=jc.device)
    dj = torch.empty_like(jc)
    flag = torch.empty(1, dtype=torch.int32, device=jc.device)
    ws = torch.empty(_n.call("spcl_iic_loss_workspace_bytes", S, T), dtype=torch.uint8, device=jc.device)
    _n.call("spcl_iic_loss", None, _n.ptr(jc), S, K, T, int(dense), c_float(scale), None, _n.ptr(loss), _n.ptr(dj),
            _n.ptr(flag), _n.ptr(ws), ws.numel(), _n.stream())
    return loss, dj, flag


def pica_balance_constant(M: int, K: int) -> float:
    """the balance term of PUISegLoss (pica_loss.py:76-77) on the simplex: its ``mean(0)`` runs over the class axis of the
    permuted [K, N, H, W] map, so ``p`` holds ``M = N H W`` entries that all equal 1/K -> ``log M - (M / K) log K``"""
    return math.log(M) - (M / K) * math.log(K)


def _pica_global_launch(xs, ys, S, K, lamda, scale, gs):
    """-> (loss, ce, dlx, dly) of [N, 1, 1, S*K] logits rows (spcl_pica_global_loss; ``gs``: a device scalar or None)"""
    N, ld, dev = xs.shape[0], xs.shape[3], xs.device
    loss, ce = torch.empty((), dtype=torch.float32, device=dev), torch.empty((), dtype=torch.float32, device=dev)
    dlx, dly = torch.empty_like(xs), torch.empty_like(ys)
    ws = torch.empty(_n.call("spcl_pica_workspace_bytes", S), dtype=torch.uint8, device=dev)
    _n.call("spcl_pica_global_loss", _n.ptr(xs), _n.ptr(ys), ld, N, S, K, c_float(lamda), c_float(scale), _n.ptr(gs),
            _n.ptr(loss), _n.ptr(ce), _n.ptr(dlx), _n.ptr(dly), _n.ptr(ws), ws.numel(), _n.stream())
    return loss, ce, dlx, dly


class _PICALossFn(torch.autograd.Function):
    """The PICA criteria of S subheads on two logit maps, logical [N, S*K, H, W] f32 (channels-last storage).  Dense
    (PUISegLoss): ``_IICLossFn``'s three launches with spcl_pica_seg_loss as the middle one (X read through its per-sample
    flips).  Global (PUILoss; H = W = 1, no flips): one launch that leaves the loss and both gradients.
    Returns the loss; ``out`` receives (ce, J f32 [S,T,T,K,K] or None)."""

    @staticmethod
    def forward(ctx, lx, ly, flags, S, K, pad, dense, lamda, scale, out):
        _n.require_gpu(lx, ly)
        xs, ys = _class_map_storage(lx.detach()), _class_map_storage(ly.detach())
        if xs.shape != ys.shape or xs.shape[3] != S * K:
            raise AssertionError(f"logit maps {tuple(xs.shape)} / {tuple(ys.shape)} do not hold {S} x {K} clusters")
        N, H, W, ld = xs.shape
        dev = xs.device
        ctx.dense, ctx.meta = dense, (S, K, pad, lamda, scale)
        if not dense:
            if H != 1 or W != 1 or flags is not None or pad != 0:
                raise ValueError("pica_loss(dense=False): [N, S*K, 1, 1] logits, no flags, no padding")
            loss, ce, dlx, dly = _pica_global_launch(xs, ys, S, K, lamda, scale, None)
            out.extend([ce, None])
            ctx.save_for_backward(xs, ys, dlx, dly)
            return loss
        T = 2 * pad + 1
        fl = _flip_flags_arg(flags, N, dev)
        jacc = torch.empty(_n.call("spcl_iic_joint_workspace_bytes", S, K, pad) // 8, dtype=torch.int64, device=dev)
        _n.call("spcl_iic_joint_forward", _n.ptr(xs), _n.ptr(ys), ld, N, H, W, S, K, pad, _n.ptr(fl), _n.ptr(jacc), _n.stream())
        jf = torch.empty(S, T, T, K, K, dtype=torch.float32, device=dev)
        dj = torch.empty_like(jf)
        loss, ce = torch.empty((), dtype=torch.float32, device=dev), torch.empty((), dtype=torch.float32, device=dev)
        ws = torch.empty(_n.call("spcl_pica_workspace_bytes", S), dtype=torch.uint8, device=dev)
        _n.call("spcl_pica_seg_loss", _n.ptr(jacc), None, S, K, T, c_double(lamda * pica_balance_constant(N * H * W, K)),
                c_float(scale), _n.ptr(jf), _n.ptr(loss), _n.ptr(ce), _n.ptr(dj), _n.ptr(ws), ws.numel(), _n.stream())
        out.extend([ce, jf])
        ctx.save_for_backward(xs, ys, dj, fl)
        return loss

    @staticmethod
    def backward(ctx, g):
        S, K, pad, lamda, scale = ctx.meta
        gs = None if is_unit_gradient(g) else g.detach().float().reshape(1).contiguous()
        if ctx.dense:
            xs, ys, dj, fl = ctx.saved_tensors
            N, H, W, ld = xs.shape
            dlx, dly = torch.empty_like(xs), torch.empty_like(ys)
            _n.call("spcl_iic_joint_backward", _n.ptr(xs), _n.ptr(ys), ld, N, H, W, S, K, pad, _n.ptr(fl), _n.ptr(dj),
                    _n.ptr(gs), _n.ptr(dlx), _n.ptr(dly), _n.stream())
        else:
            xs, ys, dlx, dly = ctx.saved_tensors
            if gs is not None:  # (the saved gradients are for a unit upstream gradient: run the launch again with the scalar)
                _, _, dlx, dly = _pica_global_launch(xs, ys, S, K, lamda, scale, gs)
        return dlx.permute(0, 3, 1, 2), dly.permute(0, 3, 1, 2), None, None, None, None, None, None, None, None


def pica_loss(lx, ly, *, num_subheads, num_clusters, padding=0, dense=True, lamda=2.0, scale=1.0, flags=None, out=None):
    """``scale * sum_s criterion(softmax(flip(lx)_s), softmax(ly_s))`` (PUISegLoss(lamda, padding) when ``dense``, PUILoss(lamda)
    otherwise: pica_loss.py) of logical [N, S*K, H, W] logits; differentiable w.r.t. both maps.  The dense criterion's balance
    term is the constant ``pica_balance_constant`` (no gradient).  ``out`` (a list) receives (ce, J): ``ce`` the
    cross-entropy part of the returned loss, ``J`` the dense joint (None for the global criterion)."""
    return _PICALossFn.apply(lx, ly, flags, int(num_subheads), int(num_clusters), int(padding), bool(dense), float(lamda),
                             float(scale), [] if out is None else out)


def pica_seg_loss_from_joint(j, *, lamda=2.0, ne=0.0, scale=1.0):
    """-> (loss, ce, dJ) of an f32 joint [S, T, T, K, K] with the balance term ``ne`` given (spcl_pica_seg_loss on a given J; a
    check tool for the criterion)"""
    _n.require_gpu(j)
    jc = j.detach().float().contiguous()
    S, T, _, K, _ = jc.shape
    loss = torch.empty((), dtype=torch.float32, device=jc.device)
    ce = torch.empty((), dtype=torch.float32, device=jc.device)
    dj = torch.empty_like(jc)
    ws = torch.empty(_n.call("spcl_pica_workspace_bytes", S), dtype=torch.uint8, device=jc.device)
    _n.call("spcl_pica_seg_loss", None, _n.ptr(jc), S, K, T, c_double(float(lamda) * float(ne)), c_float(scale), None,
            _n.ptr(loss), _n.ptr(ce), _n.ptr(dj), _n.ptr(ws), ws.numel(), _n.stream())
    return loss, ce, dj


def iic_patch_starts(h: int, patch_size: int):
    """patch_generator's starts along an axis of length ``h`` (iic_loss.py:156-159): ``0, s, 2s, ... < h - patch_size`` and
    then ``max(h - patch_size, 0)``, ``s = patch_size // 2``.  The one place the lists are computed on the Python side; the
    library derives the same lists from (h, patch_size) and ``_IICPatchLossFn`` compares the counts."""
    h, patch_size = int(h), int(patch_size)
    if patch_size < 2:
        raise ValueError(f"patch_size = {patch_size}: at least 2 (the stride is patch_size // 2)")
    if h < 1:
        raise ValueError(f"axis length {h}")
    return list(range(0, h - patch_size, patch_size // 2)) + [max(h - patch_size, 0)]


class _IICPatchLossFn(torch.autograd.Function):
    """``scale * mean over patches of IIDSegmentationLoss(softmax(lx), softmax(flip(ly)))`` (IIDSegmentationSmallPathLoss) in
    two launches -- every patch's joint, then every patch's criterion with dJ -- and one more in backward, in which a pixel
    gathers from the patches that cover it.  ``lx`` / ``ly``: logical [N, C, H, W] f32 class logits.  Returns the loss;
    ``out`` receives (per-patch losses f32 [nP], nan flag int32 [1])."""

    @staticmethod
    def forward(ctx, lx, ly, flags, pad, patch, scale, out):
        _n.require_gpu(lx, ly)
        xs, ys = _class_map_storage(lx.detach()), _class_map_storage(ly.detach())
        if xs.shape != ys.shape:
            raise AssertionError(f"class maps {tuple(xs.shape)} / {tuple(ys.shape)} differ")
        N, H, W, C = xs.shape
        dev = xs.device
        n_patches, ws_bytes, dj_elems = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        _n.call("spcl_iic_patch_plan", N, C, H, W, pad, patch, ctypes.byref(n_patches), ctypes.byref(ws_bytes),
                ctypes.byref(dj_elems))
        nP = len(iic_patch_starts(H, patch)) * len(iic_patch_starts(W, patch))
        assert nP == n_patches.value, (nP, n_patches.value)
        fl = _flip_flags_arg(flags, N, dev)
        ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device=dev)
        dj = torch.empty(dj_elems.value, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        per_patch = torch.empty(nP, dtype=torch.float32, device=dev)
        flag = torch.empty(1, dtype=torch.int32, device=dev)
        _n.call("spcl_iic_patch_forward", _n.ptr(xs), _n.ptr(ys), N, C, H, W, pad, patch, _n.ptr(fl), c_float(scale),
                _n.ptr(loss), _n.ptr(per_patch), _n.ptr(flag), _n.ptr(dj), _n.ptr(ws), ws.numel(), _n.stream())
        out.extend([per_patch, flag])
        ctx.save_for_backward(xs, ys, dj, fl)
        ctx.meta = (pad, patch)
        return loss

    @staticmethod
    def backward(ctx, g):
        xs, ys, dj, fl = ctx.saved_tensors
        pad, patch = ctx.meta
        N, H, W, C = xs.shape
        gs = None if is_unit_gradient(g) else g.detach().float().reshape(1).contiguous()
        dlx = torch.empty_like(xs)
        dly = torch.empty_like(ys) if ctx.needs_input_grad[1] else None
        _n.call("spcl_iic_patch_backward", _n.ptr(xs), _n.ptr(ys), N, C, H, W, pad, patch, _n.ptr(fl), _n.ptr(dj), _n.ptr(gs),
                _n.ptr(dlx), _n.ptr(dly), _n.stream())
        return dlx.permute(0, 3, 1, 2), None if dly is None else dly.permute(0, 3, 1, 2), None, None, None, None, None


def iic_patch_loss(lx, ly, *, padding, patch_size, scale=1.0, flags=None, out=None):
    """``scale * IIDSegmentationSmallPathLoss(padding, patch_size)(softmax(lx), softmax(flip(ly)))`` of logical [N, C, H, W]
    logits (iic_loss.py:103-128); differentiable w.r.t. ``lx``, and w.r.t. ``ly`` when it requires grad.  ``flags`` flip Y.
    ``out`` (a list) receives (per-patch losses [nP], not scaled; nan flag int32 [1])."""
    return _IICPatchLossFn.apply(lx, ly, flags, int(padding), int(patch_size), float(scale), [] if out is None else out)


class _IICPatchHeadsLossFn(torch.autograd.Function):
    """``scale * sum_s mean_P IIDSegmentationLoss(softmax(lx_s), softmax(flip(ly)_s))`` over the S subheads of two logit maps
    (the decoder criterion of ``IICEstimator``): the launches of ``_IICPatchLossFn`` with the subhead as a grid axis.
    ``lx`` / ``ly``: logical [N, ld, H, W] f32 logits, ld >= S*K, subhead s in channels s*K .. s*K+K-1; the channels beyond
    S*K get a zero gradient.  ``out`` receives (losses f32 [S, nP], nan flag int32 [1])."""

    @staticmethod
    def forward(ctx, lx, ly, flags, S, K, pad, patch, scale, out):
        _n.require_gpu(lx, ly)
        xs, ys = _class_map_storage(lx.detach()), _class_map_storage(ly.detach())
        if xs.shape != ys.shape:
            raise AssertionError(f"logit maps {tuple(xs.shape)} / {tuple(ys.shape)} differ")
        N, H, W, ld = xs.shape
        dev = xs.device
        n_patches, ws_bytes, dj_elems = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        _n.call("spcl_iic_patch_heads_plan", N, S, K, ld, H, W, pad, patch, ctypes.byref(n_patches), ctypes.byref(ws_bytes),
                ctypes.byref(dj_elems))
        nP = len(iic_patch_starts(H, patch)) * len(iic_patch_starts(W, patch))
        assert nP == n_patches.value, (nP, n_patches.value)
        fl = _flip_flags_arg(flags, N, dev)
        ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device=dev)
        dj = torch.empty(dj_elems.value, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        per_patch = torch.empty(S, nP, dtype=torch.float32, device=dev)
        flag = torch.empty(1, dtype=torch.int32, device=dev)
        _n.call("spcl_iic_patch_heads_forward", _n.ptr(xs), _n.ptr(ys), ld, N, H, W, S, K, pad, patch, _n.ptr(fl), c_float(scale),
                _n.ptr(loss), _n.ptr(per_patch), _n.ptr(flag), _n.ptr(dj), _n.ptr(ws), ws.numel(), _n.stream())
        out.extend([per_patch, flag])
        ctx.save_for_backward(xs, ys, dj, fl)
        ctx.meta = (S, K, pad, patch)
        return loss

    @staticmethod
    def backward(ctx, g):
        xs, ys, dj, fl = ctx.saved_tensors
        S, K, pad, patch = ctx.meta
        N, H, W, ld = xs.shape
        gs = None if is_unit_gradient(g) else g.detach().float().reshape(1).contiguous()
        alloc = torch.empty_like if ld == S * K else torch.zeros_like  # (the launch leaves the channels beyond S*K alone)
        dlx = alloc(xs)
        dly = alloc(ys) if ctx.needs_input_grad[1] else None
        _n.call("spcl_iic_patch_heads_backward", _n.ptr(xs), _n.ptr(ys), ld, N, H, W, S, K, pad, patch, _n.ptr(fl), _n.ptr(dj),
                _n.ptr(gs), _n.ptr(dlx), _n.ptr(dly), _n.stream())
        return (dlx.permute(0, 3, 1, 2), None if dly is None else dly.permute(0, 3, 1, 2), None, None, None, None, None, None,
                None)


def iic_patch_heads_loss(lx, ly, *, num_subheads, num_clusters, padding, patch_size, scale=1.0, flags=None, out=None):
    """``scale * sum_s IIDSegmentationSmallPathLoss(padding, patch_size)(softmax(lx_s), softmax(flip(ly)_s))`` of logical
    [N, >= S*K, H, W] logits with K <= 32 clusters a subhead (discrete_mi_estimator.py:53-60 sums the same terms and divides by
    S: pass ``scale = 1 / S``); differentiable w.r.t. ``lx``, and w.r.t. ``ly`` when it requires grad.  ``flags`` flip Y.
    ``out`` (a list) receives (losses [S, nP], not scaled; nan flag int32 [1])."""
    return _IICPatchHeadsLossFn.apply(lx, ly, flags, int(num_subheads), int(num_clusters), int(padding), int(patch_size),
                                      float(scale), [] if out is None else out)


class _GroupL2NormTempFn(torch.autograd.Function):
    """``Normalize()`` and ``SoftmaxWithT``'s division of the cluster heads on [rows, ld] f32 logits (a [N, ld, H, W] map is
    its N*H*W channels-last rows): per subhead ``l / max(||l_s||, 1e-12) / T`` (csrc/projector.hip)"""

    @staticmethod
    def forward(ctx, x, S, K, normalize, T):
        _n.require_gpu(x)
        xs = _class_map_storage(x.detach()) if x.dim() == 4 else x.detach().contiguous().float()
        ld = xs.shape[-1]
        rows = xs.numel() // ld
        z = torch.empty_like(xs) if ld == S * K else torch.zeros_like(xs)
        _n.call("spcl_group_l2norm_temp_forward", _n.ptr(xs), rows, ld, S, K, int(normalize), c_float(T), _n.ptr(z), _n.stream())
        ctx.save_for_backward(xs)
        ctx.meta = (S, K, int(normalize), T, x.dim())
        return z.permute(0, 3, 1, 2) if x.dim() == 4 else z

    @staticmethod
    def backward(ctx, dz):
        (xs,) = ctx.saved_tensors
        S, K, normalize, T, dim = ctx.meta
        ld = xs.shape[-1]
        rows = xs.numel() // ld
        dzs = _class_map_storage(dz.detach()) if dim == 4 else dz.detach().contiguous().float()
        dx = torch.empty_like(xs) if ld == S * K else torch.zeros_like(xs)
        _n.call("spcl_group_l2norm_temp_backward", _n.ptr(xs), _n.ptr(dzs), rows, ld, S, K, normalize, c_float(T), _n.ptr(dx),
                _n.stream())
        return (dx.permute(0, 3, 1, 2) if dim == 4 else dx), None, None, None, None


def group_l2norm_temp(logits, *, num_subheads, num_clusters, normalize, T=1.0):
    """the cluster heads' ``Normalize() if normalize else Identical()`` then ``/ T`` on the logits of S subheads of K clusters:
    [rows, >= S*K] rows or a logical [N, >= S*K, H, W] map.  No launch (the argument itself) when there is nothing to do."""
    if not normalize and float(T) == 1.0:
        return logits
    return _GroupL2NormTempFn.apply(logits, int(num_subheads), int(num_clusters), bool(normalize), float(T))


class _PixelCriterionFn(torch.autograd.Function):
    """A fused per-pixel criterion (csrc/pixel_criterion.hpp): ``launch()`` checks its arguments, makes the one library call
    on detached channels-last storage and returns the loss and the gradient map [N, H, W, C] w.r.t. ``x`` for a unit upstream
    gradient; ``x`` is the one input that gets a gradient."""

    @staticmethod
    def forward(ctx, x, launch):
        loss, grad = launch()
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        if is_unit_gradient(g):
            return grad.permute(0, 3, 1, 2), None
        return (grad * g.detach().float()).permute(0, 3, 1, 2), None


_MixupKLFn = _PixelCriterionFn  # (the name tests/test_gpu_mixup_kernels.py drives ``backward`` under)


def _pixel_criterion_buffers(storage, workspace_entry):
    """(loss, gradient map, workspace) of a criterion over the [N, H, W, C] ``storage``"""
    N, H, W, _ = storage.shape
    dev = storage.device
    return (torch.empty((), dtype=torch.float32, device=dev), torch.empty_like(storage),
            torch.empty(_n.call(workspace_entry, N, H, W), dtype=torch.uint8, device=dev))


def consistency_softmax_mse(a, b, weight=1.0, flags=None):
    """consistency.py:30-35: ``weight * mse(softmax(flip(a)).detach(), softmax(b))`` of logical [N, C, H, W] logits"""
    weight = float(weight)

    def launch():
        _n.require_gpu(a, b)
        as_, bs = _class_map_storage(a.detach()), _class_map_storage(b.detach())
        if as_.shape != bs.shape:
            raise AssertionError(f"class maps {tuple(as_.shape)} / {tuple(bs.shape)} differ")
        N, H, W, C = bs.shape
        fl = _flip_flags_arg(flags, N, bs.device)
        loss, db, ws = _pixel_criterion_buffers(bs, "spcl_consistency_workspace_bytes")
        _n.call("spcl_consistency_softmax_mse", _n.ptr(as_), _n.ptr(bs), N, C, H, W, _n.ptr(fl), c_float(weight),
                _n.ptr(loss), _n.ptr(db), _n.ptr(ws), ws.numel(), _n.stream())
        return loss, db

    return _PixelCriterionFn.apply(b, launch)


# ------------------------------------------------------------------- mean teacher / entropy minimisation (csrc/semi_reg.hip)
def ema_update_(teacher_flat, student_flat, alpha, decay=0.0):
    """in place ``teacher = (alpha * teacher + (1 - alpha) * student) * (1 - decay)`` over two f32 tensors of one size, each
    dense in memory (mt.py:54 -> deepclustering2 ``ema_updater``), one launch; any 4-byte-aligned view will do"""
    _n.require_gpu(teacher_flat, student_flat)
    t, s = teacher_flat.detach(), student_flat.detach()
    if t.dtype != torch.float32 or s.dtype != torch.float32 or t.numel() != s.numel() or t.device != s.device:
        raise ValueError(f"ema_update_: two f32 tensors of one size on one device, got {t.dtype} {tuple(t.shape)} on {t.device} "
                         f"and {s.dtype} {tuple(s.shape)} on {s.device}")
    if not (t.is_contiguous() and s.is_contiguous()):
        raise ValueError("ema_update_: both tensors must be contiguous (a copy would not be updated in place)")
    if t.numel() > 0:
        _n.call("spcl_ema_update", _n.ptr(t), _n.ptr(s), t.numel(), c_double(alpha), c_double(decay), _n.stream())
    return teacher_flat


def mt_softmax_mse(teacher, student_logits, weight=1.0, flags=None, teacher_softmax=False):
    """mt.py:48-52: ``weight * mse(flip(teacher), softmax(student_logits))`` of logical [N, C, H, W] maps; with
    ``teacher_softmax`` the teacher's map is soft-maxed first (_mixins.py:147)"""
    weight = float(weight)

    def launch():
        _n.require_gpu(teacher, student_logits)
        ts, ss = _class_map_storage(teacher.detach()), _class_map_storage(student_logits.detach())
        if ts.shape != ss.shape:
            raise AssertionError(f"class maps {tuple(ts.shape)} / {tuple(ss.shape)} differ")
        N, H, W, C = ss.shape
        fl = _flip_flags_arg(flags, N, ss.device)
        loss, ds, ws = _pixel_criterion_buffers(ss, "spcl_mt_softmax_mse_workspace_bytes")
        _n.call("spcl_mt_softmax_mse", _n.ptr(ts), _n.ptr(ss), N, C, H, W, _n.ptr(fl), 1 if teacher_softmax else 0,
                c_float(weight), _n.ptr(loss), _n.ptr(ds), _n.ptr(ws), ws.numel(), _n.stream())
        return loss, ds

    return _PixelCriterionFn.apply(student_logits, launch)


def entropy_softmax(logits, eps=1e-16, weight=1.0):
    """entmin.py:30-31: ``weight * mean over pixels of -sum_c p_c log(p_c + eps)``, ``p = softmax(logits)``, of logical
    [N, C, H, W] logits"""
    eps, weight = float(eps), float(weight)

    def launch():
        _n.require_gpu(logits)
        ls = _class_map_storage(logits.detach())
        N, H, W, C = ls.shape
        loss, dl, ws = _pixel_criterion_buffers(ls, "spcl_entropy_softmax_workspace_bytes")
        _n.call("spcl_entropy_softmax", _n.ptr(ls), N, C, H, W, c_float(eps), c_float(weight), _n.ptr(loss), _n.ptr(dl),
                _n.ptr(ws), ws.numel(), _n.stream())
        return loss, dl

    return _PixelCriterionFn.apply(logits, launch)


UCMT_MAX_NOISY = 16  # the K device pointers travel in the kernel's argument block


def ucmt_softmax_mse(teacher, noisy_list, student_logits, threshold, weight=1.0, flags=None, eps=1e-16, out=None):
    """comparable.py:84-105: ``weight * (mse(softmax(student_logits), softmax(flip(teacher)), reduction="none").mean(1) *
    mask).mean()`` of logical [N, C, H, W] maps, ``mask = Entropy(softmax(flip(mean of noisy_list))) / log(C) <= threshold``
    (the K noisy teacher maps are summed in list order in f32 and divided by ``float(K)``, as ``average_iter`` does; the
    average of the flipped maps is the flip of the average).  The gradient goes to the student only.  ``out`` (a list)
    receives ``(kept, mask)``: the number of pixels with mask = 1 as an int64 device scalar (no readback here) and the mask as
    uint8 [N, H, W] in the student's frame."""
    noisy = tuple(noisy_list)
    threshold, eps, weight = float(threshold), float(eps), float(weight)

    def launch():
        _n.require_gpu(teacher, student_logits, *noisy)
        if not 1 <= len(noisy) <= UCMT_MAX_NOISY:
            raise ValueError(f"ucmt_softmax_mse: {len(noisy)} noisy maps (1 <= K <= {UCMT_MAX_NOISY})")
        ts, ss = _class_map_storage(teacher.detach()), _class_map_storage(student_logits.detach())
        ns = [_class_map_storage(t.detach()) for t in noisy]
        for t in [ts] + ns:
            if t.shape != ss.shape or t.device != ss.device:
                raise AssertionError(f"class maps {tuple(t.shape)} on {t.device} / {tuple(ss.shape)} on {ss.device} differ")
        N, H, W, C = ss.shape
        dev = ss.device
        fl = _flip_flags_arg(flags, N, dev)
        loss, ds, ws = _pixel_criterion_buffers(ss, "spcl_ucmt_workspace_bytes")
        kept = torch.empty((), dtype=torch.int64, device=dev)
        mask = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if out is not None else None
        _n.call("spcl_ucmt_softmax_mse", _n.ptr(ts), _n.ptr_array(ns), len(ns), _n.ptr(ss), N, C, H, W, _n.ptr(fl),
                c_float(threshold), c_float(eps), c_float(weight), _n.ptr(loss), _n.ptr(ds), _n.ptr(kept), _n.ptr(mask),
                _n.ptr(ws), ws.numel(), _n.stream())
        if out is not None:
            out.extend((kept, mask))
        return loss, ds

    return _PixelCriterionFn.apply(student_logits, launch)


# ------------------------------------------------------------------------------- pseudo-labelling (csrc/pseudo_label.hip)
def pseudo_label_state(C, device):
    """``(tau, state)`` of the self-adaptive thresholds at their initial values (FreeMatch, Algorithm 1): ``tau`` f32 [C] and
    ``state = (tau_g, ptilde[0 .. C))`` f64 [1 + C], every entry ``1 / C``"""
    C = int(C)
    if not 1 <= C <= 16:
        raise ValueError(f"pseudo_label_state: C = {C} (1 <= C <= 16)")
    return (torch.full((C,), 1.0 / C, dtype=torch.float32, device=device),
            torch.full((1 + C,), 1.0 / C, dtype=torch.float64, device=device))


def _pseudo_label_vector(t, name, dtype, n, dev):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"pseudo_label_ce: `{name}` must be a {dtype} [{n}] tensor on {dev}, got {type(t).__name__}")
    _n.require_gpu(t)
    if t.dtype != dtype or t.dim() != 1 or t.numel() != n or t.device != dev or not t.is_contiguous():
        raise ValueError(f"pseudo_label_ce: `{name}` must be a contiguous {dtype} [{n}] tensor on {dev}: got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}")
    return t.detach()


def pseudo_label_ce(teacher, student_logits, tau, weight=1.0, flags=None, state=None, momentum=0.999, out=None):
    """FixMatch's masked cross-entropy of logical [N, C, H, W] maps in one launch: ``weight * mean over ALL pixels of [conf >=
    tau[y]] * cross_entropy(student_logits, y)`` with ``y = argmax(flip(teacher))`` (the lowest class on a tie) and ``conf =
    max softmax(flip(teacher))``.  The gradient goes to the student only.  ``tau``: f32 [C] on the device.  ``state`` (f64
    [1 + C] on the device, see ``pseudo_label_state``) switches FreeMatch's self-adaptive thresholds on: this call compares
    against ``tau`` as it stands, then the same launch moves ``state`` and ``tau`` in place by the batch's statistics with
    ``momentum`` -- nothing is read back.  ``out`` (a list) receives ``(stats, hist, label)``: ``stats`` f64 [1 + C] = (sum
    conf, sum softmax(teacher)_c) over all pixels, ``hist`` int64 [2 C] = (pixels per class, kept pixels per class), ``label``
    uint8 [N, H, W] = the pseudo-label of a kept pixel and 255 elsewhere, in the student's frame."""
    weight, momentum = float(weight), float(momentum)
    if not 0.0 <= momentum < 1.0:
        raise ValueError(f"pseudo_label_ce: momentum {momentum} outside [0, 1)")

    def launch():
        _n.require_gpu(teacher, student_logits)
        ts, ss = _class_map_storage(teacher.detach()), _class_map_storage(student_logits.detach())
        if ts.shape != ss.shape or ts.device != ss.device:
            raise AssertionError(f"class maps {tuple(ts.shape)} on {ts.device} / {tuple(ss.shape)} on {ss.device} differ")
        N, H, W, C = ss.shape
        dev = ss.device
        tv = _pseudo_label_vector(tau, "tau", torch.float32, C, dev)
        sv = None if state is None else _pseudo_label_vector(state, "state", torch.float64, 1 + C, dev)
        fl = _flip_flags_arg(flags, N, dev)
        loss, ds = torch.empty((), dtype=torch.float32, device=dev), torch.empty_like(ss)
        ws = torch.empty(max(8, _n.call("spcl_pseudo_label_workspace_bytes", N, C, H, W)), dtype=torch.uint8, device=dev)
        stats = torch.empty(1 + C, dtype=torch.float64, device=dev)
        hist = torch.empty(2 * C, dtype=torch.int64, device=dev)
        label = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if out is not None else None
        _n.call("spcl_pseudo_label_ce", _n.ptr(ts), _n.ptr(ss), N, C, H, W, _n.ptr(fl), _n.ptr(tv), _n.ptr(sv),
                c_double(momentum), c_float(weight), _n.ptr(loss), _n.ptr(ds), _n.ptr(stats), _n.ptr(hist), _n.ptr(label),
                _n.ptr(ws), ws.numel(), _n.stream())
        if out is not None:
            out.extend((stats, hist, label))
        return loss, ds

    return _PixelCriterionFn.apply(student_logits, launch)


# ------------------------------------------------------------------------ cross pseudo supervision (csrc/cross_pseudo.hip)
class _PixelCriterion2Fn(torch.autograd.Function):
    """``_PixelCriterionFn`` for a criterion of two class maps that BOTH get a gradient: ``launch()`` returns the loss and the
    two gradient maps [N, H, W, C] w.r.t. ``x`` and ``y`` for a unit upstream gradient.  (Given one tensor on both sides,
    autograd adds the two maps.)"""

    @staticmethod
    def forward(ctx, x, y, launch):
        loss, gx, gy = launch()
        ctx.save_for_backward(gx, gy)
        return loss

    @staticmethod
    def backward(ctx, g):
        gx, gy = ctx.saved_tensors
        if is_unit_gradient(g):
            return gx.permute(0, 3, 1, 2), gy.permute(0, 3, 1, 2), None
        s = g.detach().float()
        return (gx * s).permute(0, 3, 1, 2), (gy * s).permute(0, 3, 1, 2), None


_CROSS_PSEUDO_WS = {}


def _cross_pseudo_workspace(nbytes, dev, layout):
    """The criterion's workspace for calls on the current stream of ``dev``: allocated zero-filled on first use and KEPT, one
    per LAYOUT and size.  The entry zeroes nothing (include/spcl_hip.h): the ticket starts at zero here and every launch
    leaves it at zero; calls on one stream run one after the other, so they share the workspace, and a captured launch points
    at memory that outlives its graph.  ``layout`` = (entry, C): the ticket lies behind the rows of doubles, at an offset that
    depends on the number of workgroups, and two layouts can ask for the same number of bytes (``cross_pseudo_ce`` on 22 x 4 x
    32 x 32 and ``cross_pseudo_ce_mixed`` on 21 x 4 x 32 x 32: 1912 bytes each; one entry at C = 2 with 17 workgroups and at C = 3
    with 13: 948 bytes each) -- a buffer one layout has used holds partial sums where the other expects its zero ticket.  Entry,
    C and size together fix the number of workgroups, so one buffer only ever sees one layout."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream, nbytes, layout)
    ws = _CROSS_PSEUDO_WS.get(key)
    if ws is None:
        ws = _CROSS_PSEUDO_WS[key] = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    return ws


def cross_pseudo_ce(a_logits, b_logits, tau=None, weight=1.0, out=None):
    """Cross pseudo supervision (Chen et al., CVPR 2021) of logical [N, C, H, W] logits of two networks on the same images, in
    one launch: ``weight * mean over ALL pixels of [confB >= tau[yB]] * cross_entropy(a_logits, yB) + [confA >= tau[yA]] *
    cross_entropy(b_logits, yA)`` with ``yA = argmax(a_logits)``, ``yB = argmax(b_logits)`` (the lowest class on a tie) and
    ``conf = max softmax``, formed as ``pseudo_label_ce`` forms it.  BOTH maps get a gradient; the labels carry none.  ``tau``:
    f32 [C] on the device, or None: every pixel is kept.  ``out`` (a list) receives ``(parts, hist, label_a, label_b)``:
    ``parts`` f32 [2] = the two directions (a <- b, b <- a), ``hist`` int64 [4 C + 1] = (pixels per yA, pixels per yB, kept
    pixels per yA, kept pixels per yB, pixels with yA == yB), ``label_a`` / ``label_b`` uint8 [N, H, W] = the label a network
    teaches where it is kept and 255 elsewhere."""
    weight = float(weight)

    def launch():
        _n.require_gpu(a_logits, b_logits)
        as_, bs = _class_map_storage(a_logits.detach()), _class_map_storage(b_logits.detach())
        if as_.shape != bs.shape or as_.device != bs.device:
            raise AssertionError(f"class maps {tuple(as_.shape)} on {as_.device} / {tuple(bs.shape)} on {bs.device} differ")
        N, H, W, C = as_.shape
        dev = as_.device
        if C > 16:
            raise ValueError(f"cross_pseudo_ce: C = {C} (1 <= C <= 16)")
        tv = None
        if tau is not None:
            if not isinstance(tau, torch.Tensor):
                raise ValueError(f"cross_pseudo_ce: `tau` must be a torch.float32 [{C}] tensor on {dev}, got "
                                 f"{type(tau).__name__}")
            if tau.dtype != torch.float32 or tau.dim() != 1 or tau.numel() != C or tau.device != dev or not tau.is_contiguous():
                raise ValueError(f"cross_pseudo_ce: `tau` must be a contiguous torch.float32 [{C}] tensor on {dev}: got "
                                 f"{tau.dtype} {tuple(tau.shape)} on {tau.device}")
            tv = tau.detach()
        loss = torch.empty((), dtype=torch.float32, device=dev)
        parts = torch.empty(2, dtype=torch.float32, device=dev)
        da, db = torch.empty_like(as_), torch.empty_like(bs)
        ws = _cross_pseudo_workspace(max(8, _n.call("spcl_cross_pseudo_workspace_bytes", N, C, H, W)), dev, ("cps", C))
        hist = torch.empty(4 * C + 1, dtype=torch.int64, device=dev)
        la = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if out is not None else None
        lb = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if out is not None else None
        _n.call("spcl_cross_pseudo_ce", _n.ptr(as_), _n.ptr(bs), N, C, H, W, _n.ptr(tv), c_float(weight), _n.ptr(loss),
                _n.ptr(parts), _n.ptr(da), _n.ptr(db), _n.ptr(hist), _n.ptr(la), _n.ptr(lb), _n.ptr(ws), ws.numel(),
                _n.stream())
        if out is not None:
            out.extend((parts, hist, la, lb))
        return loss, da, db

    return _PixelCriterion2Fn.apply(a_logits, b_logits, launch)


# ------------------------------------------------------------------- CutMix for cross pseudo supervision (csrc/cutmix.hip)
CUTMIX_MAX_N = 1 << 20


def _cutmix_share16(prop_range, what):
    """``prop_range = (lo, hi)``, the box's share of the image area, in the kernel's units of 1 / 65536"""
    try:
        lo, hi = (float(v) for v in prop_range)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: prop_range must be a pair (lo, hi), given {prop_range!r}") from None
    if not 0.0 < lo <= hi <= 1.0:
        raise ValueError(f"{what}: prop_range ({lo}, {hi}) must satisfy 0 < lo <= hi <= 1")
    lo16, hi16 = int(round(lo * 65536)), int(round(hi * 65536))
    if not 1 <= lo16 <= hi16 <= 65536:
        raise ValueError(f"{what}: prop_range ({lo}, {hi}) is below the rule's resolution of 1 / 65536")
    return lo16, hi16


def _cutmix_boxes_arg(boxes, N, dev, what):
    if not isinstance(boxes, torch.Tensor):
        raise ValueError(f"{what}: `boxes` must be a torch.int32 [{N}, 4] tensor on {dev}, got {type(boxes).__name__}")
    if boxes.dtype != torch.int32 or tuple(boxes.shape) != (N, 4) or boxes.device != dev:
        raise ValueError(f"{what}: `boxes` must be a torch.int32 [{N}, 4] tensor on {dev}: got {boxes.dtype} "
                         f"{tuple(boxes.shape)} on {boxes.device}")
    return boxes.detach().contiguous()


def _cutmix_roll_arg(roll, N, what):
    if isinstance(roll, bool) or not isinstance(roll, int) or not 1 <= roll <= N - 1:
        raise ValueError(f"{what}: roll = {roll!r} for {N} samples (an integer in 1 .. N - 1: the mix needs two samples)")
    return roll


def cutmix_boxes(seed, N, H, W, prop_range=(0.25, 0.5), device=None):
    """One CutMix box per sample (``spcl_cutmix_boxes``, one launch) -> int32 [N, 4] = ``(y0, x0, bh, bw)``: rows ``[y0, y0 +
    bh)``, columns ``[x0, x0 + bw)`` of an H x W image.  The box's share of the area is uniform in ``prop_range``, its aspect
    ratio follows French et al.'s generator with a linear-uniform side share and a fair bit for tall / wide (include/spcl_hip.h
    states the integer rule; tests/_cutmix_oracle.py restates it exactly).  ``seed``: a Python int in [0, 2^32) or a one-element
    int32 device tensor (read by the kernel, so a captured call replays with what it holds then), as ``pixel_sample``'s.
    Nothing is read back; the same bits on every run.  Bad arguments raise ``ValueError`` on the host."""
    for name, v in (("N", N), ("H", H), ("W", W)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"cutmix_boxes: {name} must be a positive integer, given {v!r}")
    if N > CUTMIX_MAX_N:
        raise ValueError(f"cutmix_boxes: N = {N} samples (at most {CUTMIX_MAX_N})")
    lo16, hi16 = _cutmix_share16(prop_range, "cutmix_boxes")
    _pixel_seed_check(seed)
    if device is not None:
        dev = torch.device(device)
    elif isinstance(seed, torch.Tensor):
        dev = seed.device
    else:
        dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if dev.type != "cuda":
        _n.require_gpu(torch.empty(0, device=dev))  # (raises: there is no CPU path)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    sd = _pixel_seed_arg(seed, dev)
    boxes = torch.empty((N, 4), dtype=torch.int32, device=dev)
    _n.call("spcl_cutmix_boxes", _n.ptr(sd), N, H, W, lo16, hi16, _n.ptr(boxes), _n.stream())
    return boxes


def cutmix_images(x, boxes, roll=1):
    """The box-wise image mix (``spcl_cutmix_images``, one launch): ``out[n, :, h, w] = x[(n + roll) % N, :, h, w]`` inside box
    ``n`` and ``x[n, :, h, w]`` elsewhere -- ``torch.where(mask, x.roll(-roll, 0), x)``, bit for bit.  ``x``: [N, C, H, W], f32
    or bf16, contiguous or channels-last (the result has ``x``'s layout; any other striding is made contiguous first).
    ``boxes``: int32 [N, 4] on ``x``'s device (``cutmix_boxes``); their values steer the selection only, never an address.  No
    autograd: images carry no gradient."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype not in (torch.float32, torch.bfloat16) or x.numel() == 0:
        raise ValueError("cutmix_images takes a non-empty float32 or bfloat16 [N, C, H, W] batch, given "
                         f"{getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    _n.require_gpu(x)
    N, C, H, W = x.shape
    if x.numel() >= 2 ** 31:
        raise ValueError(f"cutmix_images: {tuple(x.shape)} has 2^31 elements or more")
    bx = _cutmix_boxes_arg(boxes, N, x.device, "cutmix_images")
    roll = _cutmix_roll_arg(roll, N, "cutmix_images")
    src = x.detach()
    if src.is_contiguous():
        cl = 0
    elif src.is_contiguous(memory_format=torch.channels_last):
        cl = 1
    else:
        src, cl = src.contiguous(), 0
    out = torch.empty_like(src, memory_format=torch.channels_last if cl else torch.contiguous_format)
    _n.call("spcl_cutmix_images", _n.ptr(src), _n.ptr(out), _n.dtype_code(src.dtype), N, C, H, W, cl, _n.ptr(bx), roll,
            _n.stream())
    return out


def cross_pseudo_ce_mixed(s_a, s_b, t_a, t_b, boxes=None, roll=1, tau=None, weight=1.0, out=None):
    """Cross pseudo supervision under CutMix in one launch (``spcl_cross_pseudo_ce_mixed``).  ``s_a`` / ``s_b``: the two
    networks' logits on the MIXED images (``cutmix_images``), both get a gradient; ``t_a`` / ``t_b``: their logits on the UNMIXED
    images, constants (detached here).  All four logical [N, C, H, W].  Pixel ``(n, h, w)`` takes its labels from the teachers'
    pixel ``(m, h, w)``, ``m = (n + roll) % N`` inside box ``n`` and ``n`` elsewhere (``boxes`` None: ``m = n``, ``roll`` is not
    looked at): ``weight * mean over ALL pixels of [confB >= tau[yB]] * cross_entropy(s_a, yB) + [confA >= tau[yA]] *
    cross_entropy(s_b, yA)`` with ``yA = argmax(t_a[m])``, ``confA = max softmax(t_a[m])`` formed as ``cross_pseudo_ce`` and
    ``pseudo_label_ce`` form it, likewise B.  No mixed teacher map is built.  ``tau``: f32 [C] on the device, or None: every
    pixel is kept.  ``out`` (a list) receives ``(parts, hist, label_a, label_b)``: ``parts`` f32 [2] = the two directions (s_a
    <- t_b, s_b <- t_a), ``hist`` int64 [4 C + 2] = (pixels per yA, pixels per yB, kept pixels per yA, kept pixels per yB,
    pixels with yA == yB, pixels inside a box), ``label_a`` / ``label_b`` uint8 [N, H, W] in the mixed frame = the label a
    teacher gives where it is kept and 255 elsewhere."""
    weight = float(weight)

    def launch():
        _n.require_gpu(s_a, s_b, t_a, t_b)
        maps = [_class_map_storage(t.detach()) for t in (s_a, s_b, t_a, t_b)]
        sas, sbs, tas, tbs = maps
        for other in maps[1:]:
            if other.shape != sas.shape or other.device != sas.device:
                raise AssertionError(f"class maps {tuple(sas.shape)} on {sas.device} / {tuple(other.shape)} on {other.device} "
                                     "differ")
        N, H, W, C = sas.shape
        dev = sas.device
        if C > 16:
            raise ValueError(f"cross_pseudo_ce_mixed: C = {C} (1 <= C <= 16)")
        tv = None
        if tau is not None:
            if not isinstance(tau, torch.Tensor):
                raise ValueError(f"cross_pseudo_ce_mixed: `tau` must be a torch.float32 [{C}] tensor on {dev}, got "
                                 f"{type(tau).__name__}")
            if tau.dtype != torch.float32 or tau.dim() != 1 or tau.numel() != C or tau.device != dev or not tau.is_contiguous():
                raise ValueError(f"cross_pseudo_ce_mixed: `tau` must be a contiguous torch.float32 [{C}] tensor on {dev}: got "
                                 f"{tau.dtype} {tuple(tau.shape)} on {tau.device}")
            tv = tau.detach()
        bx, r = None, 0
        if boxes is not None:
            bx = _cutmix_boxes_arg(boxes, N, dev, "cross_pseudo_ce_mixed")
            r = _cutmix_roll_arg(roll, N, "cross_pseudo_ce_mixed")
        loss = torch.empty((), dtype=torch.float32, device=dev)
        parts = torch.empty(2, dtype=torch.float32, device=dev)
        da, db = torch.empty_like(sas), torch.empty_like(sbs)
        ws = _cross_pseudo_workspace(max(8, _n.call("spcl_cross_pseudo_mixed_workspace_bytes", N, C, H, W)), dev,
                                      ("cps_mixed", C))
        hist = torch.empty(4 * C + 2, dtype=torch.int64, device=dev)
        la = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if out is not None else None
        lb = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if out is not None else None
        _n.call("spcl_cross_pseudo_ce_mixed", _n.ptr(sas), _n.ptr(sbs), _n.ptr(tas), _n.ptr(tbs), N, C, H, W, _n.ptr(bx), r,
                _n.ptr(tv), c_float(weight), _n.ptr(loss), _n.ptr(parts), _n.ptr(da), _n.ptr(db), _n.ptr(hist), _n.ptr(la),
                _n.ptr(lb), _n.ptr(ws), ws.numel(), _n.stream())
        if out is not None:
            out.extend((parts, hist, la, lb))
        return loss, da, db

    return _PixelCriterion2Fn.apply(s_a, s_b, launch)


# ------------------------------------------------------- strong intensity view of the unlabelled pair (csrc/strong_view.hip)
STRONG_VIEW_OPS = ("gamma", "contrast", "brightness", "blur", "noise")
STRONG_VIEW_NEUTRAL = (1.0, 1.0, 1.0, 0.0, 0.0)
# nnU-Net's intensity ranges restated for [0, 1] images (their effect on Dice is not measured)
STRONG_VIEW_DEFAULTS = {"gamma": {"p": 0.3, "range": (0.7, 1.5)}, "contrast": {"p": 0.5, "range": (0.75, 1.25)},
                        "brightness": {"p": 0.5, "range": (0.75, 1.25)}, "blur": {"p": 0.2, "range": (0.25, 1.0)},
                        "noise": {"p": 0.15, "range": (0.0, 0.05)}}
STRONG_VIEW_COLS = 16  # == SPCL_SV_COLS; columns: the five values, applied mask, noise seed word, mean, applied count
STRONG_VIEW_MAX_N = 1 << 20


def _f32(v: float) -> float:
    return struct.unpack("<f", struct.pack("<f", v))[0]


class StrongViewConfig:
    """The five intensity ops of ``strong_view``: for each of ``STRONG_VIEW_OPS`` a gate probability ``p`` in [0, 1] and a
    value ``range`` (lo, hi); an op left out keeps its entry of ``STRONG_VIEW_DEFAULTS``.  Normalised to what the kernel reads:
    ``p16 = round(p * 65536)`` and the range ends rounded to float32.  gamma is the exponent of the [0, 1]-clamped image,
    contrast the factor about the sample's mean, brightness a factor, blur the share t in [0, 1] of the binomial filter
    [1 4 6 4 1] / 16 (t = 1: variance 1), noise the standard deviation.  Every refusal is a ``ValueError`` on the host."""

    def __init__(self, **ops):
        unknown = sorted(set(ops) - set(STRONG_VIEW_OPS))
        if unknown:
            raise ValueError(f"StrongViewConfig: no op {unknown} (some of {list(STRONG_VIEW_OPS)})")
        self.p16, self.lo, self.hi = [], [], []
        for name in STRONG_VIEW_OPS:
            given = ops.get(name)
            if given is not None and not hasattr(given, "keys"):
                raise ValueError(f"StrongViewConfig: {name} must be a mapping with `p` and `range`, given {given!r}")
            section = dict(STRONG_VIEW_DEFAULTS[name], **(dict(given) if given is not None else {}))
            extra = sorted(set(section) - {"p", "range"})
            if extra:
                raise ValueError(f"StrongViewConfig: {name} has no key {extra} (`p` and `range`)")
            p = section["p"]
            if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
                raise ValueError(f"StrongViewConfig: {name} p = {p!r} must be a number in [0, 1]")
            try:
                lo, hi = (_f32(float(v)) for v in section["range"])
            except (TypeError, ValueError, OverflowError, struct.error):
                raise ValueError(f"StrongViewConfig: {name} range must be a pair (lo, hi) of float32 numbers, given "
                                 f"{section['range']!r}") from None
            if not lo <= hi < float("inf"):
                raise ValueError(f"StrongViewConfig: {name} range ({lo}, {hi}) must be finite with lo <= hi")
            if name in ("gamma", "brightness") and not lo > 0.0:
                raise ValueError(f"StrongViewConfig: {name} range ({lo}, {hi}) must lie above 0")
            if name in ("contrast", "noise") and lo < 0.0:
                raise ValueError(f"StrongViewConfig: {name} range ({lo}, {hi}) must not be negative")
            if name == "blur" and not (0.0 <= lo and hi <= 1.0):
                raise ValueError(f"StrongViewConfig: blur range ({lo}, {hi}) must lie in [0, 1] (the share of the binomial "
                                 "filter: variance at most 1)")
            self.p16.append(int(round(float(p) * 65536)))
            self.lo.append(lo)
            self.hi.append(hi)

    @classmethod
    def off(cls):
        """every gate at 0: the view is the plain flip"""
        return cls(**{name: {"p": 0.0} for name in STRONG_VIEW_OPS})

    def key(self):
        """the normalised config as a hashable value"""
        return tuple((name, self.p16[k], self.lo[k], self.hi[k]) for k, name in enumerate(STRONG_VIEW_OPS))

    def words(self):
        """the 15 host words of ``spcl_strong_view_params``: p16, bits of lo, bits of hi for each op"""
        w = []
        for k in range(len(STRONG_VIEW_OPS)):
            w += [self.p16[k]] + [struct.unpack("<i", struct.pack("<f", v))[0] for v in (self.lo[k], self.hi[k])]
        return (ctypes.c_int32 * len(w))(*w)

    def __eq__(self, other):
        return isinstance(other, StrongViewConfig) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return "StrongViewConfig(" + ", ".join(f"{n}={{'p': {p / 65536:g}, 'range': ({lo:g}, {hi:g})}}"
                                               for n, p, lo, hi in self.key()) + ")"


def strong_view_tile():
    """(T_h, T_w): the tile one workgroup of ``spcl_strong_view_apply`` owns"""
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    _n.call("spcl_strong_view_tile", ctypes.byref(th), ctypes.byref(tw))
    return th.value, tw.value


def _strong_view_image(x, what):
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype not in (torch.float32, torch.bfloat16) or x.numel() == 0:
        raise ValueError(f"{what} takes a non-empty float32 or bfloat16 [N, C, H, W] batch, given "
                         f"{getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    if x.requires_grad:
        raise ValueError(f"{what}: the batch requires a gradient -- the strong view has no backward (images carry none)")
    _n.require_gpu(x)
    if x.shape[0] > STRONG_VIEW_MAX_N:
        raise ValueError(f"{what}: N = {x.shape[0]} samples (at most {STRONG_VIEW_MAX_N})")
    if x[0].numel() >= 2 ** 31:
        raise ValueError(f"{what}: a sample of {tuple(x.shape[1:])} has 2^31 elements or more")
    return x.contiguous()


def strong_view_params(x, seed, cfg):
    """The per-sample table of the strong view (``spcl_strong_view_params``, one launch, one workgroup per sample) -> f32
    [N, 16]: columns 0 - 4 the values of gamma, contrast, brightness, blur, noise (the neutral 1, 1, 1, 0, 0 where the op's gate
    stayed shut), 5 the mask of applied ops as a float, 6 the sample's noise seed word bit-cast, 7 the mean of the sample
    (float64 sum in a fixed order, rounded once), 8 the number of applied ops.  ``seed``: a Python int in [0, 2^32) or a
    one-element int32 device tensor (read by the kernel: a captured call replays with what it holds then).  ``cfg``: a
    ``StrongViewConfig``.  include/spcl_hip.h states the rule; tests/_strong_view_oracle.py restates it bit for bit."""
    if not isinstance(cfg, StrongViewConfig):
        raise ValueError(f"strong_view_params: cfg must be a StrongViewConfig, given {type(cfg).__name__}")
    _pixel_seed_check(seed)
    xc = _strong_view_image(x, "strong_view_params")
    N, C, H, W = xc.shape
    sd = _pixel_seed_arg(seed, xc.device)
    table = torch.empty((N, STRONG_VIEW_COLS), dtype=torch.float32, device=xc.device)
    _n.call("spcl_strong_view_params", _n.ptr(xc), _n.dtype_code(xc.dtype), N, C, H, W, _n.ptr(sd), cfg.words(),
            _n.ptr(table), _n.stream())
    return table


def strong_view_apply(x, flags, table):
    """``flip_batch(x, flags)`` with the table's ops applied on the way (``spcl_strong_view_apply``, one launch): clamp to
    [0, 1] and gamma, contrast about the mean and brightness, the binomial blur, the integer Irwin-Hall noise, clamp.  A sample
    whose row is all-neutral is a pure copy: with every row neutral the result is ``flip_batch``'s, bit for bit.  ``flags``:
    uint8 [N] on the device (bit 0 flips H, bit 1 flips W); ``table``: f32 [N, 16] (``strong_view_params``).  No autograd."""
    xc = _strong_view_image(x, "strong_view_apply")
    N, C, H, W = xc.shape
    if not isinstance(flags, torch.Tensor) or flags.dtype != torch.uint8 or tuple(flags.shape) != (N,) or \
            flags.device != xc.device:
        raise ValueError(f"strong_view_apply: `flags` must be a torch.uint8 [{N}] tensor on {xc.device}")
    if not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or \
            tuple(table.shape) != (N, STRONG_VIEW_COLS) or table.device != xc.device:
        raise ValueError(f"strong_view_apply: `table` must be a torch.float32 [{N}, {STRONG_VIEW_COLS}] tensor on {xc.device}")
    out = torch.empty_like(xc)
    _n.call("spcl_strong_view_apply", _n.ptr(xc), _n.ptr(out), _n.dtype_code(xc.dtype), N, C, H, W,
            _n.ptr(flags.contiguous()), _n.ptr(table.detach().contiguous()), _n.stream())
    return out


def strong_view(x, flags, seed, cfg, out=None):
    """``strong_view_apply(x, flags, strong_view_params(x, seed, cfg))``: two launches.  ``out``: a list that receives the
    table."""
    table = strong_view_params(x, seed, cfg)
    if out is not None:
        out.append(table)
    return strong_view_apply(x, flags, table)


# --------------------------------------------------------------------- label-guided pixel contrast (csrc/pixel_contrast.hip)
PIXEL_CONTRAST_MAX_C, PIXEL_CONTRAST_MAX_K, PIXEL_CONTRAST_MAX_M, PIXEL_CONTRAST_MAX_D = 16, 1024, 4096, 256


def _pixel_contrast_ck(what, C, K):
    for name, v in (("C", C), ("K", K)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{what}: {name} must be an integer, given {v!r}")
    if not 2 <= C <= PIXEL_CONTRAST_MAX_C:
        raise ValueError(f"{what}: C = {C} classes (2 .. {PIXEL_CONTRAST_MAX_C})")
    if not 1 <= K <= PIXEL_CONTRAST_MAX_K:
        raise ValueError(f"{what}: K = {K} samples per class (1 .. {PIXEL_CONTRAST_MAX_K})")
    if C * K > PIXEL_CONTRAST_MAX_M:
        raise ValueError(f"{what}: C K = {C * K} rows (at most {PIXEL_CONTRAST_MAX_M})")


def _pixel_seed_check(seed):
    if isinstance(seed, torch.Tensor):
        if seed.dtype != torch.int32 or seed.numel() != 1:
            raise ValueError(f"pixel_sample: a seed tensor must hold one int32, given {seed.dtype} {tuple(seed.shape)}")
    elif isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 32:
        raise ValueError(f"pixel_sample: seed must be an integer in [0, 2^32) or a one-element int32 device tensor, given {seed!r}")


def _pixel_seed_arg(seed, dev):
    """the sampler's seed word on the device: a one-element int32 tensor as it is, a Python int in [0, 2^32) through a pinned
    asynchronous copy (no synchronisation)"""
    if isinstance(seed, torch.Tensor):
        _n.require_gpu(seed)
        if seed.device != dev:
            raise ValueError(f"pixel_sample: the seed lies on {seed.device}, the cell labels on {dev}")
        return seed.detach().reshape(1)
    host = torch.tensor([seed - 2 ** 32 if seed >= 2 ** 31 else seed], dtype=torch.int32)
    return host.pin_memory().to(dev, non_blocking=True)


def pixel_sample(cell_label, C, K, seed):
    """The class-balanced sample of cells (``spcl_pixel_sample``): ``cell_label`` int32 [B, h, w], a value c in [0, C) makes the
    cell eligible for class c, anything else (-1) for none.  Per class the ``min(K, n_c)`` eligible cells with the smallest
    keys ``fmix32(((i + 1) * 0x9E3779B1 mod 2^32) ^ seed)`` of their flat index i.  -> (``idx`` int32 [C, K]: the chosen flat
    indices in ascending order, then -1; ``count`` int32 [C]).  ``seed``: a Python int in [0, 2^32) or a one-element int32
    device tensor (read by the kernels, so a captured call replays with what it holds then).  A fixed number of launches,
    nothing read back, the same bits on every run.  Bad arguments raise ``ValueError`` on the host."""
    if not isinstance(cell_label, torch.Tensor) or cell_label.dtype != torch.int32:
        raise ValueError(f"pixel_sample takes an int32 cell-label map, given {getattr(cell_label, 'dtype', type(cell_label).__name__)}")
    if cell_label.dim() != 3 or min(cell_label.shape) < 1:
        raise ValueError(f"pixel_sample: cell labels must be [B, h, w], given {tuple(cell_label.shape)}")
    _pixel_contrast_ck("pixel_sample", C, K)
    ncells = cell_label.numel()
    if ncells >= 2 ** 31:
        raise ValueError(f"pixel_sample: {ncells} cells (fewer than 2^31)")
    _pixel_seed_check(seed)
    _n.require_gpu(cell_label)
    dev = cell_label.device
    sd = _pixel_seed_arg(seed, dev)
    cl = cell_label.detach().contiguous()
    idx = torch.empty((C, K), dtype=torch.int32, device=dev)
    count = torch.empty(C, dtype=torch.int32, device=dev)
    ws = torch.empty(_n.call("spcl_pixel_sample_workspace_bytes", ncells), dtype=torch.uint8, device=dev)
    _n.call("spcl_pixel_sample", _n.ptr(cl), ncells, C, K, _n.ptr(sd), _n.ptr(idx), _n.ptr(count), _n.ptr(ws), ws.numel(),
            _n.stream())
    return idx, count


class _GatherRowsFn(torch.autograd.Function):
    """rows[m] = feature cell idx[m] as f32 (zero rows for idx < 0), read from the map's channels-last storage in place; the
    gradient is zero except at the chosen cells (unique indices: plain stores)"""

    @staticmethod
    def forward(ctx, feat, idx):
        x, cs = as_nhwc(feat.detach())
        B, h, w, _ = x.shape
        Cf, M = feat.shape[1], idx.numel()
        rows = torch.empty((M, Cf), dtype=torch.float32, device=feat.device)
        _n.call("spcl_rows_gather_forward", _n.ptr(x), _n.dtype_code(x.dtype), B * h * w, Cf, cs, _n.ptr(idx), M, _n.ptr(rows),
                _n.stream())
        ctx.save_for_backward(idx)
        ctx.meta = (B, h, w, Cf, cs, x.dtype, feat.dtype)
        return rows

    @staticmethod
    def backward(ctx, drows):
        (idx,) = ctx.saved_tensors
        B, h, w, Cf, cs, xdt, fdt = ctx.meta
        g = drows.detach().contiguous().float()
        dfeat = torch.empty((B, h, w, cs), dtype=xdt, device=g.device)
        _n.call("spcl_rows_gather_backward", _n.ptr(g), _n.ptr(idx), idx.numel(), Cf, _n.ptr(dfeat), _n.dtype_code(xdt), B * h * w,
                cs, _n.stream())
        gfeat = nhwc_to_logical(dfeat, Cf)
        return (gfeat if gfeat.dtype == fdt else gfeat.to(fdt)), None


def gather_rows(feature, idx):
    """``rows[m, :] = feature[b, :, y, x]`` of the cell with flat index ``idx[m] = b h w + y w + x`` as f32 [idx.numel(), Cf];
    a row whose index is -1 is exactly zero.  ``feature``: a logical [B, Cf, h, w] map, f32 or bf16 (read in place when it is
    channels-last, padded pitch included); ``idx``: int32, any shape, its non-negative entries distinct (``pixel_sample``'s
    are).  Differentiable in ``feature``: the gradient is zero everywhere except the chosen cells."""
    if not isinstance(feature, torch.Tensor) or feature.dim() != 4 or feature.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("gather_rows takes a float32 or bfloat16 [B, Cf, h, w] map, given "
                         f"{getattr(feature, 'dtype', type(feature).__name__)} {tuple(getattr(feature, 'shape', ()))}")
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32 or idx.numel() < 1:
        raise ValueError(f"gather_rows: idx must be a non-empty int32 tensor, given {getattr(idx, 'dtype', type(idx).__name__)}")
    if feature.shape[0] * feature.shape[2] * feature.shape[3] >= 2 ** 31:
        raise ValueError(f"gather_rows: {tuple(feature.shape)} has 2^31 cells or more")
    _n.require_gpu(feature, idx)
    if idx.device != feature.device:
        raise ValueError(f"gather_rows: idx on {idx.device}, the feature on {feature.device}")
    return _GatherRowsFn.apply(feature, idx.detach().contiguous().reshape(-1))


class _PixelSupConFn(torch.autograd.Function):
    """``spcl_pixel_supcon_forward`` / ``_backward``: the label structure comes from ``count`` alone; the rows' log-sums stay
    in the workspace between the two calls"""

    @staticmethod
    def forward(ctx, z, count, C, K, t):
        zc = z.detach().contiguous()
        M, d = zc.shape
        dev = zc.device
        ws = torch.empty(_n.call("spcl_pixel_supcon_workspace_bytes", M, d), dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _n.call("spcl_pixel_supcon_forward", _n.ptr(zc), _n.ptr(count), C, K, d, c_float(t), _n.ptr(loss), _n.ptr(ws), ws.numel(),
                _n.stream())
        ctx.save_for_backward(zc, count, ws)
        ctx.meta = (C, K, d, t)
        return loss

    @staticmethod
    def backward(ctx, g):
        zc, count, ws = ctx.saved_tensors
        C, K, d, t = ctx.meta
        gs = None if is_unit_gradient(g) else g.detach().reshape(1).float().contiguous()
        dz = torch.empty_like(zc)
        _n.call("spcl_pixel_supcon_backward", _n.ptr(zc), _n.ptr(count), C, K, d, c_float(t), _n.ptr(gs), _n.ptr(ws), ws.numel(),
                _n.ptr(dz), _n.stream())
        return dz, None, None, None, None


def pixel_supcon(z, count, K, t=0.1):
    """The supervised-contrastive loss of the sampled rows: ``z`` f32 [C K, d] (unit rows; 4 <= d <= 256, a multiple of 4),
    ``count`` int32 [C] on the device.  Slot ``m = c K + j`` has class c and is valid iff ``j < count[c]``; with A(i) the valid
    rows other than i, P(i) those of i's class and I the valid rows with a positive,
    ``L = mean_{i in I} -(1 / |P(i)|) sum_{p in P(i)} [z_i.z_p / t - log sum_{a in A(i)} exp(z_i.z_a / t)]``, 0 for an empty
    I.  Invalid rows are never read (NaN allowed) and get an exactly zero gradient.  Nothing is read back."""
    if not isinstance(z, torch.Tensor) or z.dtype != torch.float32 or z.dim() != 2:
        raise ValueError(f"pixel_supcon takes float32 [C K, d] rows, given {getattr(z, 'dtype', type(z).__name__)} "
                         f"{tuple(getattr(z, 'shape', ()))}")
    if not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or count.dim() != 1:
        raise ValueError(f"pixel_supcon: count must be an int32 [C] tensor, given {getattr(count, 'dtype', type(count).__name__)}")
    C = int(count.numel())
    _pixel_contrast_ck("pixel_supcon", C, K)
    M, d = z.shape
    if M != C * K:
        raise ValueError(f"pixel_supcon: {M} rows for C K = {C} x {K}")
    if not 4 <= d <= PIXEL_CONTRAST_MAX_D or d % 4 != 0:
        raise ValueError(f"pixel_supcon: d = {d} (4 .. {PIXEL_CONTRAST_MAX_D}, a multiple of 4)")
    t = float(t)
    if not t > 0.0:
        raise ValueError(f"pixel_supcon: temperature {t} (> 0)")
    _n.require_gpu(z, count)
    if count.device != z.device:
        raise ValueError(f"pixel_supcon: count on {count.device}, the rows on {z.device}")
    return _PixelSupConFn.apply(z, count.detach().contiguous(), C, K, t)


def pixel_contrast_labels(labels, C, size):
    """The sampler's cell labels from label maps: ``labels`` uint8 [B, H, W] (values >= C: ignore), ``size`` = the hooked
    feature's (h, w).  A cell keeps its majority class iff its purity is 1.0 -- every label of its pooling window is that
    class, so boundary cells and windows with ignored pixels get -1.  -> int32 [B, h, w]."""
    cell, purity = cell_majority(labels, C, size)
    return torch.where(purity == 1.0, cell, -1)


# ------------------------------------------------------------------------------------------------ mix-up (csrc/semi_reg.hip)
class MixupPlan:
    """One mix-up draw (mixup.py:19-32) for a batch of B labelled samples and their second views: ``lam`` (the host's float64),
    ``pair`` = the f32 roundings of ``(lam, 1 - lam)`` the kernels compute with, ``n2`` = 2B and ``index`` = the permutation
    of the 2B samples as int32 on ``device`` (a pinned host buffer and an asynchronous copy: no synchronisation).

    ``perm``: a host integer sequence or CPU tensor, as ``torch.randperm(2B)`` returns it.  Checked HERE, on the host: an even
    length and every entry in [0, 2B) -- the kernels index their inputs by it."""

    def __init__(self, perm, lam, device):
        if isinstance(perm, torch.Tensor):
            if perm.is_cuda or perm.dim() != 1 or perm.is_floating_point() or perm.is_complex() or perm.dtype == torch.bool:
                raise ValueError("MixupPlan: `perm` must be a 1-d integer tensor on the CPU")
            entries = perm.tolist()
        else:
            entries = list(perm)
            if any(isinstance(v, bool) or int(v) != v for v in entries):
                raise ValueError("MixupPlan: `perm` must hold integers")
            entries = [int(v) for v in entries]
        n2 = len(entries)
        if n2 == 0 or n2 % 2 != 0:
            raise ValueError(f"MixupPlan: `perm` must index two batches of one size, got {n2} entries")
        if min(entries) < 0 or max(entries) >= n2:
            raise ValueError(f"MixupPlan: every entry of `perm` must lie in [0, {n2}), got {min(entries)} .. {max(entries)}")
        self.lam = float(lam)
        self.pair = (float(torch.tensor(self.lam, dtype=torch.float32)), float(torch.tensor(1 - self.lam, dtype=torch.float32)))
        self.n2 = n2
        host = torch.tensor(entries, dtype=torch.int32)
        device = torch.device(device)
        self.index = host.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else host


def _mixup_plan_arg(plan, n2, device):
    if not isinstance(plan, MixupPlan):
        raise TypeError(f"a MixupPlan is expected, got {type(plan).__name__}")
    if plan.n2 != n2:
        raise ValueError(f"the plan permutes {plan.n2} samples, the two batches hold {n2}")
    if plan.index.device != device:
        raise RuntimeError(f"the plan's index lives on {plan.index.device}, the tensors on {device}")
    return plan.index


def mixup_images(image, image_tf, plan):
    """mixup.py:30,70 in one launch: ``lam * x + (1 - lam) * x[index]`` over ``x = cat([image, image_tf])`` (never built) ->
    [2B, Cin, H, W] f32, bit for bit what torch computes on f32 tensors.  No autograd: the inputs are data."""
    _n.require_gpu(image, image_tf)
    a, b = image.detach(), image_tf.detach()
    if a.shape != b.shape or a.dim() < 2 or a.dtype != torch.float32 or b.dtype != torch.float32 or a.device != b.device:
        raise ValueError(f"mixup_images: two f32 batches of one shape on one device, got {a.dtype} {tuple(a.shape)} on "
                         f"{a.device} and {b.dtype} {tuple(b.shape)} on {b.device}")
    a, b = a.contiguous(), b.contiguous()
    B = a.shape[0]
    index = _mixup_plan_arg(plan, 2 * B, a.device)
    out = torch.empty((2 * B,) + tuple(a.shape[1:]), dtype=torch.float32, device=a.device)
    per = a.numel() // B if B else 0
    if per > 0:
        lam, oml = plan.pair
        _n.call("spcl_mixup_images", _n.ptr(a), _n.ptr(b), _n.ptr(index), 2 * B, per, c_float(lam), c_float(oml), _n.ptr(out),
                _n.stream())
    return out


def _label_map_arg(t, B, H, W, name):
    if t.dim() == 4 and t.shape[1] == 1:
        t = t.squeeze(1)
    if tuple(t.shape) != (B, H, W):
        raise ValueError(f"mixup_kl_onehot: `{name}` must be [{B}, 1, {H}, {W}] or [{B}, {H}, {W}], got {tuple(t.shape)}")
    if t.dtype != torch.int64:
        t = t.long()
    return t.contiguous()


def mixup_kl_onehot(logits, target, target_tf, plan, eps=1e-16, weight=1.0):
    """mixup.py:31,66-75: ``weight * KL_div(eps)(softmax(logits), mixed_y)`` of logical [2B, C, H, W] logits, ``mixed_y`` the
    plan's blend of the one-hot maps of ``cat([target, target_tf])`` and of their permutation (never built); targets
    [B, 1, H, W] or [B, H, W] integer label maps"""
    eps, weight = float(eps), float(weight)

    def launch():
        _n.require_gpu(logits, target, target_tf)
        ls = _class_map_storage(logits.detach())
        N2, H, W, C = ls.shape
        index = _mixup_plan_arg(plan, N2, ls.device)
        ya = _label_map_arg(target.detach(), N2 // 2, H, W, "target")
        yb = _label_map_arg(target_tf.detach(), N2 // 2, H, W, "target_tf")
        lam, oml = plan.pair
        loss, dl, ws = _pixel_criterion_buffers(ls, "spcl_mixup_kl_workspace_bytes")
        _n.call("spcl_mixup_kl_onehot", _n.ptr(ls), _n.ptr(ya), _n.ptr(yb), _n.ptr(index), N2, C, H, W, c_float(lam),
                c_float(oml), c_float(eps), c_float(weight), _n.ptr(loss), _n.ptr(dl), _n.ptr(ws), ws.numel(), _n.stream())
        return loss, dl

    return _PixelCriterionFn.apply(logits, launch)


# --------------------------------------------------------------------------------------------- DCGAN discriminator
# (csrc/discr.hip: the adversarial baseline, semi_seg/arch/discr.py:17-36 + nn.BCELoss of new_comparable.py:124)
DISCR_IDENTITY, DISCR_LEAKY, DISCR_BN_LEAKY = 0, 1, 2


class RowsBN:
    """what a training- or eval-mode ``nn.BatchNorm2d`` brings to a fused layer besides gamma / beta: its running
    statistics (updated in place by the forward launch in training mode), momentum, eps and the mode"""

    def __init__(self, running_mean, running_var, training, momentum=0.1, eps=1e-5):
        self.running_mean, self.running_var = running_mean, running_var
        self.training, self.momentum, self.eps = bool(training), float(momentum), float(eps)


def _f32_map(t, name):
    if t.dim() != 4 or t.dtype != torch.float32:
        raise ValueError(f"{name}: a float32 [N, C, H, W] map, got {t.dtype} {tuple(t.shape)}")
    return t.detach()


def patch4s2_rows(x, mode=DISCR_IDENTITY, scale=None, shift=None, x2=None):
    """patch rows [N Ho Wo, 16 C] of ``Conv2d(C, ., 4, 2, 1)`` over the logical [N, C, H, W] map ``x`` (any strides; with
    ``x2`` the channel concatenation [x, x2], nothing is concatenated), k = 16 c + 4 kh + kw, the input transform ``mode``
    applied on the way (include/spcl_hip.h).  No autograd."""
    _n.require_gpu(x, x2, scale, shift)
    x = _f32_map(x, "patch4s2_rows")
    N, Ca, H, W = x.shape
    Cb = 0
    if x2 is not None:
        x2 = _f32_map(x2, "patch4s2_rows")
        if x2.shape[0] != N or tuple(x2.shape[2:]) != (H, W):
            raise ValueError(f"patch4s2_rows: maps {tuple(x.shape)} and {tuple(x2.shape)} do not stack")
        Cb = x2.shape[1]
    C = Ca + Cb
    if mode == DISCR_BN_LEAKY and (scale is None or scale.numel() != C or shift.numel() != C):
        raise ValueError("patch4s2_rows: scale and shift of C elements")
    rows = torch.empty(N * (H // 2) * (W // 2), 16 * C, dtype=torch.float32, device=x.device)
    sa = x.stride()
    sb = x2.stride() if x2 is not None else (0, 0, 0, 0)
    _n.call("spcl_patch4s2_rows_forward", _n.ptr(x), Ca, sa[0], sa[1], sa[2], sa[3], _n.ptr(x2), Cb, sb[0], sb[1], sb[2], sb[3],
            N, H, W, int(mode), _n.ptr(scale), _n.ptr(shift), _n.ptr(rows), _n.stream())
    return rows


def patch4s2_rows_backward(drows, shape, mode=DISCR_IDENTITY, x_store=None, scale=None, shift=None, c_lo=0):
    """gather form of the patch rows' backward: ``drows`` [N Ho Wo, 16 C] -> [N, H, W, C - c_lo] (NHWC storage) times the
    transform's derivative at ``x_store`` [N, H, W, C]; in BN mode the gradient w.r.t. ``scale x + shift``"""
    _n.require_gpu(drows, x_store, scale, shift)
    N, C, H, W = shape
    if tuple(drows.shape) != (N * (H // 2) * (W // 2), 16 * C) or not drows.is_contiguous() or drows.dtype != torch.float32:
        raise ValueError(f"patch4s2_rows_backward: drows {tuple(drows.shape)} for a map {tuple(shape)}")
    if mode != DISCR_IDENTITY and (tuple(x_store.shape) != (N, H, W, C) or not x_store.is_contiguous()):
        raise ValueError("patch4s2_rows_backward: the stored map is [N, H, W, C], contiguous")
    dx = torch.empty(N, H, W, C - c_lo, dtype=torch.float32, device=drows.device)
    _n.call("spcl_patch4s2_rows_backward", _n.ptr(drows), _n.ptr(x_store), N, H, W, C, int(c_lo), int(mode), _n.ptr(scale),
            _n.ptr(shift), _n.ptr(dx), _n.stream())
    return dx


def _rows_bn_ws(M, C, dev):
    nbytes = _n.call("spcl_rows_bn_workspace_bytes", M, C)
    if nbytes == 0:
        raise ValueError(f"rows BatchNorm: M >= 2 rows of C % 4 == 0, C <= 1024 channels (got {M}, {C})")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def rows_bn_stats(x, gamma, beta, bn: RowsBN):
    """``stats`` [4, C] = (mean, invstd, scale, shift) of a BatchNorm over the rows of ``x`` [M, C]: batch statistics (and the
    running-statistic update, in place) in training mode, the running statistics otherwise"""
    _n.require_gpu(x, gamma, beta, bn.running_mean, bn.running_var)
    M, C = x.shape
    stats = torch.empty(4, C, dtype=torch.float32, device=x.device)
    if bn.training:
        ws = _rows_bn_ws(M, C, x.device)
        _n.call("spcl_rows_bn_forward", _n.ptr(x), M, C, _n.ptr(gamma), _n.ptr(beta), c_float(bn.eps), c_float(bn.momentum),
                _n.ptr(bn.running_mean), _n.ptr(bn.running_var), _n.ptr(stats), _n.ptr(ws), ws.numel(), _n.stream())
    else:
        _n.call("spcl_rows_bn_eval_affine", _n.ptr(gamma), _n.ptr(beta), _n.ptr(bn.running_mean), _n.ptr(bn.running_var),
                c_float(bn.eps), C, _n.ptr(stats), _n.stream())
    return stats


def rows_bn_backward(du, x, gamma, stats, training, sinks=(None, None)):
    """from ``du`` = dLoss/d(scale x + shift) [M, C]: (dx, dgamma, dbeta) of the BatchNorm, batch terms included in
    training mode.  ``dx`` overwrites ``du``."""
    M, C = x.shape
    dev = x.device
    dgamma, dbeta = _grad_buffer(sinks[0], (C,), dev), _grad_buffer(sinks[1], (C,), dev)
    ws = _rows_bn_ws(M, C, dev)
    _n.call("spcl_rows_bn_backward", _n.ptr(du), _n.ptr(x), M, C, _n.ptr(gamma), _n.ptr(stats), int(bool(training)), _n.ptr(du),
            _n.ptr(dgamma), _n.ptr(dbeta), _n.ptr(ws), ws.numel(), _n.stream())
    return du, dgamma, dbeta


def _rows_product(rows, w2d):
    """y [M, Cout] = rows [M, K] w2d[Cout, K]^T on the exact-f32 rows product (no bias: the discriminator's convolutions have none)"""
    M, K = rows.shape
    cout = w2d.shape[0]
    y = torch.empty(M, cout, dtype=torch.float32, device=rows.device)
    _n.call("spcl_rows_linear_forward", _n.ptr(rows), _n.SPCL_F32, K, 0, _n.ptr(w2d), None, M, K, cout, _n.ptr(y), _n.stream())
    return y


def _rows_product_backward(g, w2d, rows, sink):
    """(drows [M, K], dW [Cout, K] or None when ``rows`` is None: a pass that keeps no weight gradient computes none)"""
    M, cout = g.shape
    K = w2d.shape[1]
    dev = g.device
    drows = torch.empty(M, K, dtype=torch.float32, device=dev)
    _n.call("spcl_rows_linear_backward_input", _n.ptr(g), _n.SPCL_F32, _n.ptr(w2d), None, M, cout, K, _n.ptr(drows), _n.SPCL_F32, K,
            _n.stream())
    dw = None
    if rows is not None:
        dw = _grad_buffer(sink, (cout, K), dev)
        ws = torch.empty(_n.call("spcl_rows_linear_backward_weight_workspace_bytes", M, cout, K) // 4 + 1, dtype=torch.float32,
                         device=dev)
        _n.call("spcl_rows_linear_backward_weight", _n.ptr(g), _n.SPCL_F32, _n.ptr(rows), _n.SPCL_F32, K, 0, M, cout, K, _n.ptr(ws),
                ws.numel() * 4, _n.ptr(dw), None, _n.stream())
    return drows, dw


def _conv4_weight(w, C):
    """the contiguous [Cout, C, 4, 4] parameter as the product's [Cout, 16 C] matrix (a view: the k order is the parameter's)"""
    if w.dim() != 4 or tuple(w.shape[1:]) != (C, 4, 4) or w.dtype != torch.float32:
        raise ValueError(f"a float32 [Cout, {C}, 4, 4] convolution weight, got {w.dtype} {tuple(w.shape)}")
    if w.shape[0] % 4 != 0:
        raise ValueError(f"the rows product needs Cout % 4 == 0 (got {w.shape[0]}): hidden_dim must be a multiple of 4")
    return w.detach().contiguous().view(w.shape[0], 16 * C)


class _DiscrConvFn(torch.autograd.Function):
    """``Conv2d(C, Cout, 4, 2, 1, bias=False)`` over ``T(x)``, T the identity (discr.py:19; ``x2``: the class map behind the
    image ``x``, which gets no gradient) or LeakyReLU(0.2) of the stored pre-activation ``x`` (discr.py:20-22): patch rows +
    rows product.  Returns the pre-activation map, logical [N, Cout, Ho, Wo] on NHWC storage.  ``need_w`` False: no weight
    gradient is computed and the patch rows are not kept."""

    @staticmethod
    def forward(ctx, x, x2, weight, mode, need_w):
        _n.require_gpu(x, x2, weight)
        N, Ca, H, W = x.shape
        C = Ca + (x2.shape[1] if x2 is not None else 0)
        w2d = _conv4_weight(weight, C)
        xs = _class_map_storage(x.detach()) if mode == DISCR_LEAKY else None  # (kept for LeakyReLU')
        src = xs.permute(0, 3, 1, 2) if xs is not None else x
        rows = patch4s2_rows(src, mode, x2=x2)
        y = _rows_product(rows, w2d)
        ctx.save_for_backward(xs, w2d, rows if need_w else None)
        ctx.meta = (N, C, H, W, Ca if x2 is not None else 0, mode)
        ctx.weight = weight
        return y.view(N, H // 2, W // 2, w2d.shape[0]).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dy):
        xs, w2d, rows = ctx.saved_tensors
        N, C, H, W, c_lo, mode = ctx.meta
        g = _class_map_storage(dy.detach())
        g = g.view(-1, g.shape[3])
        ng = ctx.needs_input_grad
        want_w = rows is not None and ng[2]
        drows, dw = _rows_product_backward(g, w2d, rows if want_w else None, take_grad_sink(ctx.weight, want_w))
        dx = None
        if ng[1] if c_lo else ng[0]:
            dx = patch4s2_rows_backward(drows, (N, C, H, W), mode, xs, c_lo=c_lo).permute(0, 3, 1, 2)
        dwv = None if dw is None else dw.view(ctx.weight.shape)
        return (None, dx, dwv, None, None) if c_lo else (dx, None, dwv, None, None)


class _DiscrBnConvFn(torch.autograd.Function):
    """``BatchNorm2d -> LeakyReLU(0.2) -> Conv2d(C, Cout, 4, 2, 1, bias=False)`` of the stored pre-BN map ``x`` (discr.py:23-26,
    27-30): one statistics launch, patch rows with the affine + activation applied on read, rows product.  Backward: the
    full BatchNorm gradient (mean and variance terms) in training mode."""

    @staticmethod
    def forward(ctx, x, gamma, beta, weight, bn: RowsBN, need_w):
        _n.require_gpu(x, gamma, beta, weight)
        N, C, H, W = x.shape
        w2d = _conv4_weight(weight, C)
        xs = _class_map_storage(x.detach())
        gm, bt = gamma.detach().contiguous(), beta.detach().contiguous()
        stats = rows_bn_stats(xs.view(-1, C), gm, bt, bn)
        rows = patch4s2_rows(xs.permute(0, 3, 1, 2), DISCR_BN_LEAKY, stats[2], stats[3])
        y = _rows_product(rows, w2d)
        ctx.save_for_backward(xs, gm, stats, w2d, rows if need_w else None)
        ctx.meta = (N, C, H, W, bn.training, need_w)
        ctx.params = (gamma, beta, weight)
        return y.view(N, H // 2, W // 2, w2d.shape[0]).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dy):
        xs, gm, stats, w2d, rows = ctx.saved_tensors
        N, C, H, W, training, need_w = ctx.meta
        gamma, beta, weight = ctx.params
        g = _class_map_storage(dy.detach())
        g = g.view(-1, g.shape[3])
        ng = ctx.needs_input_grad
        want_w = rows is not None and ng[3]
        drows, dw = _rows_product_backward(g, w2d, rows if want_w else None, take_grad_sink(weight, want_w))
        du = patch4s2_rows_backward(drows, (N, C, H, W), DISCR_BN_LEAKY, xs, stats[2], stats[3])
        sinks = (take_grad_sink(gamma, need_w and ng[1]), take_grad_sink(beta, need_w and ng[2]))
        dx, dgamma, dbeta = rows_bn_backward(du.view(-1, C), xs.view(-1, C), gm, stats, training, sinks)
        if not need_w:
            dgamma = dbeta = None
        return (dx.view(N, H, W, C).permute(0, 3, 1, 2), dgamma, dbeta, None if dw is None else dw.view(weight.shape), None,
                None)


class _DiscrBnHeadFn(torch.autograd.Function):
    """``BatchNorm2d -> LeakyReLU(0.2) -> Conv2d(C, 1, 4, 1, 0, bias=False) -> Sigmoid`` of the stored pre-BN map ``x``
    (discr.py:31-35) and, with ``label`` 0 or 1, ``nn.BCELoss()(., label)`` (new_comparable.py:124,162-163,183-191) in the same
    launch.  Returns the loss (a 0-dim tensor) or, with ``label`` None, sigmoid(t) [N, 1, H - 3, W - 3]."""

    @staticmethod
    def forward(ctx, x, gamma, beta, weight, bn: RowsBN, label, need_w):
        _n.require_gpu(x, gamma, beta, weight)
        N, C, H, W = x.shape
        if tuple(weight.shape) != (1, C, 4, 4) or weight.dtype != torch.float32:
            raise ValueError(f"the head's weight is float32 [1, {C}, 4, 4], got {tuple(weight.shape)}")
        if label is not None and label not in (0, 1):
            raise ValueError(f"the BCE target is the constant 0 or 1, got {label!r}")
        dev = x.device
        xs = _class_map_storage(x.detach())
        gm, bt = gamma.detach().contiguous(), beta.detach().contiguous()
        w1d = weight.detach().contiguous().view(-1)
        stats = rows_bn_stats(xs.view(-1, C), gm, bt, bn)
        nbytes = _n.call("spcl_discr_head_workspace_bytes", N, H, W, C)
        if nbytes == 0:
            raise ValueError(f"discriminator head: a map of at least 4 x 4 with C % 4 == 0 (got {H} x {W}, C = {C})")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        M = N * (H - 3) * (W - 3)
        t, d = torch.empty(M, dtype=torch.float32, device=dev), torch.empty(M, dtype=torch.float32, device=dev)
        loss = dt = None
        if label is not None:
            loss, dt = torch.empty((), dtype=torch.float32, device=dev), torch.empty(M, dtype=torch.float32, device=dev)
        _n.call("spcl_discr_head_forward", _n.ptr(xs), N, H, W, C, _n.ptr(stats[2]), _n.ptr(stats[3]), _n.ptr(w1d),
                -1 if label is None else int(label), _n.ptr(t), _n.ptr(d), _n.ptr(loss), _n.ptr(dt), _n.ptr(ws), ws.numel(),
                _n.stream())
        ctx.save_for_backward(xs, gm, stats, w1d, dt if label is not None else d)
        ctx.meta = (N, C, H, W, bn.training, need_w, label is not None)
        ctx.params = (gamma, beta, weight)
        return loss if label is not None else d.view(N, 1, H - 3, W - 3)

    @staticmethod
    def backward(ctx, gout):
        xs, gm, stats, w1d, saved = ctx.saved_tensors
        N, C, H, W, training, need_w, is_loss = ctx.meta
        gamma, beta, weight = ctx.params
        dev = xs.device
        ng = ctx.needs_input_grad
        if is_loss:
            dt, grad = saved, (None if is_unit_gradient(gout) else gout.detach().float().reshape(1).contiguous())
        else:  # d sigmoid(t) = d (1 - d): M elements, not a hot path (the epocher goes through the loss)
            dt, grad = (gout.detach().float().reshape(-1) * saved * (1.0 - saved)).contiguous(), None
        want_w = need_w and ng[3]
        du = torch.empty(N, H, W, C, dtype=torch.float32, device=dev)
        dw = _grad_buffer(take_grad_sink(weight, want_w), (16 * C,), dev) if want_w else None
        ws = torch.empty(_n.call("spcl_discr_head_workspace_bytes", N, H, W, C), dtype=torch.uint8, device=dev)
        _n.call("spcl_discr_head_backward", _n.ptr(xs), N, H, W, C, _n.ptr(stats[2]), _n.ptr(stats[3]), _n.ptr(w1d), _n.ptr(dt),
                _n.ptr(grad), _n.ptr(du), _n.ptr(dw), _n.ptr(ws), ws.numel(), _n.stream())
        sinks = (take_grad_sink(gamma, need_w and ng[1]), take_grad_sink(beta, need_w and ng[2]))
        dx, dgamma, dbeta = rows_bn_backward(du.view(-1, C), xs.view(-1, C), gm, stats, training, sinks)
        if not need_w:
            dgamma = dbeta = None
        return (dx.view(N, H, W, C).permute(0, 3, 1, 2), dgamma, dbeta, None if dw is None else dw.view(weight.shape), None,
                None, None)


def discr_conv(x, weight, *, leaky_in=False, x2=None, weight_grads=True):
    """``Conv2d(., ., 4, 2, 1, bias=False)`` of ``x`` (``leaky_in``: of LeakyReLU(0.2)(x)); ``x2``: stacked behind ``x``, which
    then gets no gradient (the image in front of a class map)"""
    return _DiscrConvFn.apply(x, x2, weight, DISCR_LEAKY if leaky_in else DISCR_IDENTITY, bool(weight_grads))


def discr_bn_conv(x, gamma, beta, weight, bn: RowsBN, *, weight_grads=True):
    return _DiscrBnConvFn.apply(x, gamma, beta, weight, bn, bool(weight_grads))


def discr_bn_head(x, gamma, beta, weight, bn: RowsBN, *, label=None, weight_grads=True):
    return _DiscrBnHeadFn.apply(x, gamma, beta, weight, bn, label, bool(weight_grads))


# --------------------------------------------------------------------------------------------- MINE statistics network
class _MinePairsFn(torch.autograd.Function):
    """The statistics network's two inputs from the extracted feature ``feat`` [2n, C, H, W] (rows 0..n-1: the unlabelled
    images, rows n..2n-1: their transformed copies): ``cat(feat1, feat2)`` and ``cat(feat1, roll(feat2))`` of
    mineestimator.py:33-35 with ``feat2 = flip(feat[:n])`` of _mixins.py:79-82, one launch each way (spcl_mine_pairs_*)."""

    @staticmethod
    def forward(ctx, feat, flags, dtype):
        _n.require_gpu(feat)
        if feat.dim() != 4 or feat.shape[0] < 2 or feat.shape[0] % 2:
            raise ValueError(f"mine_pairs: a feature of 2n samples [2n, C, H, W], got {tuple(feat.shape)}")
        N2, C, H, W = feat.shape
        n = N2 // 2
        flags = _flip_flags_arg(flags, n, feat.device)
        xs = to_nhwc_padded(feat.detach(), dtype)
        c2s = _ru16(2 * C)
        joint = torch.empty(n, H, W, c2s, dtype=dtype, device=feat.device)
        marg = torch.empty(n, H, W, c2s, dtype=dtype, device=feat.device)
        _n.call("spcl_mine_pairs_forward", _n.ptr(xs), _n.ptr(flags), _n.dtype_code(dtype), n, H, W, C, _n.ptr(joint),
                _n.ptr(marg), _n.stream())
        ctx.flags = flags
        ctx.meta = (n, C, H, W, xs.shape[3], dtype, feat.dtype)
        return nhwc_to_logical(joint, 2 * C), nhwc_to_logical(marg, 2 * C)

    @staticmethod
    def backward(ctx, dj, dm):
        n, C, H, W, cs, dtype, xdt = ctx.meta
        djs, dms = to_nhwc_padded(dj, dtype), to_nhwc_padded(dm, dtype)
        dfeat = torch.empty(2 * n, H, W, cs, dtype=dtype, device=dj.device)
        _n.call("spcl_mine_pairs_backward", _n.ptr(djs), _n.ptr(dms), _n.ptr(ctx.flags), _n.dtype_code(dtype), n, H, W, C,
                _n.ptr(dfeat), _n.stream())
        g = nhwc_to_logical(dfeat, C)
        return (g if g.dtype == xdt else g.to(xdt)), None, None


def _mine_dtype(dtype):
    if dtype is None:
        from . import config as _config
        dtype = _config.get_compute_dtype()
    return dtype


def mine_pairs(feat, flags=None, dtype=None):
    """-> (joint, marg), logical [n, 2C, H, W] views over NHWC storage of the compute dtype; ``flags``: uint8 [n] or None"""
    return _MinePairsFn.apply(feat, flags, _mine_dtype(dtype))


class _MineHeadFn(torch.autograd.Function):
    """``AdaptiveMaxPool2d((1, 1)) -> Flatten -> Linear(C / 2, 1)`` of the two passes' stored activations and
    ``softplus(t_marg).mean() + softplus(t_joint).mean()`` (mineestimator.py:27-29,34-36) in one launch; the backward, one
    launch too, writes the two dense activation gradients the BatchNorm-ReLU backward of ``conv_bn_relu`` consumes.
    ``dead``: parameters that cannot move the loss (the convolution biases in front of a training-mode BatchNorm): their
    gradient is exact zeros rather than None."""

    @staticmethod
    def forward(ctx, act_j, act_m, lw, lb, dtype, out, *dead):
        _n.require_gpu(act_j, act_m, lw, lb)
        if act_j.dim() != 4 or act_j.shape != act_m.shape:
            raise ValueError(f"mine_head: two activations of one shape [n, C/2, H, W], got {tuple(act_j.shape)} and "
                             f"{tuple(act_m.shape)}")
        n, CH, H, W = act_j.shape
        if lw.numel() != CH or lb.numel() != 1:
            raise ValueError(f"mine_head: Linear({CH}, 1), got a weight {tuple(lw.shape)} and a bias {tuple(lb.shape)}")
        dev = act_j.device
        aj, am = to_nhwc_padded(act_j.detach(), dtype), to_nhwc_padded(act_m.detach(), dtype)
        w = lw.detach().reshape(-1).contiguous().float()
        b = lb.detach().reshape(1).contiguous().float()
        t = torch.empty(2, n, dtype=torch.float32, device=dev)
        mx = torch.empty(2, n, CH, dtype=torch.float32, device=dev)
        arg = torch.empty(2, n, CH, dtype=torch.int32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        nbytes = _n.call("spcl_mine_head_workspace_bytes", n, H, W, 2 * CH)
        if nbytes == 0:
            raise ValueError(f"mine_head: at most 256 pooled channels and a map below 2^24 pixels (got {CH}, {H} x {W})")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _n.call("spcl_mine_head_forward", _n.ptr(aj), _n.ptr(am), _n.dtype_code(dtype), n, H, W, 2 * CH, _n.ptr(w), _n.ptr(b),
                _n.ptr(t), _n.ptr(mx), _n.ptr(arg), _n.ptr(loss), _n.ptr(ws), nbytes, _n.stream())
        if out is not None:
            out.update(t=t, maxima=mx, argmax=arg)
        ctx.save_for_backward(t, mx, arg, w)
        ctx.params = (lw, lb)
        ctx.dead = tuple((tuple(d.shape), d.numel()) for d in dead)
        ctx.meta = (n, CH, H, W, aj.shape[3], dtype, act_j.dtype)
        return loss

    @staticmethod
    def backward(ctx, g):
        t, mx, arg, w = ctx.saved_tensors
        n, CH, H, W, cs, dtype, adt = ctx.meta
        lw, lb = ctx.params
        dev = t.device
        ng = ctx.needs_input_grad
        grad = None if is_unit_gradient(g) else g.detach().float().reshape(1).contiguous()
        dj = torch.empty(n, H, W, cs, dtype=dtype, device=dev)
        dm = torch.empty(n, H, W, cs, dtype=dtype, device=dev)
        dw = _grad_buffer(take_grad_sink(lw, ng[2]), (CH,), dev) if ng[2] else None
        db = _grad_buffer(take_grad_sink(lb, ng[3]), (1,), dev) if ng[3] else None
        _n.call("spcl_mine_head_backward", _n.ptr(t), _n.ptr(mx), _n.ptr(arg), _n.ptr(w), _n.ptr(grad), _n.dtype_code(dtype), n,
                H, W, 2 * CH, _n.ptr(dj), _n.ptr(dm), _n.ptr(dw), _n.ptr(db), _n.stream())
        gj, gm = nhwc_to_logical(dj, CH), nhwc_to_logical(dm, CH)
        if adt != dtype:
            gj, gm = gj.to(adt), gm.to(adt)
        zeros, at = [], 0
        if ctx.dead:
            flat = torch.zeros(sum(k for _, k in ctx.dead), dtype=torch.float32, device=dev)
            for i, (shape, k) in enumerate(ctx.dead):
                zeros.append(flat[at:at + k].view(shape) if ng[6 + i] else None)
                at += k
        return (gj if ng[0] else None, gm if ng[1] else None, None if dw is None else dw.view(lw.shape),
                None if db is None else db.view(lb.shape), None, None, *zeros)


def mine_head(act_joint, act_marg, weight, bias, dtype=None, dead=(), out=None):
    """-> ``Em - Ej`` (0-dim f32).  ``out``: a dict that receives the logits ``t`` [2, n], the pooled ``maxima`` [2, n, C/2] and
    their ``argmax`` [2, n, C/2] (pass 0 is the joint one)"""
    return _MineHeadFn.apply(act_joint, act_marg, weight, bias, _mine_dtype(dtype), out, *dead)


class MineBN:
    """one ``nn.BatchNorm2d`` of the statistics network as the kernels see it"""
    __slots__ = ("running_mean", "running_var", "num_batches_tracked", "training", "track", "momentum", "eps")

    def __init__(self, running_mean, running_var, num_batches_tracked, training, track, momentum, eps):
        self.running_mean, self.running_var, self.num_batches_tracked = running_mean, running_var, num_batches_tracked
        self.training, self.track, self.momentum, self.eps = bool(training), bool(track), float(momentum), float(eps)


def _mine_layer(x, w, b, gamma, beta, bn: MineBN, dtype):
    """``Conv2d(., ., 3, 1, 1)`` WITH bias -> BatchNorm2d -> ReLU.  With batch statistics the bias cancels in the
    normalisation, so the kernels never see it; only the running mean does (``+= momentum * bias``, what tracking the biased
    output would have added).  With running statistics the bias moves into the BatchNorm shift: normalising ``conv + b`` with
    mean ``m`` is normalising ``conv`` with mean ``m - b``."""
    rm, rv, nbt = bn.running_mean, bn.running_var, bn.num_batches_tracked
    if not bn.training:
        rm = rm.float() - b.detach().float()
    cfg = BlockCfg(dtype, bn.training, bn.momentum, bn.eps, (bn.track,), True, False, False, ((rm, rv, nbt),))
    act = conv_bn_relu(x, w, gamma, beta, cfg)
    if bn.training and bn.track:
        with torch.no_grad():
            bn.running_mean.add_(b.detach().to(bn.running_mean.dtype), alpha=bn.momentum)
    return act


def mine_loss(feat, flags, layers, linear, dtype=None, out=None):
    """``MineEstimator.forward`` (mineestimator.py:32-36) on the extracted feature ``feat`` [2n, C, H, W] and the batch's flip
    flags: ``Em - Ej``.  ``layers``: two tuples ``(conv weight, conv bias, bn weight, bn bias, MineBN)``; ``linear``:
    ``(weight [1, C/2], bias [1])``.  The joint pass runs first, each pass with its own batch statistics."""
    dtype = _mine_dtype(dtype)
    joint, marg = mine_pairs(feat, flags, dtype)
    dtc, (H, W) = _n.dtype_code(dtype), feat.shape[2:]
    packed = [_pack_both(layer[0], dtc, dtype) for layer in layers]  # once: both passes use the same weights
    acts = []
    for x in (joint, marg):
        for (w, b, gamma, beta, bn), pk in zip(layers, packed):
            _PREPACKED[(w.data_ptr(), w._version, dtc, int(H), int(W))] = pk  # (consumed by the call below: take_prepacked)
            x = _mine_layer(x, w, b, gamma, beta, bn, dtype)
        acts.append(x)
    dead = tuple(b for _, b, _, _, bn in layers if bn.training and b.requires_grad)
    return mine_head(acts[0], acts[1], linear[0], linear[1], dtype, dead=dead, out=out)
