"""Fused RAdam over one flat fp32 parameter (``ddp.FlatParams.param``): the optimizer step of the pre-train
iteration as ONE HIP streaming kernel (+ a one-thread coefficient kernel, or -- in a staged step, whose host-written bytes
travel to the device anyway -- four coefficients computed on the host) instead of torch's ~40 foreach launches.

Semantics are ``torch.optim.RAdam(lr, betas, eps, weight_decay, decoupled_weight_decay=False)`` (the reference builds
its RAdam from the un-vendored deepclustering2, ``contrastyou/trainer/base.py:62``; SURVEY.md section 8c fixes torch's as
the restatement).  The step counter and the learning rate live on the device, so a captured hipGraph replays
correctly; ``param_groups[i]["lr"]`` stays an ordinary float that LR schedulers may rewrite: it is pushed to the
device at every eager ``step()`` and by ``sync_lr()`` (call that between graph replays after a scheduler step).

``FusedAdam``, ``FusedAdamW`` and ``FusedSGD`` are the other names ``config["Optim"]["name"]`` may carry (the reference builds
``optim.__dict__[name]``, ``contrastyou/trainer/base.py:60-69``) with the semantics of ``torch.optim.Adam`` / ``AdamW`` / ``SGD``,
built the same way; all four share ``FusedOptimizer``'s protocol (``step(scalar_adds=, grad_scale=, stage=)``, ``sync_lr``,
``forget_staged_steps``), which is what the epochers test for before they capture the step, fold the data-parallel mean into
the update and let the meters ride in the optimizer's launch."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import native as _n

_STAGED_COEF = os.environ.get("SPCL_RADAM_STAGED", "1") != "0"  # A/B switch: 0 keeps the coefficient launch in staged steps


def _ipow(b: float, e: int) -> float:
    """b ** e by repeated squaring, multiplication by multiplication what csrc/optim.hip ipow does (same bits)"""
    r = 1.0
    while e > 0:
        if e & 1:
            r *= b
        b *= b
        e >>= 1
    return r


def radam_coefficients(t: int, lr: float, beta1: float, beta2: float):
    """the step's three scalars (csrc/optim.hip radam_tick_kernel, torch.optim.RAdam's formulas, in double) + t; every
    operation is an IEEE double operation in the kernel's order: the floats are the kernel's, bit for bit"""
    lr = float(np.float32(lr))  # (the kernel reads the learning rate from a float32 device scalar)
    b1t, b2t = _ipow(beta1, t), _ipow(beta2, t)
    bc1, bc2 = 1.0 - b1t, 1.0 - b2t
    rho_inf = 2.0 / (1.0 - beta2) - 1.0
    rho_t = rho_inf - 2.0 * t * b2t / bc2
    if rho_t > 5.0:
        rect = math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t))
        return [lr / bc1, rect * math.sqrt(bc2), 1.0, float(t)]
    return [lr / bc1, 0.0, 0.0, float(t)]


def adam_coefficients(t: int, lr: float, beta1: float, beta2: float, weight_decay: float = 0.0, decoupled: bool = False):
    """the step's scalars of Adam / AdamW (csrc/optim.hip adam_tick_kernel; torch/optim/adam.py _single_tensor_adam's step_size,
    bias_correction2_sqrt and -- decoupled -- the factor of ``param.mul_(1 - lr * weight_decay)``) + t, operation by operation
    what the kernel computes in double.  The kernel writes the decay factor whether or not the decay is decoupled (it is only
    read when it is), so ``decoupled`` does not change the values."""
    lr = float(np.float32(lr))  # (the kernel reads the learning rate from a float32 device scalar)
    bc1, bc2 = 1.0 - _ipow(beta1, t), 1.0 - _ipow(beta2, t)
    return [lr / bc1, math.sqrt(bc2), 1.0 - lr * weight_decay, float(t)]


def sgd_coefficients(t: int, lr: float):
    """SGD has no bias correction: the learning rate as the float32 the device holds, and t (csrc/optim.hip sgd_tick_kernel)"""
    return [float(np.float32(lr)), 0.0, 0.0, float(t)]


class FusedOptimizer(torch.optim.Optimizer):
    """What the four fused optimizers share: the device-resident ``step`` / ``lr_dev`` / ``coef`` scalars beside torch's state
    keys, the staged step's host mirror of the step count, and ``step()``'s protocol.  A subclass names its f32 state tensors
    (``_moments``), computes a step's four floats on the host (``_coefficients``) and issues its two entry points (``_launch``)."""
    _tag = None      # key of this class's stage slots
    _moments = ()    # the per-parameter f32 state tensors, torch's names

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        name = type(self).__name__
        for group in self.param_groups:
            for p in group["params"]:
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise TypeError(f"{name} takes contiguous fp32 parameters (use ddp.FlatParams)")
                _n.require_gpu(p)
        self._step_host = {}  # id(p) -> host mirror of the device step counter while staged steps run (absent: unknown)

    def _moments_of(self, group):
        return self._moments

    def _state(self, p, group):
        st = self.state[p]
        if not st:
            st["step"] = torch.zeros((), dtype=torch.int64, device=p.device)
            for k in self._moments_of(group):
                st[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["lr_dev"] = torch.full((), float(group["lr"]), dtype=torch.float32, device=p.device)
            st["lr_host"] = float(group["lr"])
            st["coef"] = torch.zeros(4, dtype=torch.float32, device=p.device)
        return st

    def _coefficients(self, t, group):
        raise NotImplementedError

    def _launch(self, p, g, st, group, grad_scale, coef, adds):
        """``coef``: the staged step's four floats on the device, or None for the eager entry (``st["lr_dev"]`` / ``st["coef"]``)"""
        raise NotImplementedError

    def _staged_coef(self, p, group):
        """fill function of this parameter's stage slot: called once per staged step (stepgraph.StepStage.begin / bind)"""
        if id(p) not in self._step_host:
            self._step_host[id(p)] = int(self.state[p]["step"].item())  # (one readback: the first staged step, or after eager steps)
        t = self._step_host[id(p)] = self._step_host[id(p)] + 1
        if t >= 1 << 24:
            raise OverflowError(f"{type(self).__name__}: staged step count beyond 2^24 (the count travels as a float)")
        return self._coefficients(t, group)

    def forget_staged_steps(self):
        """drop the host mirrors of the step counts: a staged step whose update launch did not happen left them one ahead of
        the device counters (``_staged_coef`` advances at fill time); the next staged step reads the device's counts back"""
        self._step_host.clear()

    @torch.no_grad()
    def sync_lr(self):
        """push the groups' current learning rates to the device (outside graph capture)."""
        for group in self.param_groups:
            for p in group["params"]:
                st = self._state(p, group)
                if st["lr_host"] != float(group["lr"]):
                    st["lr_dev"].fill_(float(group["lr"]))
                    st["lr_host"] = float(group["lr"])

    @torch.no_grad()
    def step(self, closure=None, scalar_adds=None, grad_scale: float = 1.0, stage=None):
        """``scalar_adds``: what ``contrastyou.meters.take_batch()`` returned -- the step's meter updates, performed by
        the first parameter's coefficient launch (one launch less per step).  ``grad_scale``: the update uses
        ``grad_scale * p.grad`` (ddp.FlatParams hands over the ranks' gradient SUM and 1 / world: the mean costs no pass
        of its own); 1.0 is the exact identity.  ``stage``: the epocher's ``stepgraph.StepStage`` while a staged step
        runs -- the step's scalar coefficients are then computed on the host from ``param_groups[i]["lr"]`` and a host
        mirror of the step count, and ride in the stage's upload (no coefficient launch, no ``sync_lr``)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = torch.cuda.is_current_stream_capturing()
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if g.dtype != torch.float32 or not g.is_contiguous():
                    raise TypeError(f"{type(self).__name__} needs a contiguous fp32 gradient")
                st = self._state(p, group)
                if not capturing and st["lr_host"] != float(group["lr"]):  # None after load_state_dict
                    st["lr_dev"].fill_(float(group["lr"]))
                    st["lr_host"] = float(group["lr"])
                adds = (0, None, None, None)
                if scalar_adds is not None:
                    src, dst, cnt, k = scalar_adds[:4]
                    adds = (k, src, dst, cnt)
                    scalar_adds = None
                if _STAGED_COEF and stage is not None and stage.active:
                    coef = stage.bind((self._tag, id(p)), 4, "f32", lambda b, p=p, group=group: self._staged_coef(p, group))
                    self._launch(p, g, st, group, float(grad_scale), coef, adds)
                    continue
                self._step_host.pop(id(p), None)  # (the device counter advances by itself below)
                self._launch(p, g, st, group, float(grad_scale), None, adds)
        if scalar_adds is not None:  # no parameter was stepped: the adds still have to happen
            _n.call("spcl_accumulate_scalars", scalar_adds[3], scalar_adds[0], scalar_adds[1], scalar_adds[2], _n.stream())
        return loss

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:  # torch casts floating state to the parameter's dtype/device; restore ours
            for p in group["params"]:
                st = self.state.get(p)
                if st:
                    st["step"] = st["step"].to(device=p.device, dtype=torch.int64)
                    for k in ("lr_dev", "coef") + tuple(self._moments_of(group)):
                        st[k] = st[k].to(device=p.device, dtype=torch.float32)
                    st["lr_host"] = None  # force a push of the group's lr at the next eager step
        self._step_host = {}


def is_fused(optimizer) -> bool:
    """True for the optimizers whose step is the product's (``FusedOptimizer``): the epochers then capture the step in a
    hipGraph, fold the data-parallel mean into the update and hand the meters' adds to the optimizer's launch.  An object
    built from ``torch.optim`` directly is not, and stays on the eager path."""
    return isinstance(optimizer, FusedOptimizer)


class FusedRAdam(FusedOptimizer):
    _tag = "radam"
    _moments = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError("invalid RAdam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _coefficients(self, t, group):
        b1, b2 = group["betas"]
        return radam_coefficients(t, float(group["lr"]), float(b1), float(b2))

    def _launch(self, p, g, st, group, grad_scale, coef, adds):
        b1, b2 = group["betas"]
        k, src, dst, cnt = adds
        if coef is not None:
            _n.call("spcl_radam_apply_staged", _n.ptr(p), _n.ptr(g), grad_scale, _n.ptr(st["exp_avg"]),
                    _n.ptr(st["exp_avg_sq"]), p.numel(), _n.ptr(st["step"]), _n.ptr(coef), float(b1), float(b2),
                    float(group["eps"]), float(group["weight_decay"]), k, src, dst, cnt, _n.stream())
        else:
            _n.call("spcl_radam_step_scaled", _n.ptr(p), _n.ptr(g), grad_scale, _n.ptr(st["exp_avg"]),
                    _n.ptr(st["exp_avg_sq"]), p.numel(), _n.ptr(st["step"]), _n.ptr(st["lr_dev"]), float(b1), float(b2),
                    float(group["eps"]), float(group["weight_decay"]), _n.ptr(st["coef"]), k, src, dst, cnt, _n.stream())


class FusedAdam(FusedOptimizer):
    """``torch.optim.Adam(lr, betas, eps, weight_decay, decoupled_weight_decay)`` (single-tensor path, amsgrad = maximize =
    False) as one streaming HIP kernel: csrc/optim.hip adam_apply_kernel"""
    _tag = "adam"
    _moments = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      decoupled_weight_decay=bool(decoupled_weight_decay)))

    def _coefficients(self, t, group):
        b1, b2 = group["betas"]
        return adam_coefficients(t, float(group["lr"]), float(b1), float(b2), float(group["weight_decay"]),
                                 bool(group["decoupled_weight_decay"]))

    def _launch(self, p, g, st, group, grad_scale, coef, adds):
        b1, b2 = group["betas"]
        k, src, dst, cnt = adds
        dec = int(bool(group["decoupled_weight_decay"]))
        if coef is not None:
            _n.call("spcl_adam_apply_staged", _n.ptr(p), _n.ptr(g), grad_scale, _n.ptr(st["exp_avg"]),
                    _n.ptr(st["exp_avg_sq"]), p.numel(), _n.ptr(st["step"]), _n.ptr(coef), float(b1), float(b2),
                    float(group["eps"]), float(group["weight_decay"]), dec, k, src, dst, cnt, _n.stream())
        else:
            _n.call("spcl_adam_step_scaled", _n.ptr(p), _n.ptr(g), grad_scale, _n.ptr(st["exp_avg"]),
                    _n.ptr(st["exp_avg_sq"]), p.numel(), _n.ptr(st["step"]), _n.ptr(st["lr_dev"]), float(b1), float(b2),
                    float(group["eps"]), float(group["weight_decay"]), dec, _n.ptr(st["coef"]), k, src, dst, cnt,
                    _n.stream())


class FusedAdamW(FusedAdam):
    """``torch.optim.AdamW``: Adam with the decoupled decay and torch's default ``weight_decay=1e-2``"""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=True)


class FusedSGD(FusedOptimizer):
    """``torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov)`` as one streaming HIP kernel (csrc/optim.hip
    sgd_apply_kernel).  ``momentum_buffer`` exists only with a momentum; whether a step is the first (``buf = grad``) is
    decided on the device, from the step counter."""
    _tag = "sgd"

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=bool(nesterov)))

    def _moments_of(self, group):
        return ("momentum_buffer",) if group["momentum"] != 0 else ()

    def _coefficients(self, t, group):
        return sgd_coefficients(t, float(group["lr"]))

    def _launch(self, p, g, st, group, grad_scale, coef, adds):
        k, src, dst, cnt = adds
        buf = _n.ptr(st.get("momentum_buffer"))
        hyper = (float(group["momentum"]), float(group["dampening"]), float(group["weight_decay"]), int(group["nesterov"]))
        if coef is not None:
            _n.call("spcl_sgd_apply_staged", _n.ptr(p), _n.ptr(g), grad_scale, buf, p.numel(), _n.ptr(st["step"]),
                    _n.ptr(coef), *hyper, k, src, dst, cnt, _n.stream())
        else:
            _n.call("spcl_sgd_step_scaled", _n.ptr(p), _n.ptr(g), grad_scale, buf, p.numel(), _n.ptr(st["step"]),
                    _n.ptr(st["lr_dev"]), *hyper, _n.ptr(st["coef"]), k, src, dst, cnt, _n.stream())
