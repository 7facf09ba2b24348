"""The update step of training on the package's own kernels (csrc/optim.hip): ``clip_grad_norm_`` and ``SGD``.

The reference's ``train_impl`` ends every mini-batch with ``nn.utils.clip_grad_norm_(net.parameters(), 1000)`` and
``optimizer.step()`` of a ``torch.optim.SGD``.  Both are here as multi-tensor HIP launches with torch's arithmetic, one fp32
rounding per operation (include/yv3.h states it; tests/optim_ref.py restates it in numpy), and the norm summed in fp64 in a
fixed order: repeated steps give identical bits.  ``SGD`` keeps torch's optimizer contract -- param groups, ``state_dict``
(interchangeable with ``torch.optim.SGD`` in both directions), hooks, ``torch.optim.lr_scheduler`` -- and adds
``step_clipped(max_norm)``, which applies the clip coefficient inside the update instead of rewriting the gradients.

Everything runs on the current stream of the parameters' device, without a device-to-host read; the only allocations are the
workspace (sized by the first call, grown when a later call has more chunks) and the momentum buffers of a parameter's first step.
The workspace is per device: calls on one device are meant to come from one stream at a time.

Parameters and gradients must be fp32, contiguous and on one GPU: anything else raises ``TypeError`` -- dtype and layout at
construction already, the device at ``step()`` -- before any launch.
"""
import ctypes

import torch

from . import _ffi

CHUNK = 16384             # elements per workgroup: YV3_OPTIM_CHUNK of include/yv3.h (yv3_optim_chunk() returns it)
_SGD_FIRST, _SGD_NESTEROV, _SGD_MAXIMIZE = 1, 2, 4

_workspaces = {}          # device index -> _Workspace


class _Workspace:
    def __init__(self, device):
        self.device = device
        self.partials = None
        self.out = torch.zeros(2, dtype=torch.float32, device=device)        # total_norm, coef

    def partials_for(self, chunks):
        if self.partials is None or self.partials.numel() < chunks:
            self.partials = torch.empty(max(chunks, 1), dtype=torch.float64, device=self.device)
        return self.partials


def _workspace(device):
    ws = _workspaces.get(device.index)
    if ws is None:
        ws = _workspaces[device.index] = _Workspace(device)
    return ws


def _check(t, what, device=None, need_gpu=True):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a tensor, got %s" % (what, type(t).__name__))
    if (need_gpu and not t.is_cuda) or t.layout != torch.strided:
        raise TypeError("%s must be a dense GPU tensor (device %s, layout %s): the update kernels run on the GPU only"
                        % (what, t.device, t.layout))
    if t.dtype != torch.float32:
        raise TypeError("%s must be fp32, got %s" % (what, t.dtype))
    if not t.is_contiguous():
        raise TypeError("%s must be contiguous (shape %s, strides %s)" % (what, tuple(t.shape), t.stride()))
    if device is not None and t.device != device:
        raise TypeError("%s is on %s, its parameter on %s" % (what, t.device, device))


def _with_grads(params):
    """The (p, g) pairs an update touches -- requires_grad, a .grad, at least one element -- checked; and their one device."""
    pairs, device = [], None
    for p in params:
        if not p.requires_grad or p.grad is None:
            continue
        _check(p, "a parameter")
        g = p.grad
        _check(g, "a gradient", p.device)
        if g.numel() != p.numel():
            raise TypeError("a gradient of %d elements for a parameter of %d" % (g.numel(), p.numel()))
        if device is None:
            device = p.device
        elif p.device != device:
            raise TypeError("parameters on %s and %s: one update runs on one GPU" % (device, p.device))
        if p.numel():
            pairs.append((p, g))
    return pairs, device


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _sizes(tensors):
    return (ctypes.c_longlong * len(tensors))(*[t.numel() for t in tensors])


def _norm_and_coef(grads, max_norm, device):
    """Enqueues sum of squares + clip coefficient of `grads`; returns the workspace (out[0] = total_norm, out[1] = coef)."""
    lib, s, ws = _ffi.lib(), _ffi.stream_ptr(), _workspace(device)
    n = _sizes(grads)
    chunks = sum((k + CHUNK - 1) // CHUNK for k in n)
    part = ws.partials_for(chunks)
    _ffi.check(lib.yv3_grad_sumsq(_ptrs(grads), n, len(grads), part.data_ptr(), part.numel(), s), "yv3_grad_sumsq")
    _ffi.check(lib.yv3_clip_coef(part.data_ptr(), chunks, float(max_norm), ws.out.data_ptr(), s), "yv3_clip_coef")
    return ws


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_`` for the 2-norm: scales every ``.grad`` in place by
    ``min(max_norm / (total_norm + 1e-6), 1)`` and returns ``total_norm`` as a 0-dim fp32 GPU tensor, without synchronising.
    ``total_norm`` is ``fp32(sqrt(sum of g^2 in fp64))`` (torch sums in fp32).  Parameters without a ``.grad`` (or that do not
    require one) are skipped; an empty set returns 0 (on the CPU: there is no device to ask).  The returned tensor is a view of
    the per-device workspace, valid until the next clip or ``step_clipped`` on that device: ``clone()`` it to keep it.
    ``foreach`` is accepted and ignored; ``error_if_nonfinite`` would need a device-to-host read and is not supported."""
    if float(norm_type) != 2.0:
        raise ValueError("only the 2-norm is supported (norm_type=%r)" % (norm_type,))
    if error_if_nonfinite:
        raise NotImplementedError("error_if_nonfinite needs a device-to-host read: test torch.isfinite(total_norm) yourself")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    pairs, device = _with_grads(list(parameters))
    if not pairs:
        return torch.tensor(0.0)
    grads = [g for _, g in pairs]
    with torch.cuda.device(device):
        ws = _norm_and_coef(grads, max_norm, device)
        _ffi.check(_ffi.lib().yv3_grad_scale(_ptrs(grads), _sizes(grads), len(grads), ws.out.data_ptr() + 4, _ffi.stream_ptr()),
                   "yv3_grad_scale")
    torch.autograd.graph.increment_version(grads)
    return ws.out[0]


class SGD(torch.optim.Optimizer):
    """``torch.optim.SGD`` on the package's kernels: the same constructor, ``defaults``, param groups and state
    (``momentum_buffer`` per parameter, created by the parameter's first step with momentum), so ``state_dict()`` /
    ``load_state_dict()`` interchange with torch's and ``torch.optim.lr_scheduler`` works (hyper-parameters are read from
    ``param_groups`` at every step).  ``foreach``, ``differentiable`` and ``fused`` are accepted and ignored.  One launch per block
    of 64 tensors with the same hyper-parameters.  Every written parameter's ``_version`` moves, so the inference engine and the
    training path re-pack their weights."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None):
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if lr < 0.0:
            raise ValueError("Invalid learning rate: %s" % (lr,))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: %s" % (momentum,))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: %s" % (weight_decay,))
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused)
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, defaults)
        self._total_norm = None

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("nesterov", False)
            group.setdefault("maximize", False)
            group.setdefault("foreach", None)
            group.setdefault("differentiable", False)
            group.setdefault("fused", None)
        self.__dict__.setdefault("_total_norm", None)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:           # (the device is checked by step(): a net may move to the GPU later)
            _check(p, "a parameter", need_gpu=False)

    def step(self, closure=None, *, max_norm=None):
        """One update of every parameter that requires grad and has a ``.grad``.  With ``max_norm``, the gradients' clip coefficient
        is computed first and applied inside the update (see ``step_clipped``)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._total_norm = self._update(max_norm)
        return loss

    def step_clipped(self, max_norm):
        """``clip_grad_norm_(all parameters, max_norm)`` and ``step()`` in one pass over the gradients: parameters and momentum buffers
        get the bits of the two separate calls, but the coefficient is applied while the update reads ``g``, so ``.grad`` IS LEFT
        UNSCALED (the two calls leave ``g * coef`` there).  Returns ``total_norm`` like ``clip_grad_norm_``."""
        self.step(max_norm=max_norm)
        return self._total_norm

    @torch.no_grad()
    def _update(self, max_norm):
        # everything is checked before the first launch
        work, device, everything = [], None, []
        for group in self.param_groups:
            pairs, dev = _with_grads(group["params"])
            if not pairs:
                continue
            if device is None:
                device = dev
            elif dev != device:
                raise TypeError("parameters on %s and %s: one update runs on one GPU" % (device, dev))
            momentum = float(group["momentum"])
            first, later = [], []
            for p, g in pairs:
                buf = self.state.get(p, {}).get("momentum_buffer") if momentum != 0 else None      # (no state entry made by looking)
                if buf is not None:
                    _check(buf, "a momentum buffer", p.device)
                    if buf.numel() != p.numel():
                        raise TypeError("a momentum buffer of %d elements for a parameter of %d" % (buf.numel(), p.numel()))
                (later if buf is not None else first).append((p, g, buf))
            flags = (_SGD_NESTEROV if group["nesterov"] else 0) | (_SGD_MAXIMIZE if group["maximize"] else 0)
            hyper = (float(group["lr"]), momentum, 1.0 - float(group["dampening"]), float(group["weight_decay"]))
            for entries, first_step in ((first, True), (later, False)):
                if entries:
                    work.append((entries, hyper, flags | (_SGD_FIRST if first_step and momentum != 0 else 0)))
                    everything += entries
        if not everything:
            return torch.tensor(0.0) if max_norm is not None else None
        lib = _ffi.lib()
        with torch.cuda.device(device):
            s, coef, total_norm = _ffi.stream_ptr(), None, None
            if max_norm is not None:
                ws = _norm_and_coef([g for _, g, _ in everything], max_norm, device)
                coef, total_norm = ws.out.data_ptr() + 4, ws.out[0]
            written = []
            for entries, (lr, momentum, omd, wd), flags in work:
                ps, gs = [p for p, _, _ in entries], [g for _, g, _ in entries]
                bufs = None
                if momentum != 0:
                    if flags & _SGD_FIRST:
                        bufs = [torch.empty_like(p, memory_format=torch.contiguous_format) for p in ps]
                        for p, b in zip(ps, bufs):
                            self.state[p]["momentum_buffer"] = b
                    else:
                        bufs = [b for _, _, b in entries]
                    written += bufs
                _ffi.check(lib.yv3_sgd_step(_ptrs(ps), _ptrs(gs), _ptrs(bufs) if bufs else None, _sizes(ps), len(ps), coef,
                                            lr, momentum, omd, wd, flags, s), "yv3_sgd_step")
                written += ps
        torch.autograd.graph.increment_version(written)
        return total_norm
