"""The update step of training on the package's own kernels (csrc/optim.hip): ``clip_grad_norm_``, ``SGD``, ``Adam`` and ``AdamW``.

The reference's ``train_impl`` ends every mini-batch with ``nn.utils.clip_grad_norm_(net.parameters(), 1000)`` and
``optimizer.step()`` of a ``torch.optim.SGD``.  Both are here as multi-tensor HIP launches with torch's arithmetic, one fp32
rounding per operation (include/yv3.h states it; tests/optim_ref.py restates it in numpy), and the norm summed in fp64 in a
fixed order: repeated steps give identical bits.  ``SGD`` keeps torch's optimizer contract -- param groups, ``state_dict``
(interchangeable with ``torch.optim.SGD`` in both directions), hooks, ``torch.optim.lr_scheduler`` -- and adds
``step_clipped(max_norm)``, which applies the clip coefficient inside the update instead of rewriting the gradients.  ``Adam`` and
``AdamW`` do the same for ``torch.optim.Adam`` / ``AdamW`` (tests/adam_ref.py is their definition).

Everything runs on the current stream of the parameters' device, without a device-to-host read; the only allocations are the
workspace (sized by the first call, grown when a later call has more chunks) and the state tensors of a parameter's first step.
The workspace is per device: calls on one device are meant to come from one stream at a time.

Parameters and gradients must be fp32, contiguous and on one GPU: anything else raises ``TypeError`` -- dtype and layout at
construction already, the device at ``step()`` -- before any launch.
"""
import ctypes

import torch

from . import _ffi

CHUNK = 16384             # elements per workgroup: YV3_OPTIM_CHUNK of include/yv3.h (yv3_optim_chunk() returns it)
_SGD_FIRST, _SGD_NESTEROV, _SGD_MAXIMIZE = 1, 2, 4
_ADAM_FIRST, _ADAM_AMSGRAD, _ADAM_MAXIMIZE, _ADAM_DECOUPLED = 1, 2, 4, 8
_ADAM_STATE = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")

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


def _check_state(t, what, p):
    """A per-parameter state tensor the kernels read and write: as its parameter, element for element."""
    _check(t, what, p.device)
    if t.numel() != p.numel():
        raise TypeError("%s of %d elements for a parameter of %d" % (what, t.numel(), p.numel()))


def _grouped(param_groups):
    """[(group, its (p, g) pairs)] for the groups that have any, and the one device of them all."""
    out, device = [], None
    for group in param_groups:
        pairs, dev = _with_grads(group["params"])
        if not pairs:
            continue
        if device is None:
            device = dev
        elif dev != device:
            raise TypeError("parameters on %s and %s: one update runs on one GPU" % (device, dev))
        out.append((group, pairs))
    return out, device


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
        work, everything = [], []
        grouped, device = _grouped(self.param_groups)
        for group, pairs in grouped:
            momentum = float(group["momentum"])
            first, later = [], []
            for p, g in pairs:
                buf = self.state.get(p, {}).get("momentum_buffer") if momentum != 0 else None      # (no state entry made by looking)
                if buf is not None:
                    _check_state(buf, "a momentum buffer", p)
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


def _refuse_device_reads(lr, betas, capturable):
    """What would need a device-to-host read at every step."""
    if capturable:
        raise ValueError("capturable=True keeps `step` on the GPU; the bias corrections are computed on the host here")
    if isinstance(betas[0], torch.Tensor) or isinstance(betas[1], torch.Tensor):
        raise ValueError("tensor betas are not supported: pass floats")
    if isinstance(lr, torch.Tensor):
        if lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if lr.device.type != "cpu":
            raise ValueError("a tensor lr on %s would be read back at every step: pass a float or a CPU tensor" % (lr.device,))


def _adam_hyper(group):
    """A param group's hyper-parameters as host numbers: (lr, beta1, beta2, eps, weight_decay, amsgrad, maximize, decoupled)."""
    _refuse_device_reads(group["lr"], group["betas"], group.get("capturable"))
    return (float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
            float(group["weight_decay"]), bool(group["amsgrad"]), bool(group["maximize"]), bool(group["decoupled_weight_decay"]))


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam`` on the package's kernels: the same constructor, ``defaults``, param groups and per-parameter state
    (``step`` as a 0-dim fp32 CPU tensor, ``exp_avg``, ``exp_avg_sq``, ``max_exp_avg_sq`` with amsgrad; created by the parameter's
    first step, uninitialised: that step does not read them), so ``state_dict()`` / ``load_state_dict()`` interchange with torch's
    and ``torch.optim.lr_scheduler`` works (hyper-parameters are read from ``param_groups`` at every step).  The arithmetic is
    torch's single-tensor path, one fp32 rounding per operation (include/yv3.h).  ``foreach``, ``differentiable`` and ``fused``
    are accepted and ignored; ``capturable=True``, a tensor ``lr`` on the GPU, tensor betas and a ``step`` state on the GPU are
    refused, since each would need a device-to-host read at every step.  ``load_state_dict`` brings ``step`` to the CPU (one read
    per load), so checkpoints of torch's ``fused=True`` Adam load, and a group that carries ``fused=True`` resumes from its own.  Parameters are bucketed by
    (hyper-parameters, step count, first step or not) -- the bias corrections depend on the step -- with one launch per block of
    64 tensors of a bucket.  ``step_clipped`` and ``max_norm`` are those of ``SGD``."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        _refuse_device_reads(lr, betas, capturable)                # (before the range checks: they would read a GPU lr)
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %s" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %s" % (eps,))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: %s" % (betas[0],))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: %s" % (betas[1],))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %s" % (weight_decay,))
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)
        self._total_norm = None

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("amsgrad", False)
            group.setdefault("maximize", False)
            group.setdefault("foreach", None)
            group.setdefault("capturable", False)
            group.setdefault("differentiable", False)
            group.setdefault("fused", None)
            group.setdefault("decoupled_weight_decay", False)
            for p in group["params"]:
                st = self.state.get(p, {})
                if len(st) == 0:
                    continue
                if not torch.is_tensor(st["step"]):
                    st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
                elif st["step"].device.type != "cpu":       # torch's fused layout, or load_state_dict's cast under fused=True
                    st["step"] = st["step"].to("cpu", torch.float32)
        self.__dict__.setdefault("_total_norm", None)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        _adam_hyper(self.param_groups[-1])
        for p in self.param_groups[-1]["params"]:           # (the device is checked by step(): a net may move to the GPU later)
            _check(p, "a parameter", need_gpu=False)

    def step(self, closure=None, *, max_norm=None):
        """One update of every parameter that requires grad and has a ``.grad``; only their ``step`` moves.  With ``max_norm``, the
        gradients' clip coefficient is computed first and applied inside the update (see ``step_clipped``)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._total_norm = self._update(max_norm)
        return loss

    def step_clipped(self, max_norm):
        """``clip_grad_norm_(all parameters, max_norm)`` and ``step()`` in one pass over the gradients: parameters and state get the
        bits of the two separate calls, but the coefficient is applied while the update reads ``g``, so ``.grad`` IS LEFT UNSCALED
        (the two calls leave ``g * coef`` there).  Returns ``total_norm`` like ``clip_grad_norm_``."""
        self.step(max_norm=max_norm)
        return self._total_norm

    @torch.no_grad()
    def _update(self, max_norm):
        # everything is checked before the first launch and before any state is made or moved
        buckets, everything = {}, []
        hypers = {id(group): _adam_hyper(group) for group in self.param_groups}
        grouped, device = _grouped(self.param_groups)
        for group, pairs in grouped:
            hyper = hypers[id(group)]
            amsgrad = hyper[5]
            for p, g in pairs:
                st = self.state.get(p)                      # (no state entry made by looking)
                if not st:
                    now, entry = 1.0, (p, g, None, None, None)
                else:
                    step = st["step"]
                    if not isinstance(step, torch.Tensor) or step.numel() != 1:
                        raise TypeError("the `step` state must be a 1-element tensor, got %r" % (step,))
                    if step.device.type != "cpu":
                        raise TypeError("a `step` state on %s (torch's capturable / fused layout) would be read back at every step: "
                                        "move it to the CPU" % (step.device,))
                    now = step.item() + 1.0                 # (a CPU tensor: no device read)
                    for name in _ADAM_STATE if amsgrad else _ADAM_STATE[:2]:
                        if name not in st:
                            raise TypeError("a parameter's state lacks %s" % name)
                        _check_state(st[name], name, p)
                    entry = (p, g, st["exp_avg"], st["exp_avg_sq"], st["max_exp_avg_sq"] if amsgrad else None)
                buckets.setdefault((hyper, now, not st), []).append(entry)
                everything.append(entry)
        if not everything:
            return torch.tensor(0.0) if max_norm is not None else None
        lib = _ffi.lib()
        with torch.cuda.device(device):
            s, coef, total_norm = _ffi.stream_ptr(), None, None
            if max_norm is not None:
                ws = _norm_and_coef([e[1] for e in everything], max_norm, device)
                coef, total_norm = ws.out.data_ptr() + 4, ws.out[0]
            written = []
            for ((lr, beta1, beta2, eps, wd, amsgrad, maximize, decoupled), now, first), entries in buckets.items():
                ps, gs = [e[0] for e in entries], [e[1] for e in entries]
                if first:
                    for p in ps:
                        st = self.state[p]
                        st["step"] = torch.tensor(0.0, dtype=torch.float32)
                        st["exp_avg"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                        st["exp_avg_sq"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                        if amsgrad:
                            st["max_exp_avg_sq"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                states = [self.state[p] for p in ps]
                for st in states:
                    st["step"].fill_(now)                   # step + 1, rounded to the tensor's dtype as `step += 1` rounds it
                ms, vs = [st["exp_avg"] for st in states], [st["exp_avg_sq"] for st in states]
                xs = [st["max_exp_avg_sq"] for st in states] if amsgrad else None
                bc1, bc2 = 1 - beta1 ** now, 1 - beta2 ** now
                flags = (_ADAM_FIRST if first else 0) | (_ADAM_AMSGRAD if amsgrad else 0) | (_ADAM_MAXIMIZE if maximize else 0)
                decay = 0.0
                if wd != 0:
                    decay = 1 - lr * wd if decoupled else wd
                    flags |= _ADAM_DECOUPLED if decoupled else 0
                _ffi.check(lib.yv3_adam_step(_ptrs(ps), _ptrs(gs), _ptrs(ms), _ptrs(vs), _ptrs(xs) if xs else None, _sizes(ps), len(ps),
                                             coef, 1 - beta1, beta2, 1 - beta2, bc2 ** 0.5, eps, -(lr / bc1), decay, flags, s),
                           "yv3_adam_step")
                written += ps + ms + vs + (xs or [])
        torch.autograd.graph.increment_version(written)
        return total_norm


class AdamW(Adam):
    """``torch.optim.AdamW``: ``Adam`` with ``decoupled_weight_decay=True`` and torch's default ``weight_decay=1e-2``."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=True)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group["decoupled_weight_decay"] = True
