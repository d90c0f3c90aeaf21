"""The trainer's optimizer tail on the HIP kernels (csrc/mzgo_optim.hip,
``mzgo_optim_step``): ``clip_grad_norm_``, ``torch.optim.Adam.step`` and
``StepLR.step`` (main.py:481-484, :379) over any list of float32 parameters,
from one stream-ordered call of three launches instead of some two dozen torch
ops.

``DeviceAdam`` is the optimizer (``TrainConfig.device_optimizer``);
``adam_step_host`` runs the same scalar functions serially on numpy arrays (the
formulas' CPU check).  Three things differ from the torch ops on purpose:

* a step whose gradient norm is not finite is refused on the device -- no
  parameter, moment or step count changes -- and counted (``skipped()``);
  ``clip_grad_norm_`` would turn every parameter into NaN;
* the gradients are only read: the clipped values are not written back into
  ``p.grad`` (``clip_grad_norm_`` scales ``.grad`` in place);
* the arithmetic is float64 on the float32 values, rounded once on the store,
  and the norm is a fixed-order float64 sum: the same inputs give the same
  bits.
"""
import ctypes

import numpy as np
import torch

from ._lib import OptimHyper, check, lib, stream_of


def optim_chunk():
    """Elements of one (tensor, chunk) segment of the kernels (``mzgo_optim_chunk``)."""
    return int(lib.mzgo_optim_chunk())


def _hyper(lr, betas, eps, weight_decay, decoupled_weight_decay, max_grad_norm, lr_step_size, lr_gamma):
    return OptimHyper(lr0=float(lr), beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps),
                      weight_decay=float(weight_decay), decoupled=int(bool(decoupled_weight_decay)),
                      max_norm=0.0 if max_grad_norm is None else float(max_grad_norm),
                      step_size=1 if lr_step_size is None else int(lr_step_size),
                      gamma=1.0 if lr_step_size is None else float(lr_gamma))


def _lr(hyper, sched):
    out = ctypes.c_double()
    check(lib.mzgo_optim_lr(ctypes.byref(hyper), int(sched), ctypes.byref(out)))
    return out.value


def _table(addresses):
    return (ctypes.c_void_p * len(addresses))(*addresses)


class _Handle:
    """A ``mzgo_optim`` (destroyed with the last reference to it)."""

    def __init__(self, numels, device_index):
        self.opt = ctypes.c_void_p()
        check(lib.mzgo_optim_create(len(numels), (ctypes.c_int64 * len(numels))(*numels), device_index,
                                    ctypes.byref(self.opt)))

    def __del__(self):
        opt, self.opt = getattr(self, "opt", None), None
        if opt:
            lib.mzgo_optim_destroy(opt)


class _DeviceBlob:
    """Device memory of the library as ``__cuda_array_interface__`` (keeps its owner alive)."""

    def __init__(self, address, shape, typestr, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (address, False), "version": 2,
                                         "strides": None}


class DeviceAdam:
    """Adam / AdamW with gradient-norm clipping and a StepLR schedule, one HIP
    call per step.

    ``params``: contiguous float32 CUDA tensors on one device (any module's;
    nothing here knows the network).  ``max_grad_norm`` None (or <= 0) means no
    clipping; ``lr_step_size`` None a constant rate.  ``weight_decay`` is
    Adam's classic decay (added to the gradient) or, with
    ``decoupled_weight_decay``, AdamW's.

    ``step()`` enqueues the call on the current stream and synchronises
    nothing; a parameter whose ``.grad`` is None is left out (norm, update and
    step count), as torch leaves it out.  ``p.grad`` is only read.  A step with
    a non-finite gradient norm changes nothing but the scheduler count and the
    skipped-step count.  ``record`` is the device's f64 [4] record of the
    latest step -- norm, clip coefficient, learning rate, applied (1 / 0)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 decoupled_weight_decay=False, max_grad_norm=None, lr_step_size=None, lr_gamma=1.0):
        self.params = list(params)
        if not self.params:
            raise ValueError("DeviceAdam got an empty parameter list")
        dev = self.params[0].device
        for i, p in enumerate(self.params):
            if not isinstance(p, torch.Tensor) or p.device.type != "cuda" or p.dtype != torch.float32:
                raise ValueError(f"DeviceAdam takes float32 CUDA tensors: parameter {i} is "
                                 f"{getattr(p, 'dtype', type(p).__name__)} on {getattr(p, 'device', 'the host')} "
                                 "(there is no eager fall-back)")
            if p.device != dev:
                raise ValueError(f"DeviceAdam takes parameters on one device: parameter {i} is on {p.device}, "
                                 f"parameter 0 on {dev}")
            if not p.is_contiguous():
                raise ValueError(f"DeviceAdam takes contiguous parameters: parameter {i} has strides {p.stride()}")
        self.device = dev
        self.hyper = _hyper(lr, betas, eps, weight_decay, decoupled_weight_decay, max_grad_norm, lr_step_size,
                            lr_gamma)
        _lr(self.hyper, 0)                                # (refuses a step_size < 1 here, not at the first step)
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        self._handle = _Handle([p.numel() for p in self.params], dev.index or 0)
        self._opt = self._handle.opt
        self._sched = 0                                   # host mirror of the device's scheduler count
        self._moments()
        rec = ctypes.c_void_p()
        check(lib.mzgo_optim_record(self._opt, ctypes.byref(rec)))
        self._record = torch.as_tensor(_DeviceBlob(rec.value, (4,), "<f8", self._handle), device=dev)

    def _moments(self):
        self._m_table = _table([t.data_ptr() for t in self.exp_avg])
        self._v_table = _table([t.data_ptr() for t in self.exp_avg_sq])

    # -- the step -------------------------------------------------------------
    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def step(self):
        grads = []
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None:
                grads.append(None)
                continue
            if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape or not g.is_contiguous():
                raise ValueError(f"DeviceAdam.step: the gradient of parameter {i} must be a contiguous float32 "
                                 f"tensor of shape {tuple(p.shape)} on {p.device}, got {g.dtype} "
                                 f"{tuple(g.shape)} strides {g.stride()} on {g.device}")
            grads.append(g.data_ptr())
        with torch.cuda.device(self.device):
            check(lib.mzgo_optim_step(self._opt, _table([p.data_ptr() for p in self.params]), _table(grads),
                                      self._m_table, self._v_table, ctypes.byref(self.hyper),
                                      stream_of(self.device)))
        self._sched += 1
        # the kernels wrote the parameters behind autograd's back: bump their
        # version counters, which is what MuZeroNet._version() reads to tell a
        # stale engine from a current one
        torch.autograd.graph.increment_version(self.params)

    @property
    def lr(self):
        """The learning rate of the next step (after ``step()``: what
        ``param_groups[0]["lr"]`` holds once StepLR has stepped), from the
        host's copy of the scheduler count; does not read the device."""
        return _lr(self.hyper, self._sched)

    @property
    def record(self):
        """CUDA f64 [4]: norm, clip coefficient, learning rate, applied (1 / 0)
        of the latest step.  A view of the optimizer's device memory, valid in
        stream order; reading it here does not synchronise."""
        return self._record

    def counts(self):
        """(step counts int64 [n], scheduler count, skipped steps); synchronises."""
        n = len(self.params)
        steps = np.zeros(n, np.int64)
        sched, skipped = ctypes.c_int64(), ctypes.c_int64()
        with torch.cuda.device(self.device):
            check(lib.mzgo_optim_counts(self._opt, steps.ctypes.data_as(ctypes.c_void_p), ctypes.byref(sched),
                                        ctypes.byref(skipped), stream_of(self.device)))
        return steps, sched.value, skipped.value

    def skipped(self):
        """Steps refused so far for a non-finite gradient norm; synchronises."""
        return self.counts()[2]

    # -- checkpoints ------------------------------------------------------------
    def state_dict(self):
        """``torch.optim.Adam.state_dict()``'s layout -- ``state[i]`` = ``step``
        (a float32 scalar on the host, as torch keeps it), ``exp_avg``,
        ``exp_avg_sq`` (clones) for every parameter that has stepped, and one
        ``param_groups`` entry -- plus ``"schedule"``: the scheduler count and
        the skipped-step count.  ``torch.optim.Adam.load_state_dict`` takes it
        as it is.  Synchronises (the counts come from the device)."""
        steps, sched, skipped = self.counts()
        h = self.hyper
        state = {i: {"step": torch.tensor(float(s), dtype=torch.float32), "exp_avg": self.exp_avg[i].clone(),
                     "exp_avg_sq": self.exp_avg_sq[i].clone()} for i, s in enumerate(steps) if s > 0}
        group = {"lr": _lr(h, sched), "betas": (h.beta1, h.beta2), "eps": h.eps, "weight_decay": h.weight_decay,
                 "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                 "fused": None, "decoupled_weight_decay": bool(h.decoupled), "initial_lr": h.lr0,
                 "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group], "schedule": {"count": sched, "skipped": skipped}}

    def load_state_dict(self, sd):
        """A ``DeviceAdam`` or ``torch.optim.Adam`` state_dict: the moments and
        step counts, and the group's betas, eps and weight decay.  With a
        ``"schedule"`` entry the rate resumes as ``initial_lr`` (else ``lr``)
        decayed by the stored count; without one (a torch checkpoint) the
        schedule restarts from the group's current ``lr``.  Synchronises."""
        groups = sd["param_groups"]
        n = len(self.params)
        if len(groups) != 1 or list(groups[0]["params"]) != list(range(n)):
            raise ValueError(f"DeviceAdam.load_state_dict: expected one param group over parameters 0..{n - 1}")
        g = groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("DeviceAdam has no amsgrad and no maximize")
        sched = sd.get("schedule")
        h = self.hyper
        new = OptimHyper(lr0=float(g.get("initial_lr", g["lr"]) if sched is not None else g["lr"]),
                         beta1=float(g["betas"][0]), beta2=float(g["betas"][1]), eps=float(g["eps"]),
                         weight_decay=float(g["weight_decay"]),
                         decoupled=int(bool(g.get("decoupled_weight_decay", False))), max_norm=h.max_norm,
                         step_size=h.step_size, gamma=h.gamma)
        steps = np.zeros(n, np.int64)
        for i in range(n):
            st = sd["state"].get(i)
            if st is None:
                self.exp_avg[i].zero_()
                self.exp_avg_sq[i].zero_()
                continue
            for name, mine in (("exp_avg", self.exp_avg[i]), ("exp_avg_sq", self.exp_avg_sq[i])):
                if tuple(st[name].shape) != tuple(mine.shape):
                    raise ValueError(f"DeviceAdam.load_state_dict: state[{i}][{name!r}] has shape "
                                     f"{tuple(st[name].shape)}, the parameter {tuple(mine.shape)}")
                mine.copy_(st[name])
            steps[i] = int(round(float(st["step"])))
        count = int(sched["count"]) if sched is not None else 0
        skipped = int(sched.get("skipped", 0)) if sched is not None else 0
        with torch.cuda.device(self.device):
            check(lib.mzgo_optim_set_counts(self._opt, steps.ctypes.data_as(ctypes.c_void_p), count, skipped,
                                            stream_of(self.device)))
        self.hyper = new
        self._sched = count


def adam_step_host(params, grads, exp_avg, exp_avg_sq, steps, *, sched=0, skipped=0, lr=1e-3, betas=(0.9, 0.999),
                   eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False, max_grad_norm=None, lr_step_size=None,
                   lr_gamma=1.0):
    """``mzgo_optim_step_host``: one ``DeviceAdam.step()`` on numpy arrays, by
    the kernels' scalar functions with their chunking and summation orders.
    ``params`` / ``exp_avg`` / ``exp_avg_sq`` are lists of float32 arrays,
    ``grads`` the same with None for a tensor without gradient, ``steps`` the
    step counts.  Nothing is changed in place; returns ``(params, exp_avg,
    exp_avg_sq, steps, sched, skipped, record)`` after the step, ``record`` the
    f64 [4] norm, clip coefficient, learning rate, applied.  Needs no GPU."""
    n = len(params)
    if not (len(grads) == len(exp_avg) == len(exp_avg_sq) == len(steps) == n):
        raise ValueError("adam_step_host: params, grads, exp_avg, exp_avg_sq and steps must have one entry per tensor")
    f32 = lambda x: np.array(x, dtype=np.float32, order="C")          # (a copy)
    p, m, v = [f32(x) for x in params], [f32(x) for x in exp_avg], [f32(x) for x in exp_avg_sq]
    g = [None if x is None else np.ascontiguousarray(x, dtype=np.float32) for x in grads]
    for i in range(n):
        for name, a in (("grads", g[i]), ("exp_avg", m[i]), ("exp_avg_sq", v[i])):
            if a is not None and a.shape != p[i].shape:
                raise ValueError(f"adam_step_host: {name}[{i}] has shape {a.shape}, params[{i}] {p[i].shape}")
    addr = lambda xs: _table([None if x is None else x.ctypes.data for x in xs])
    numels = (ctypes.c_int64 * max(n, 1))(*(x.size for x in p))
    st = np.array(steps, dtype=np.int64)
    c_sched, c_skipped = ctypes.c_int64(int(sched)), ctypes.c_int64(int(skipped))
    record = np.zeros(4, np.float64)
    hyper = _hyper(lr, betas, eps, weight_decay, decoupled_weight_decay, max_grad_norm, lr_step_size, lr_gamma)
    check(lib.mzgo_optim_step_host(n, numels, addr(p), addr(g), addr(m), addr(v), ctypes.byref(hyper),
                                   st.ctypes.data_as(ctypes.c_void_p), ctypes.byref(c_sched), ctypes.byref(c_skipped),
                                   record.ctypes.data_as(ctypes.c_void_p)))
    return p, m, v, st, c_sched.value, c_skipped.value, record
