"""The trainer's whole unroll as ONE autograd node on the HIP kernels
(csrc/mzgo_unroll.hip, ``mzgo_unroll_forward`` / ``mzgo_unroll_backward``):
main.py:431-482's representation, K dynamics steps and the heads of all K + 1
latents for B samples from one forward call (K + 5 launches enqueued from
C++) and one backward call (K + 17), instead of some forty torch ops per
unroll step with their autograd nodes.

``unroll`` is differentiable in the net's 22 parameters only (there is no
observation gradient); with ``return_latents`` it also returns the K + 1
latents and takes a gradient with respect to them, which is how an auxiliary
loss (``mzgo.ownership``, ``mzgo.consistency``) attaches to the fused step;
``encode`` is the representation alone, without a gradient (the consistency
loss's targets); ``unroll_heads_host``
runs the heads' scalar functions serially on host arrays (the formulas' CPU
check).
"""
import ctypes

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from ._lib import check, lib, ptr, stream_of
from .net import MuZeroNet

HEAD_KEYS = ("dynamics.reward_conv.weight", "dynamics.reward_conv.bias", "dynamics.fc_reward_hidden.weight",
             "dynamics.fc_reward_hidden.bias", "dynamics.fc_reward_output.weight", "dynamics.fc_reward_output.bias",
             "prediction.pass_logit", "prediction.value_conv.weight", "prediction.value_conv.bias",
             "prediction.value_fc.weight", "prediction.value_fc.bias", "prediction.policy_conv.weight",
             "prediction.policy_conv.bias")

PRECISIONS = {"fp32": 0, "bf16": 1}      # mzgo.h: MZGO_PREC_F32, MZGO_PREC_BF16

_sizes = {}      # (B, K, C, N, emb_rows, precision) -> (saved_bytes, work_bytes)


def _precision(precision):
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be 'fp32' or 'bf16', got {precision!r}")
    return PRECISIONS[precision]


def workspace_bytes(B, K, C, N, emb_rows, precision="fp32"):
    """``mzgo_unroll_workspace_p``: (saved_bytes, work_bytes) of a call's two device buffers."""
    key = (B, K, C, N, emb_rows, precision)
    if key not in _sizes:
        saved, work = ctypes.c_int64(), ctypes.c_int64()
        check(lib.mzgo_unroll_workspace_p(B, K, C, N, emb_rows, _precision(precision), ctypes.byref(saved),
                                          ctypes.byref(work)))
        _sizes[key] = (saved.value, work.value)
    return _sizes[key]


class _Table:
    """The key / shape half of a parameter table (``mzgo_set_weights_device``'s
    convention): built once per set of names and shapes."""

    def __init__(self, names, shapes):
        n = self.n = len(names)
        self.keys = (ctypes.c_char_p * n)(*(k.encode() for k in names))
        self._shape = [(ctypes.c_int64 * max(len(s), 1))(*s) for s in shapes]
        self.shapes = (ctypes.POINTER(ctypes.c_int64) * n)(
            *(ctypes.cast(s, ctypes.POINTER(ctypes.c_int64)) for s in self._shape))
        self.ndims = (ctypes.c_int * n)(*(len(s) for s in shapes))

    def pointers(self, arrays):
        """The data half: a pointer per entry (None -> NULL); tensors give ``data_ptr()``."""
        return (ctypes.c_void_p * self.n)(*(None if a is None else a.data_ptr() if isinstance(a, torch.Tensor)
                                            else a.ctypes.data for a in arrays))


_tables = {}     # (latent_dim, embedding rows) -> (the net's table, its parameter names)


def _net_table(net):
    key = (net.latent_dim, net.max_action_size)
    if key not in _tables:
        names = [k for k, _ in net.named_parameters()]
        _tables[key] = (_Table(names, [tuple(p.shape) for p in net.parameters()]), names)
    return _tables[key]


_latents = {}    # (B, K, C, N, emb_rows, precision) -> (offset_bytes, bytes) of the latents inside ``saved``


def latents_span(B, K, C, N, emb_rows, precision="fp32"):
    """``mzgo_unroll_latents``: (offset_bytes, bytes) of the step-major latents inside a call's ``saved``."""
    key = (B, K, C, N, emb_rows, precision)
    if key not in _latents:
        off, size = ctypes.c_int64(), ctypes.c_int64()
        check(lib.mzgo_unroll_latents(B, K, C, N, emb_rows, _precision(precision), ctypes.byref(off),
                                      ctypes.byref(size)))
        _latents[key] = (off.value, size.value)
    return _latents[key]


class _Unroll(torch.autograd.Function):
    @staticmethod
    def forward(ctx, obs0, acts, table, names, dims, precision, return_latents, *params):
        B, K, C, N, emb_rows = dims
        dev = obs0.device
        A = N * N + 1
        saved_bytes, _ = workspace_bytes(*dims, precision)
        saved = torch.empty(saved_bytes, dtype=torch.uint8, device=dev)
        logits = torch.empty(K + 1, B, A, device=dev)
        value = torch.empty(K + 1, B, device=dev)
        reward = torch.empty(K, B, device=dev) if K > 0 else None
        data = [p.detach() for p in params]
        with torch.cuda.device(dev):
            check(lib.mzgo_unroll_forward_p(table.keys, table.pointers(data), table.shapes, table.ndims, table.n,
                                            ptr(obs0), ptr(acts) if K > 0 else None, B, K, C, N, emb_rows,
                                            ptr(saved), saved_bytes, ptr(logits), ptr(value), ptr(reward),
                                            PRECISIONS[precision], stream_of(dev)))
        ctx.save_for_backward(saved, *params)
        ctx.table, ctx.names, ctx.dims, ctx.precision = table, names, dims, precision
        ctx.return_latents = return_latents
        out = (logits, value) if K == 0 else (logits, value, reward)
        if return_latents:
            # a view of ``saved``, no copy: the backward reads the same memory, and autograd's version counter
            # (shared by a view and its base) turns an in-place write into an error at backward() instead of
            # wrong gradients.  A gradient that never arrives stays None (-> NULL), not a tensor of zeros.
            ctx.set_materialize_grads(False)
            off, size = latents_span(*dims, precision)
            out += (saved[off:off + size].view(torch.float32).view(K + 1, B, C, N, N),)
        return out

    @staticmethod
    @once_differentiable                 # the HIP backward builds no graph: create_graph=True is an error, not silence
    def backward(ctx, *g_out):
        saved, *params = ctx.saved_tensors
        g_out = list(g_out)
        g_latent = g_out.pop() if ctx.return_latents else None
        g_logits, g_value = g_out[0], g_out[1]
        g_reward = g_out[2] if len(g_out) > 2 else None
        table, names, dims, precision = ctx.table, ctx.names, ctx.dims, ctx.precision
        B, K, C, N, emb_rows = dims
        dev = saved.device
        A = N * N + 1
        saved_bytes, work_bytes = workspace_bytes(*dims, precision)

        def grad(g, *shape):
            if g is None:
                return torch.zeros(*shape, device=dev)
            return g.to(torch.float32).contiguous()

        g_logits, g_value = grad(g_logits, K + 1, B, A), grad(g_value, K + 1, B)
        g_reward = grad(g_reward, K, B) if K > 0 else None
        if g_latent is not None:
            g_latent = g_latent.to(torch.float32).contiguous()
            if g_latent.data_ptr() % 16:             # (a slice of a larger tensor: the add kernel loads float4)
                g_latent = g_latent.clone()
        work = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
        # at K = 0 the dynamics take no part: no gradient, as autograd gives
        grads = [None if K == 0 and k.startswith("dynamics.") else torch.empty_like(p) for k, p in zip(names, params)]
        data = [p.detach() for p in params]
        with torch.cuda.device(dev):
            if g_latent is None:         # (mzgo_unroll_backward_l with NULL: the same call)
                check(lib.mzgo_unroll_backward_p(table.keys, table.pointers(data), table.shapes, table.ndims,
                                                 table.pointers(grads), table.n, ptr(saved), saved_bytes,
                                                 ptr(g_logits), ptr(g_value), ptr(g_reward), B, K, C, N, emb_rows,
                                                 ptr(work), work_bytes, PRECISIONS[precision], stream_of(dev)))
            else:
                check(lib.mzgo_unroll_backward_l(table.keys, table.pointers(data), table.shapes, table.ndims,
                                                 table.pointers(grads), table.n, ptr(saved), saved_bytes,
                                                 ptr(g_logits), ptr(g_value), ptr(g_reward), ptr(g_latent), B, K, C, N,
                                                 emb_rows, ptr(work), work_bytes, PRECISIONS[precision],
                                                 stream_of(dev)))
        return (None, None, None, None, None, None, None, *grads)


def bf16_round_host(x):
    """``mzgo_bf16_round_host``: float32 -> bfloat16 round-to-nearest-even, returned as float32
    (``t.bfloat16().float()``), by the function the bf16 kernels round with.  A numpy array in, one out."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    check(lib.mzgo_bf16_round_host(ptr(x), x.size, ptr(out)))
    return out


def unroll(net, obs0, acts, precision="fp32", return_latents=False):
    """The K-step unroll of ``net`` (a ``MuZeroNet`` on the GPU) from the
    observations ``obs0`` f32 [B, 6, N, N] under the actions ``acts`` i64
    [B, K] (``device_targets``' layout; None or [B, 0] for K = 0), values in
    0 .. the embedding's rows - 1 (not checked: that would synchronise).
    Returns the heads' outputs stacked step-major, as ``unroll_loss`` takes
    them: ``(logits [K+1, B, A], value [K+1, B], reward [K, B] or None)``.

    One autograd node over the net's 22 parameters: the forward is one
    ``mzgo_unroll_forward`` call, the backward one ``mzgo_unroll_backward``
    call; a net whose embedding is larger than the board (``board_size=``)
    gets a full-size embedding gradient.  Each call owns its buffers, so calls
    may overlap freely.  Device tensors only: there is no eager fall-back.

    ``precision="bf16"`` runs the dynamics conv's three matrix products --
    forward, input gradient and weight gradient -- on bf16 MFMA with their
    operands rounded to bfloat16 (nearest even) and float32 accumulation
    (``mzgo_unroll_forward_p`` with ``MZGO_PREC_BF16``, mzgo.h); the weights,
    the latents, every gradient and everything else stay float32.  It needs
    ``latent_dim`` to be a multiple of 32.  Any other string is a ValueError.

    ``return_latents=True`` adds a fourth output, ``latents`` f32 [K+1, B, C, N,
    N]: the K + 1 latents the heads read, step-major, handed out without a copy
    as a view of the call's saved buffer (``mzgo_unroll_latents``; so they must
    not be written in place, which autograd refuses at ``backward()``).
    ``latents`` is differentiable: a gradient that arrives there -- an
    auxiliary loss on the latents, ``mzgo.ownership_loss`` for one -- is added
    to the heads' latent gradient before the chain
    (``mzgo_unroll_backward_l``); when none arrives the backward is the call it
    is without the flag, bit for bit."""
    from .resnet import ResMuZeroNet
    _precision(precision)
    if isinstance(net, ResMuZeroNet):
        raise TypeError("mzgo.unroll runs the reference network (MuZeroNet) only: ResMuZeroNet's residual tower has "
                        "no fused unroll kernels")
    if not isinstance(net, MuZeroNet):
        raise TypeError(f"mzgo.unroll needs a MuZeroNet, got {type(net).__name__}")
    if precision == "bf16" and net.latent_dim % 32:
        raise ValueError(f"mzgo.unroll: precision='bf16' needs latent_dim to be a multiple of 32, got "
                         f"{net.latent_dim}")
    params = list(net.parameters())
    dev = params[0].device
    if dev.type != "cuda":
        raise ValueError("mzgo.unroll runs on the GPU: call net.to('cuda') first")
    N, C = net.board_size, net.latent_dim
    if C < 16 or C % 16:
        raise ValueError(f"mzgo.unroll needs latent_dim to be a multiple of 16, got {C}")
    if not isinstance(obs0, torch.Tensor) or obs0.device != dev:
        raise ValueError(f"mzgo.unroll: obs0 must be a tensor on {dev} (the net's device)")
    if obs0.ndim != 4 or tuple(obs0.shape[1:]) != (6, N, N):
        raise ValueError(f"obs0 must be [B, 6, {N}, {N}], got {tuple(obs0.shape)}")
    B = obs0.shape[0]
    if acts is None or acts.shape[-1] == 0:
        K, acts = 0, None
    else:
        if acts.device != dev:
            raise ValueError(f"mzgo.unroll: acts is on {acts.device}, the net on {dev}")
        if acts.ndim != 2 or acts.shape[0] != B:
            raise ValueError(f"acts must be [B = {B}, K], got {tuple(acts.shape)}")
        K = acts.shape[1]
        acts = acts.to(torch.int64).contiguous()
    for k, p in net.named_parameters():
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError(f"mzgo.unroll: parameter '{k}' must be contiguous float32")
    table, names = _net_table(net)
    obs0 = obs0.detach().to(torch.float32).contiguous()
    out = _Unroll.apply(obs0, acts, table, names, (B, K, C, N, net.max_action_size), precision, bool(return_latents),
                        *params)
    heads = (out[0], out[1], out[2] if K > 0 else None)
    return heads + (out[-1],) if return_latents else heads


_encode_work = {}    # (B, C, N) -> mzgo_encode_workspace bytes


def encode(net, obs):
    """The representation alone: ``obs`` f32 [B', 6, N, N] -> latents f32 [B',
    C, N, N] by the fused unroll's three representation convs
    (``mzgo_encode``): the bits of ``unroll(net, obs, None,
    return_latents=True)``'s latents, without the heads and the saved buffer
    that call carries.  Not differentiable: the result never requires grad,
    whatever the grad mode (the consistency loss's targets carry no gradient).
    Any B' >= 1 (past the convs' grid limit of 65535 boards the call runs them
    in chunks).  ``unroll``'s checks: a ``MuZeroNet`` on the GPU, ``latent_dim``
    a multiple of 16.  Stream-ordered; device tensors only."""
    from .resnet import ResMuZeroNet
    if isinstance(net, ResMuZeroNet):
        raise TypeError("mzgo.encode runs the reference network (MuZeroNet) only: ResMuZeroNet's residual tower has "
                        "no fused unroll kernels")
    if not isinstance(net, MuZeroNet):
        raise TypeError(f"mzgo.encode needs a MuZeroNet, got {type(net).__name__}")
    params = list(net.parameters())
    dev = params[0].device
    if dev.type != "cuda":
        raise ValueError("mzgo.encode runs on the GPU: call net.to('cuda') first")
    N, C = net.board_size, net.latent_dim
    if C < 16 or C % 16:
        raise ValueError(f"mzgo.encode needs latent_dim to be a multiple of 16, got {C}")
    if not isinstance(obs, torch.Tensor) or obs.device != dev:
        raise ValueError(f"mzgo.encode: obs must be a tensor on {dev} (the net's device)")
    if obs.ndim != 4 or tuple(obs.shape[1:]) != (6, N, N) or obs.shape[0] < 1:
        raise ValueError(f"obs must be [B >= 1, 6, {N}, {N}], got {tuple(obs.shape)}")
    for k, p in net.named_parameters():
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError(f"mzgo.encode: parameter '{k}' must be contiguous float32")
    B = obs.shape[0]
    if (B, C, N) not in _encode_work:
        n = ctypes.c_int64()
        check(lib.mzgo_encode_workspace(B, C, N, ctypes.byref(n)))
        _encode_work[(B, C, N)] = n.value
    nbytes = _encode_work[(B, C, N)]
    table, _ = _net_table(net)
    obs = obs.detach().to(torch.float32).contiguous()
    latents = torch.empty(B, C, N, N, device=dev)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.mzgo_encode(table.keys, table.pointers([p.detach() for p in params]), table.shapes, table.ndims,
                              table.n, ptr(obs), B, C, N, net.max_action_size, ptr(latents), ptr(work), nbytes,
                              stream_of(dev)))
    return latents


def unroll_heads_host(params, latents, g_logits, g_value, g_reward):
    """``mzgo_unroll_heads_host`` on numpy arrays: the heads of ``latents``
    f32 [S, B, C, N, N] (S = K + 1 steps) under ``params`` (the thirteen head
    tensors by state_dict key), forward and backward from the output gradients
    ``g_logits`` [S, B, A], ``g_value`` [S, B], ``g_reward`` [K, B] (None at
    K = 0).  Returns ``(logits, value, reward or None, grads, g_latent)`` with
    ``grads`` a dict over the head keys (the reward head's missing at K = 0)."""
    f32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float32)
    latents, g_logits, g_value, g_reward = map(f32, (latents, g_logits, g_value, g_reward))
    if latents.ndim != 5 or latents.shape[3] != latents.shape[4]:
        raise ValueError(f"latents must be [S, B, C, N, N], got {tuple(latents.shape)}")
    S, B, C, N, _ = latents.shape
    A = N * N + 1
    names = list(params)
    arrays = [f32(params[k]) for k in names]
    table = _Table(names, [a.shape for a in arrays])
    grads = [None if S == 1 and k.startswith("dynamics.") else np.empty_like(a) for k, a in zip(names, arrays)]
    logits = np.empty((S, B, A), np.float32)
    value = np.empty((S, B), np.float32)
    reward = np.empty((S - 1, B), np.float32) if S > 1 else None
    g_latent = np.empty_like(latents)
    check(lib.mzgo_unroll_heads_host(table.keys, table.pointers(arrays), table.shapes, table.ndims,
                                     table.pointers(grads), table.n, ptr(latents), S, B, C, N, ptr(logits), ptr(value),
                                     ptr(reward), ptr(g_logits), ptr(g_value), ptr(g_reward) if S > 1 else None,
                                     ptr(g_latent)))
    return logits, value, reward, {k: g for k, g in zip(names, grads) if g is not None}, g_latent
