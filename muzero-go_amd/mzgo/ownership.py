"""The ownership auxiliary target (KataGo's ownership head, on MuZero's
unrolled latents): a 1x1 conv on every latent of the fused unroll predicts,
for each board point, who owns it on the game's final board, seen from the
colour to move; it is trained next to value, policy and reward and gives the
latents ``s_1..s_K``, which never see a real board, N*N grounded targets each.

``OwnershipHead`` is a separate module: ``MuZeroNet`` keeps the reference's 22
tensors and its ``state_dict``, and the engines, the weight packers and the
search never see the head.  ``ownership_loss`` is the head and its loss on the
HIP kernels (csrc/mzgo_ownership.hip, ``mzgo_ownership_loss`` /
``mzgo_ownership_loss_backward``) as one autograd node on the latents
``mzgo.unroll(..., return_latents=True)`` returns; the targets come from the
store (``DeviceReplay.ownership`` / ``ownership_from``).
``ownership_loss_host`` runs the same scalar functions serially on host arrays
(the formulas' CPU check).
"""
import ctypes

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from ._lib import check, lib, ptr, stream_of


class OwnershipHead(nn.Module):
    """``conv = nn.Conv2d(latent_dim, 1, 1)``; ``forward(latent)`` is the plain
    torch ``tanh(conv(latent))`` in [-1, 1] (+1: the colour to move owns the
    point) -- for inspection, the CPU and the tests' reference.  Training goes
    through ``ownership_loss``, which reads the conv's two parameters."""

    def __init__(self, latent_dim):
        super().__init__()
        self.latent_dim = int(latent_dim)
        self.conv = nn.Conv2d(self.latent_dim, 1, 1)

    def forward(self, latent):
        return torch.tanh(self.conv(latent))


_work = {}       # (B, K, C) -> mzgo_ownership_loss_workspace bytes


def _work_bytes(B, K, C):
    if (B, K, C) not in _work:
        n = ctypes.c_int64()
        check(lib.mzgo_ownership_loss_workspace(B, K, C, ctypes.byref(n)))
        _work[(B, K, C)] = n.value
    return _work[(B, K, C)]


def _shapes(latents, w, bias, t_own, own_mask):
    if latents.ndim != 5 or latents.shape[3] != latents.shape[4]:
        raise ValueError(f"latents must be [K+1, B, C, N, N], got {tuple(latents.shape)}")
    K1, B, C, N, _ = latents.shape
    want = {"head.conv.weight": (w, (1, C, 1, 1)), "head.conv.bias": (bias, (1,)),
            "t_own": (t_own, (B, K1, N * N)), "own_mask": (own_mask, (B, K1))}
    for name, (t, shape) in want.items():
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {list(shape)} for latents {list(latents.shape)}, got {list(t.shape)}")
    return B, K1 - 1, C, N


class _OwnershipLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, latents, w, bias, t_own, own_mask, weight):
        B, K, C, N = _shapes(latents, w, bias, t_own, own_mask)
        dev = latents.device
        lat, wv, bv, t, m = (x.detach().to(dev, torch.float32).contiguous() for x in (latents, w, bias, t_own, own_mask))
        per = torch.empty(B, device=dev)
        total = torch.empty(1, dtype=torch.float64, device=dev)
        g_x = torch.empty(K + 1, B, N * N, device=dev)
        nbytes = _work_bytes(B, K, C)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(lib.mzgo_ownership_loss(ptr(lat), ptr(wv), ptr(bv), ptr(t), ptr(m), B, K, C, N, weight, ptr(per),
                                          ptr(total), ptr(g_x), ptr(work), nbytes, stream_of(dev)))
        ctx.save_for_backward(lat, wv, m, g_x)
        ctx.dims = (B, K, C, N)
        ctx.mark_non_differentiable(total)
        return per, total

    @staticmethod
    @once_differentiable
    def backward(ctx, g_per, _g_total):
        lat, wv, m, g_x = ctx.saved_tensors
        B, K, C, N = ctx.dims
        dev = lat.device
        g_per = g_per.to(torch.float32).contiguous()
        g_lat = torch.empty_like(lat)
        g_w = torch.empty(1, C, 1, 1, device=dev)
        g_b = torch.empty(1, device=dev)
        nbytes = _work_bytes(B, K, C)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(lib.mzgo_ownership_loss_backward(ptr(lat), ptr(wv), ptr(m), ptr(g_x), ptr(g_per), B, K, C, N,
                                                   ptr(g_lat), ptr(g_w), ptr(g_b), ptr(work), nbytes, stream_of(dev)))
        return g_lat, g_w, g_b, None, None, None


def ownership_loss(latents, head, t_own, own_mask, weight=1.0):
    """The ownership loss of ``head`` (an ``OwnershipHead``) on the latents
    ``latents`` f32 [K+1, B, C, N, N] (``mzgo.unroll(..., return_latents=True)``'s
    fourth output) against ``t_own`` f32 [B, K+1, N*N] in {-1, 0, +1} and
    ``own_mask`` f32 [B, K+1] (``DeviceReplay.ownership``).  With the logit
    x = conv(latent) per cell and l(x, t) = softplus(2x) - (1 + t) x -- the
    cross entropy of (1 + tanh x) / 2 against (1 + t) / 2, whose derivative is
    tanh(x) - t -- returns ``(per_sample, total)``: ``per_sample[b] = weight *
    sum_k own_mask[b, k] * mean_c l`` f32 [B] (differentiable in ``latents``,
    ``head.conv.weight`` and ``head.conv.bias``; any weighting over samples)
    and the f64 [1] total over the samples (not differentiable).  Two launches
    forward, two backward; a masked row contributes exact zeros.  Device
    tensors only: there is no eager fall-back."""
    if not isinstance(head, OwnershipHead):
        raise TypeError(f"ownership_loss needs an OwnershipHead, got {type(head).__name__}")
    for name, t in (("latents", latents), ("head.conv.weight", head.conv.weight), ("t_own", t_own),
                    ("own_mask", own_mask)):
        if t.device.type != "cuda":
            raise ValueError(f"ownership_loss runs on the GPU: {name} is on {t.device} (ownership_loss_host checks "
                             "the formulas on host arrays)")
    return _OwnershipLoss.apply(latents, head.conv.weight, head.conv.bias, t_own, own_mask, float(weight))


def ownership_loss_host(latents, w, bias, t_own, own_mask, weight=1.0, g_per=None):
    """``mzgo_ownership_loss_host`` on numpy arrays of ``ownership_loss``'s
    layouts (``w`` [C] or the conv's [1, C, 1, 1], ``bias`` one value): a dict
    of ``per`` f32 [B], ``total`` (float), ``g_x`` f32 [K+1, B, N*N] (the
    derivative of ``per.sum()`` with respect to the logits) and, under the
    incoming ``g_per`` f32 [B] (default: ones), ``g_latents``, ``g_w`` [C] and
    ``g_bias`` [1]."""
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    latents, t_own, own_mask = f32(latents), f32(t_own), f32(own_mask)
    w, bias = f32(w).reshape(-1), f32(bias).reshape(-1)
    B, K, C, N = _shapes(latents, w.reshape(1, -1, 1, 1), bias, t_own, own_mask)
    g_per = np.ones(B, np.float32) if g_per is None else f32(g_per).reshape(-1)
    if len(g_per) != B:
        raise ValueError(f"g_per must be [{B}], got {list(g_per.shape)}")
    per = np.empty(B, np.float32)
    total = ctypes.c_double()
    g_x = np.empty((K + 1, B, N * N), np.float32)
    g_lat, g_w, g_b = np.empty_like(latents), np.empty(C, np.float32), np.empty(1, np.float32)
    check(lib.mzgo_ownership_loss_host(ptr(latents), ptr(w), ptr(bias), ptr(t_own), ptr(own_mask), ptr(g_per), B, K, C,
                                       N, float(weight), ptr(per), ctypes.byref(total), ptr(g_x), ptr(g_lat), ptr(g_w),
                                       ptr(g_b)))
    return dict(per=per, total=total.value, g_x=g_x, g_latents=g_lat, g_w=g_w, g_bias=g_b)
