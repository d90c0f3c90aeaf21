"""The latent consistency loss (EfficientZero's temporal consistency loss, in
SimSiam's form, on MuZero's unrolled latents): the dynamics' k-th latent
``s_k``, rolled forward from position t under the stored actions, is pulled
towards what the representation gives for the real board at t + k; the target
side carries no gradient.  It is the one training signal that tells the
dynamics what a latent should *be*, not only what its heads should say.

``ConsistencyHead`` is a separate module of two 1x1 convs: ``MuZeroNet`` keeps
the reference's 22 tensors and its ``state_dict``, and the engines, the weight
packers and the search never see the head.  ``consistency_loss`` is the head
and its loss on the HIP kernels (csrc/mzgo_consistency.hip,
``mzgo_consistency_loss`` / ``mzgo_consistency_loss_backward``) as one autograd
node on the latents ``mzgo.unroll(..., return_latents=True)`` returns; the
targets are ``mzgo.encode`` of the store's real boards
(``DeviceReplay.window_obs`` / ``window_obs_from``).
``consistency_loss_host`` runs the same scalar functions serially on host
arrays (the formulas' CPU check).
"""
import ctypes

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from ._lib import check, lib, ptr, stream_of

PROJ_DIMS = (16, 32, 48, 64)
MAX_LATENT_DIM = 256        # csrc/mzgo_consistency.hpp: kConsMaxC (proj's weights are staged in LDS whole)


class ConsistencyHead(nn.Module):
    """``proj = nn.Conv2d(latent_dim, proj_dim, 1)`` and ``pred =
    nn.Conv2d(proj_dim, proj_dim, 1)``, ``proj_dim`` one of 16, 32, 48, 64.
    ``project(x) = proj(x)``, ``predict(z) = pred(relu(z))`` and ``forward(x) =
    predict(project(x))`` are plain torch -- for inspection, the CPU and the
    tests' reference.  Training goes through ``consistency_loss``, which reads
    the two convs' four parameters."""

    def __init__(self, latent_dim, proj_dim=32):
        super().__init__()
        if proj_dim not in PROJ_DIMS:
            raise ValueError(f"proj_dim must be one of {PROJ_DIMS}, got {proj_dim!r}")
        self.latent_dim, self.proj_dim = int(latent_dim), int(proj_dim)
        self.proj = nn.Conv2d(self.latent_dim, self.proj_dim, 1)
        self.pred = nn.Conv2d(self.proj_dim, self.proj_dim, 1)

    def project(self, x):
        return self.proj(x)

    def predict(self, z):
        return self.pred(torch.relu(z))

    def forward(self, x):
        return self.predict(self.project(x))


_work = {}       # (B, K, C, P, N) -> mzgo_consistency_loss_workspace bytes


def _work_bytes(B, K, C, P, N):
    key = (B, K, C, P, N)
    if key not in _work:
        n = ctypes.c_int64()
        check(lib.mzgo_consistency_loss_workspace(B, K, C, P, N, ctypes.byref(n)))
        _work[key] = n.value
    return _work[key]


def _shapes(latents, targets, mask, w1, b1, w2, b2):
    if latents.ndim != 5 or latents.shape[3] != latents.shape[4]:
        raise ValueError(f"latents must be [K+1, B, C, N, N], got {tuple(latents.shape)}")
    K1, B, C, N, _ = latents.shape
    if K1 < 2:
        raise ValueError(f"consistency_loss needs K >= 1 unroll steps (step 0 takes no part), got latents "
                         f"{list(latents.shape)}")
    P = w1.shape[0]
    want = {"targets": (targets, (K1 - 1, B, C, N, N)), "mask": (mask, (B, K1 - 1)),
            "head.proj.weight": (w1, (P, C, 1, 1)), "head.proj.bias": (b1, (P,)),
            "head.pred.weight": (w2, (P, P, 1, 1)), "head.pred.bias": (b2, (P,))}
    for name, (t, shape) in want.items():
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {list(shape)} for latents {list(latents.shape)}, got {list(t.shape)}")
    return B, K1 - 1, C, P, N


class _ConsistencyLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, latents, w1, b1, w2, b2, targets, mask, weight):
        B, K, C, P, N = _shapes(latents, targets, mask, w1, b1, w2, b2)
        dev = latents.device
        lat, wv1, bv1, wv2, bv2, t, m = (x.detach().to(dev, torch.float32).contiguous()
                                         for x in (latents, w1, b1, w2, b2, targets, mask))
        per = torch.empty(B, device=dev)
        total = torch.empty(1, dtype=torch.float64, device=dev)
        nbytes = _work_bytes(B, K, C, P, N)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)     # (what the backward reads stays in it)
        with torch.cuda.device(dev):
            check(lib.mzgo_consistency_loss(ptr(lat), ptr(t), ptr(m), ptr(wv1), ptr(bv1), ptr(wv2), ptr(bv2), B, K, C,
                                            P, N, weight, ptr(per), ptr(total), ptr(work), nbytes, stream_of(dev)))
        ctx.save_for_backward(lat, m, wv1, wv2, work)
        ctx.dims, ctx.weight = (B, K, C, P, N), weight
        ctx.mark_non_differentiable(total)
        return per, total

    @staticmethod
    @once_differentiable
    def backward(ctx, g_per, _g_total):
        lat, m, wv1, wv2, work = ctx.saved_tensors
        B, K, C, P, N = ctx.dims
        dev = lat.device
        g_per = g_per.to(torch.float32).contiguous()
        g_lat = torch.empty_like(lat)
        g_w1, g_b1 = torch.empty(P, C, 1, 1, device=dev), torch.empty(P, device=dev)
        g_w2, g_b2 = torch.empty(P, P, 1, 1, device=dev), torch.empty(P, device=dev)
        with torch.cuda.device(dev):
            check(lib.mzgo_consistency_loss_backward(ptr(lat), ptr(m), ptr(g_per), ptr(wv1), ptr(wv2), B, K, C, P, N,
                                                     ctx.weight, ptr(g_lat), ptr(g_w1), ptr(g_b1), ptr(g_w2),
                                                     ptr(g_b2), ptr(work), work.numel(), stream_of(dev)))
        return g_lat, g_w1, g_b1, g_w2, g_b2, None, None, None


def consistency_loss(latents, targets, mask, head, weight=1.0):
    """The consistency loss of ``head`` (a ``ConsistencyHead``) on the latents
    ``latents`` f32 [K+1, B, C, N, N] (``mzgo.unroll(..., return_latents=True)``'s
    fourth output, taken WHOLE: step 0 takes no part and gets a gradient of
    exact zeros -- a slice ``latents[1:]`` would make autograd zero-fill and
    copy the whole tensor in its backward) against ``targets`` f32 [K, B, C, N,
    N] (``mzgo.encode`` of ``DeviceReplay.window_obs``'s boards) and ``mask``
    f32 [B, K].  For row (k, b), k = 1..K, over the P N N entries: ``u =
    proj(latents[k, b])``, ``p = pred(relu(u))``, ``z = proj(targets[k-1, b])``
    (no gradient flows through z, neither to ``targets`` nor to ``proj``: the
    stop-gradient of SimSiam and EfficientZero), ``cos = <p, z> / (|p| |z|)``
    and ``row = mask[b, k-1] (1 - cos)``; a row with ``|p|`` or ``|z|`` below
    1e-8 has ``cos := 0`` and a gradient of exact zeros.

    Returns ``(per_sample, total)``: ``per_sample[b] = weight * sum_k row`` f32
    [B] (differentiable in ``latents`` and the head's four parameters; any
    weighting over samples) and the f64 [1] total over the samples (not
    differentiable).  Two launches forward, two backward; a masked row is not
    read and contributes exact zeros; repeats give the same bits.  Device
    tensors only: there is no eager fall-back."""
    if not isinstance(head, ConsistencyHead):
        raise TypeError(f"consistency_loss needs a ConsistencyHead, got {type(head).__name__}")
    for name, t in (("latents", latents), ("targets", targets), ("mask", mask),
                    ("head.proj.weight", head.proj.weight), ("head.pred.weight", head.pred.weight)):
        if t.device.type != "cuda":
            raise ValueError(f"consistency_loss runs on the GPU: {name} is on {t.device} (consistency_loss_host "
                             "checks the formulas on host arrays)")
    return _ConsistencyLoss.apply(latents, head.proj.weight, head.proj.bias, head.pred.weight, head.pred.bias,
                                  targets, mask, float(weight))


def consistency_loss_host(latents, targets, mask, proj_w, proj_b, pred_w, pred_b, weight=1.0, g_per=None):
    """``mzgo_consistency_loss_host`` on numpy arrays of ``consistency_loss``'s
    layouts (``proj_w`` [P, C] or the conv's [P, C, 1, 1], ``pred_w`` [P, P] or
    [P, P, 1, 1]): a dict of ``per`` f32 [B], ``total`` (float) and, under the
    incoming ``g_per`` f32 [B] (default: ones), ``g_latents`` [K+1, B, C, N, N],
    ``g_proj_w`` [P, C], ``g_proj_b`` [P], ``g_pred_w`` [P, P] and ``g_pred_b``
    [P]."""
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    latents, targets, mask = f32(latents), f32(targets), f32(mask)
    proj_b, pred_b = f32(proj_b).reshape(-1), f32(pred_b).reshape(-1)
    P = len(proj_b)
    proj_w, pred_w = f32(proj_w).reshape(P, -1), f32(pred_w).reshape(P, -1)
    B, K, C, P, N = _shapes(latents, targets, mask, proj_w.reshape(P, -1, 1, 1), proj_b,
                            pred_w.reshape(P, -1, 1, 1), pred_b)
    g_per = np.ones(B, np.float32) if g_per is None else f32(g_per).reshape(-1)
    if len(g_per) != B:
        raise ValueError(f"g_per must be [{B}], got {list(g_per.shape)}")
    per = np.empty(B, np.float32)
    total = ctypes.c_double()
    g_lat = np.empty_like(latents)
    g_w1, g_b1 = np.empty((P, C), np.float32), np.empty(P, np.float32)
    g_w2, g_b2 = np.empty((P, P), np.float32), np.empty(P, np.float32)
    check(lib.mzgo_consistency_loss_host(ptr(latents), ptr(targets), ptr(mask), ptr(proj_w), ptr(proj_b), ptr(pred_w),
                                         ptr(pred_b), ptr(g_per), B, K, C, P, N, float(weight), ptr(per),
                                         ctypes.byref(total), ptr(g_lat), ptr(g_w1), ptr(g_b1), ptr(g_w2), ptr(g_b2)))
    return dict(per=per, total=total.value, g_latents=g_lat, g_proj_w=g_w1, g_proj_b=g_b1, g_pred_w=g_w2,
                g_pred_b=g_b2)
