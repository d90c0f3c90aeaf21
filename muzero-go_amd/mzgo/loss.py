"""The trainer's unroll loss on the HIP kernel (csrc/mzgo_loss.hip,
``mzgo_unroll_loss``): main.py:431-482's value, policy and reward losses of all
K + 1 unroll steps of B samples, and their gradients with respect to the
heads' outputs, from one call instead of some thirty-five torch ops per step.

``unroll_loss`` is differentiable in ``logits``, ``value`` and ``reward``
through ``per_sample``; ``unroll_loss_host`` runs the same scalar functions
serially on host arrays (the formulas' CPU check).
"""
import numpy as np
import torch

from ._lib import check, lib, ptr, stream_of


def _shapes(logits, value, reward, t_pol, t_val, t_rew):
    if logits.ndim != 3:
        raise ValueError(f"logits must be [K+1, B, A], got {tuple(logits.shape)}")
    K1, B, A = logits.shape
    K = K1 - 1
    want = {"value": (value, (K1, B)), "t_pol": (t_pol, (B, K1, A)), "t_val": (t_val, (B, K1))}
    if K > 0:
        want.update(reward=(reward, (K, B)), t_rew=(t_rew, (B, K)))
    for name, (t, shape) in want.items():
        if t is None or tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {list(shape)} for logits {list(logits.shape)}, got "
                             f"{None if t is None else list(t.shape)}")
    return B, K, A


class _UnrollLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, value, reward, t_pol, t_val, t_rew, w_value, w_policy, w_reward, value_transform):
        B, K, A = _shapes(logits, value, reward, t_pol, t_val, t_rew)
        dev = logits.device
        f = [None if t is None or (K == 0 and i in (2, 5)) else t.detach().to(dev, torch.float32).contiguous()
             for i, t in enumerate((logits, value, reward, t_pol, t_val, t_rew))]
        per = torch.empty(B, device=dev)
        totals = torch.empty(4, dtype=torch.float64, device=dev)
        g_logits, g_value = torch.empty_like(f[0]), torch.empty_like(f[1])
        g_reward = torch.empty_like(f[2]) if K > 0 else None
        with torch.cuda.device(dev):
            check(lib.mzgo_unroll_loss(*(ptr(t) for t in f), B, K, A, w_value, w_policy, w_reward,
                                       int(bool(value_transform)), ptr(per), ptr(totals), ptr(g_logits), ptr(g_value),
                                       ptr(g_reward), stream_of(dev)))
        ctx.save_for_backward(g_logits, g_value, *(() if g_reward is None else (g_reward,)))
        ctx.mark_non_differentiable(totals)
        return per, totals

    @staticmethod
    def backward(ctx, g_per, _g_totals):
        g_logits, g_value, *rest = ctx.saved_tensors
        g_per = g_per.to(g_value.dtype)
        return (g_logits * g_per[None, :, None], g_value * g_per[None, :],
                rest[0] * g_per[None, :] if rest else None, None, None, None, None, None, None, None)


def unroll_loss(logits, value, reward, t_pol, t_val, t_rew, *, value_loss_weight, policy_loss_weight,
                reward_loss_weight, value_transform):
    """The unroll's loss from the heads' outputs stacked step-major (``logits``
    [K+1, B, A], ``value`` [K+1, B], ``reward`` [K, B]; None at K = 0) and the
    targets sample-major as ``device_targets`` / ``host_targets`` return them
    (``t_pol`` [B, K+1, A], ``t_val`` [B, K+1], ``t_rew`` [B, K]).  Returns
    ``(per_sample, totals)``: the per-sample losses f32 [B] (``_unroll_step``'s
    ``per``; differentiable, any weighting over samples) and the f64 [4]
    totals loss / value / policy / reward over all samples (not
    differentiable).  Device tensors only: there is no eager fall-back."""
    for name, t in (("logits", logits), ("value", value), ("reward", reward), ("t_pol", t_pol), ("t_val", t_val),
                    ("t_rew", t_rew)):
        if t is not None and t.device.type != "cuda":
            raise ValueError(f"unroll_loss runs on the GPU: {name} is on {t.device} (unroll_loss_host checks the "
                             "formulas on host arrays)")
    return _UnrollLoss.apply(logits, value, reward, t_pol, t_val, t_rew, float(value_loss_weight),
                             float(policy_loss_weight), float(reward_loss_weight), bool(value_transform))


def unroll_loss_host(logits, value, reward, t_pol, t_val, t_rew, *, value_loss_weight, policy_loss_weight,
                     reward_loss_weight, value_transform):
    """``mzgo_unroll_loss_host`` on numpy arrays of ``unroll_loss``'s layouts:
    (per_sample f32 [B], totals f64 [4], g_logits, g_value, g_reward or None),
    the gradients of ``per_sample.sum()``."""
    f32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float32)
    logits, value, reward, t_pol, t_val, t_rew = map(f32, (logits, value, reward, t_pol, t_val, t_rew))
    B, K, A = _shapes(logits, value, reward, t_pol, t_val, t_rew)
    if K == 0:
        reward = t_rew = None
    per = np.empty(B, np.float32)
    totals = np.empty(4, np.float64)
    g_logits, g_value = np.empty_like(logits), np.empty_like(value)
    g_reward = np.empty_like(reward) if K > 0 else None
    check(lib.mzgo_unroll_loss_host(ptr(logits), ptr(value), ptr(reward), ptr(t_pol), ptr(t_val), ptr(t_rew), B, K, A,
                                    float(value_loss_weight), float(policy_loss_weight), float(reward_loss_weight),
                                    int(bool(value_transform)), ptr(per), ptr(totals), ptr(g_logits), ptr(g_value),
                                    ptr(g_reward)))
    return per, totals, g_logits, g_value, g_reward
