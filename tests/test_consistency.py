"""The latent consistency loss without a GPU: the head's loss and all five
gradients (``mzgo.consistency_loss_host``, the kernels' scalar functions walked
serially) against the torch definition -- ``ConsistencyHead``'s own methods and
``F.cosine_similarity(..., eps=1e-8)`` under autograd -- in float64 under
``f64_reference.check_bar``; the masked rows, step 0 and the degenerate rule as
exact zeros; and the configurations the head and the trainer refuse.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mzgo
from f64_reference import check_bar
from mzgo.trainer import MuZeroTrainer, TrainConfig

# (N, C, P, B, K)
LOSS_SHAPES = [(2, 16, 16, 1, 1), (5, 48, 32, 3, 2), (9, 128, 32, 2, 1), (19, 16, 64, 2, 1)]
WEIGHT = 0.7
KEYS = ("per", "total", "g_latents", "g_proj_w", "g_proj_b", "g_pred_w", "g_pred_b")
MIN_PRE, MIN_NORM = 1e-3, 1e-2


@functools.lru_cache(maxsize=None)
def loss_inputs(N, C, P, B, K, seed=0):
    """Fixed-seed inputs with O(1) norms.  The latents and targets are ReLU outputs, as the network's are.  proj's
    biases sit at +-(1.5..2) with alternating signs and its weights give u a spread of about 0.2 around them, so half
    the ReLUs are on, half off, and none is near its kink (the tests assert it)."""
    g = torch.Generator().manual_seed(seed + 1000 * N + 10 * C + P)
    lat = torch.relu(torch.randn(K + 1, B, C, N, N, generator=g))
    tgt = torch.relu(torch.randn(K, B, C, N, N, generator=g))
    proj_w = torch.randn(P, C, 1, 1, generator=g) * (0.3 / C ** 0.5)
    sign = torch.where(torch.arange(P) % 2 == 0, 1.0, -1.0)
    proj_b = sign * (1.5 + 0.5 * torch.rand(P, generator=g))
    pred_w = torch.randn(P, P, 1, 1, generator=g) * (1.0 / P ** 0.5)
    pred_b = torch.randn(P, generator=g) * 0.1
    mask = torch.ones(B, K)
    if B * K > 1:
        mask[-1, -1] = 0                                   # one row without a target
    g_per = torch.rand(B, generator=g) + 0.5               # non-uniform
    return lat, tgt, mask, proj_w, proj_b, pred_w, pred_b, g_per


def make_head(proj_w, proj_b, pred_w, pred_b, dtype=torch.float32):
    P, C = proj_w.shape[:2]
    head = mzgo.ConsistencyHead(C, P).to(dtype)
    with torch.no_grad():
        for p, v in zip((head.proj.weight, head.proj.bias, head.pred.weight, head.pred.bias),
                        (proj_w, proj_b, pred_w, pred_b)):
            p.copy_(v.to(dtype))
    return head


def torch_loss(lat, tgt, mask, proj_w, proj_b, pred_w, pred_b, g_per, weight, dtype):
    """The definition with torch ops under autograd in ``dtype``: a dict over KEYS, plus ``min_u``, ``min_p`` and
    ``min_z``, the smallest |u| entry and the smallest |p| and |z| over the unmasked rows."""
    head = make_head(proj_w, proj_b, pred_w, pred_b, dtype)
    lat = lat.detach().to(dtype).requires_grad_()
    tgt, mask = tgt.to(dtype), mask.to(dtype)
    K1, B, C, N, _ = lat.shape
    K = K1 - 1
    u = head.project(lat[1:].reshape(K * B, C, N, N))
    p = head.predict(u).reshape(K * B, -1)
    z = head.project(tgt.reshape(K * B, C, N, N)).detach().reshape(K * B, -1)      # the stop-gradient
    cos = F.cosine_similarity(p, z, dim=1, eps=1e-8).view(K, B)
    per = weight * (mask.t() * (1 - cos)).sum(dim=0)
    (per * g_per.to(dtype)).sum().backward()
    on = mask.t().reshape(-1) > 0
    out = dict(per=per.detach(), total=per.detach().sum(), g_latents=lat.grad, g_proj_w=head.proj.weight.grad.view(-1, C),
               g_proj_b=head.proj.bias.grad, g_pred_w=head.pred.weight.grad.view(p.shape[1] // (N * N), -1),
               g_pred_b=head.pred.bias.grad)
    out["min_u"] = u.detach()[on].abs().min().item()
    out["min_p"] = p.detach()[on].norm(dim=1).min().item()
    out["min_z"] = z[on].norm(dim=1).min().item()
    return out


def host_loss(lat, tgt, mask, proj_w, proj_b, pred_w, pred_b, g_per, weight):
    return mzgo.consistency_loss_host(lat.numpy(), tgt.numpy(), mask.numpy(), proj_w.numpy(), proj_b.numpy(),
                                      pred_w.numpy(), pred_b.numpy(), weight, g_per.numpy())


@functools.lru_cache(maxsize=None)
def references(N, C, P, B, K):
    """(torch float32, torch float64) of ``loss_inputs(N, C, P, B, K)`` at WEIGHT: computed once, read by the CPU
    and the GPU tests."""
    args = loss_inputs(N, C, P, B, K)
    return torch_loss(*args, WEIGHT, torch.float32), torch_loss(*args, WEIGHT, torch.float64)


@pytest.mark.parametrize("N,C,P,B,K", LOSS_SHAPES)
def test_loss_host_against_float64(N, C, P, B, K):
    args = loss_inputs(N, C, P, B, K)
    mask = args[2]
    ref32, ref64 = references(N, C, P, B, K)
    print(f"min |u| {ref64['min_u']:.3g}  min |p| {ref64['min_p']:.3g}  min |z| {ref64['min_z']:.3g}")
    assert ref64["min_u"] >= MIN_PRE                       # no precision flips a ReLU
    assert ref64["min_p"] > MIN_NORM and ref64["min_z"] > MIN_NORM
    assert mask.sum() >= 1 and (B * K == 1 or (mask == 0).sum() >= 1)
    got = host_loss(*args, WEIGHT)
    for k in KEYS:
        check_bar(k, got[k], ref32[k], ref64[k])
    assert np.abs(ref64["g_latents"].numpy()).max() > 0 and np.abs(ref64["g_proj_w"].numpy()).max() > 0
    assert (got["g_latents"][0] == 0).all()                # step 0 takes no part
    if B * K > 1:                                          # the masked row: exact zeros
        assert (got["g_latents"][K, B - 1] == 0).all()
        assert (ref64["g_latents"][K, B - 1] == 0).all()


def test_a_masked_row_is_not_read():
    N, C, P, B, K = 5, 48, 32, 3, 2
    lat, tgt, mask, *rest = loss_inputs(N, C, P, B, K)
    base = host_loss(lat, tgt, mask, *rest, WEIGHT)
    tgt2, lat2 = tgt.clone(), lat.clone()
    tgt2[K - 1, B - 1] = torch.randn_like(tgt2[K - 1, B - 1]) * 100
    lat2[K, B - 1] = float("nan")
    again = host_loss(lat2, tgt2, mask, *rest, WEIGHT)
    for k in KEYS:
        np.testing.assert_array_equal(base[k], again[k], err_msg=k)
    # the masked row's share of its sample's loss is an exact zero: per[B-1] is the sample's other row alone
    m2 = mask.clone()
    m2[B - 1, :K - 1] = 0
    assert host_loss(lat, tgt, m2, *rest, WEIGHT)["per"][B - 1] == 0.0


def test_all_zero_head_parameters_are_the_degenerate_rule():
    N, C, P, B, K = 5, 48, 32, 3, 2
    lat, tgt, mask, proj_w, proj_b, pred_w, pred_b, g_per = loss_inputs(N, C, P, B, K)
    zeros = [torch.zeros_like(t) for t in (proj_w, proj_b, pred_w, pred_b)]
    got = host_loss(lat, tgt, mask, *zeros, g_per, 0.5)
    np.testing.assert_array_equal(got["per"], 0.5 * mask.sum(dim=1).numpy())
    assert got["total"] == 0.5 * mask.sum().item()
    for k in KEYS[2:]:
        assert np.isfinite(got[k]).all() and (got[k] == 0).all(), k


def test_the_head():
    head = mzgo.ConsistencyHead(16)
    assert [k for k, _ in head.named_parameters()] == ["proj.weight", "proj.bias", "pred.weight", "pred.bias"]
    assert tuple(head.proj.weight.shape) == (32, 16, 1, 1) and tuple(head.pred.weight.shape) == (32, 32, 1, 1)
    x = torch.randn(2, 16, 5, 5)
    torch.testing.assert_close(head.project(x), F.conv2d(x, head.proj.weight, head.proj.bias))
    z = head.project(x)
    torch.testing.assert_close(head.predict(z), F.conv2d(torch.relu(z), head.pred.weight, head.pred.bias))
    torch.testing.assert_close(head(x), head.predict(head.project(x)))
    for P in (16, 32, 48, 64):
        assert mzgo.ConsistencyHead(16, P).proj_dim == P
    for P in (24, 80):
        with pytest.raises(ValueError, match="proj_dim must be one of"):
            mzgo.ConsistencyHead(16, P)
    # the net keeps the reference's 22 tensors
    assert len(list(mzgo.MuZeroNet(16, 26).parameters())) == 22


# ---------------------------------------------------------------------------
# what is refused
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs,mode,match", [
    (dict(), "reference", "consistency_loss_weight needs mode='batched'"),
    (dict(fused_loss=True), "batched", "consistency_loss_weight needs fused_unroll=True"),
    (dict(fused_unroll=True), "batched", "consistency_loss_weight needs fused_loss=True"),
    (dict(fused_unroll=True, fused_loss=True, unroll_steps=0), "batched",
     "consistency_loss_weight needs unroll_steps >= 1"),
    (dict(fused_unroll=True, fused_loss=True), "batched", "consistency_loss_weight needs the net on the GPU"),
])
def test_consistency_loss_weight_is_refused_without_its_requirements(kwargs, mode, match):
    net = mzgo.MuZeroNet(16, 26)
    with pytest.raises(ValueError, match=match):
        MuZeroTrainer(net, TrainConfig(consistency_loss_weight=0.5, **kwargs), mode=mode)


def test_other_refusals():
    net = mzgo.MuZeroNet(16, 26)
    assert TrainConfig().consistency_loss_weight == 0.0 and TrainConfig().consistency_proj_dim == 32
    assert MuZeroTrainer(net, TrainConfig()).consistency_head is None
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="consistency_loss_weight must be finite and >= 0"):
            MuZeroTrainer(net, TrainConfig(consistency_loss_weight=bad))
    with pytest.raises(ValueError, match="belong to consistency_loss_weight"):
        MuZeroTrainer(net, TrainConfig(), consistency_head=mzgo.ConsistencyHead(16))
    with pytest.raises(ValueError, match="belong to consistency_loss_weight"):
        MuZeroTrainer(net, TrainConfig(consistency_proj_dim=64))
    on = dict(consistency_loss_weight=0.5, fused_unroll=True, fused_loss=True)
    with pytest.raises(ValueError, match=r"consistency_head must be a ConsistencyHead\(16"):
        MuZeroTrainer(net, TrainConfig(**on), mode="batched", consistency_head=mzgo.ConsistencyHead(32))
    with pytest.raises(ValueError, match=r"consistency_head must be a ConsistencyHead\(16"):
        MuZeroTrainer(net, TrainConfig(**on), mode="batched", consistency_head=mzgo.OwnershipHead(16))
    with pytest.raises(ValueError, match="mzgo.encode runs on the GPU"):
        mzgo.encode(net, torch.zeros(1, 6, 5, 5))
    with pytest.raises(ValueError, match="consistency_loss runs on the GPU"):
        mzgo.consistency_loss(torch.zeros(2, 1, 16, 5, 5), torch.zeros(1, 1, 16, 5, 5), torch.ones(1, 1),
                              mzgo.ConsistencyHead(16))
    with pytest.raises(TypeError, match="needs a ConsistencyHead"):
        mzgo.consistency_loss(torch.zeros(2, 1, 16, 5, 5), torch.zeros(1, 1, 16, 5, 5), torch.ones(1, 1),
                              mzgo.OwnershipHead(16))
