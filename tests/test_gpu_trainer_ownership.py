"""``TrainConfig.ownership_loss_weight`` in the batched step: one step's 24
gradients (the net's 22 and the ownership head's 2) against the full loss --
value + policy + reward + ownership on the same targets -- under torch autograd
in float64 (``f64_reference.check_bar``), determinism on the host-index and the
``device_sampling`` paths, weight 0 as the configuration without the field,
the reported ``ownership_loss``, ``deferred_stats``, and the loss falling on a
fixed batch.  N = 5, C = 16, B = 4, K = 2, a store of host-added finished games
with planted root values (search-value targets: the library builds no engine
for the bootstrap inference at these sizes).
"""
import copy
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mzgo
from f64_reference import RELU_INPUTS, check_bar
from mzgo.trainer import (MuZeroTrainer, TrainConfig, initial_inference_torch, recurrent_inference_torch,
                          reward_value_transform)
from oracle.make_golden import synthetic_trajectories

pytestmark = pytest.mark.gpu

N, C, B, K = 5, 16, 4, 2
A = N * N + 1
# NET_SEED: the smallest seed whose float64 graph keeps every ReLU input of the first step at least MIN_PRE from 0
NET_SEED, HEAD_SEED, WEIGHT = 0, 11, 0.5
STARTS = [0, 2, 1, 3]
MIN_PRE = 1e-5


def trajectories():
    out = []
    for i, t in enumerate(synthetic_trajectories(N, B, seed=9)):
        T = len(t["actions"])
        obs = [o.copy() for o in t["observations"]]
        for o in obs[T:]:
            o[5] = 1.0                                      # every game ended: the final board has owners
        out.append(dict(t, observations=obs, root_values=[((7 * i + 3 * j) % 11 - 5) / 8.0 for j in range(T)]))
    return out


def build_store():
    rp = mzgo.DeviceReplay(N, B, int(1.5 * N * N), "cuda")
    for t in trajectories():
        rp.add(t)
    return rp


def build_trainer(fixed_batch=True, head=True, **cfg):
    net = mzgo.MuZeroNet(C, A).cuda()
    net.load_state_dict(mzgo.deterministic_state_dict(C, A, NET_SEED))
    cfg = dict(dict(learning_rate=1e-3, unroll_steps=K, fused_loss=True, fused_unroll=True, value_target="search",
                    max_grad_norm=1e9), **cfg)
    torch.manual_seed(HEAD_SEED)                            # the head's initial weights
    starts = itertools.cycle(STARTS)
    tr = MuZeroTrainer(net, TrainConfig(**cfg), mode="batched", sample_seed=5,
                       start_index=(lambda T: min(next(starts), T - 1)) if fixed_batch else None)
    return tr


def fix_batch(rp):
    rp.sample_indices = lambda n: np.arange(n)              # game b from STARTS[b], every step
    return rp


def reference(net, head, targets, own, dtype, weights=(1.0, 1.0, 1.0)):
    """The full loss on the CPU in ``dtype`` -> (grads by name, the head's two last, min |ReLU input|, the
    ownership total)."""
    obs0, acts, t_val, t_rew, t_pol = (t.detach().cpu() for t in targets)
    t_own, mask = (t.detach().cpu().to(dtype) for t in own)
    net, head = copy.deepcopy(net).cpu().to(dtype), copy.deepcopy(head).cpu().to(dtype)
    net.zero_grad()
    head.zero_grad()
    pre = []
    modules = dict(net.named_modules())
    hooks = [modules[name].register_forward_hook(lambda m, i, o: pre.append(o.detach().abs().min().item()))
             for name in RELU_INPUTS]
    t_val, t_rew, t_pol = t_val.to(dtype), t_rew.to(dtype), t_pol.to(dtype)
    vloss = lambda v, t: F.mse_loss(reward_value_transform(v), reward_value_transform(t), reduction="none")
    kl = lambda lg, tp: F.kl_div(F.log_softmax(lg, dim=1), tp, reduction="none").sum(dim=1)
    w_v, w_p, w_r = weights

    def own_loss(latent, k):
        x = head.conv(latent).view(B, N * N)
        cell = torch.logaddexp(torch.zeros_like(x), 2 * x) - (1 + t_own[:, k]) * x
        return WEIGHT * mask[:, k] * cell.mean(dim=1)

    latent, value, logits = initial_inference_torch(net, obs0.to(dtype))
    per = w_v * vloss(value.squeeze(1), t_val[:, 0]) + w_p * kl(logits, t_pol[:, 0])
    per_own = own_loss(latent, 0)
    for k in range(1, K + 1):
        latent, reward, value, logits = recurrent_inference_torch(net, latent, acts[:, k - 1])
        per = per + w_r * F.mse_loss(reward.squeeze(1), t_rew[:, k - 1], reduction="none") \
            + w_v * vloss(value.squeeze(1), t_val[:, k]) + w_p * kl(logits, t_pol[:, k])
        per_own = per_own + own_loss(latent, k)
    for h in hooks:
        h.remove()
    (per + per_own).sum().backward()
    grads = {k: p.grad.double().numpy() for k, p in net.named_parameters()}
    grads.update({"ownership." + k: p.grad.double().numpy() for k, p in head.named_parameters()})
    return grads, min(pre), per_own.sum().item()


def test_one_steps_24_gradients_against_float64():
    rp = fix_batch(build_store())
    tr = build_trainer(ownership_loss_weight=WEIGHT)
    head = tr.ownership_head
    assert isinstance(head, mzgo.OwnershipHead) and head.conv.weight.is_cuda
    assert len(tr.optimizer.param_groups[0]["params"]) == 24
    targets = tr.device_targets(rp, np.arange(B), STARTS, None)
    own = rp.ownership(np.arange(B), STARTS, K)
    assert own[1].sum().item() > 0
    before = copy.deepcopy(tr.net), copy.deepcopy(head)
    ref32, _, own_total32 = reference(*before, targets, own, torch.float32)
    ref64, min_pre, own_total = reference(*before, targets, own, torch.float64)
    assert min_pre >= MIN_PRE, min_pre                     # no ReLU of the float64 graph sits on its kink
    assert tr.train(rp, B) is not None
    got = {k: p.grad for k, p in tr.net.named_parameters()}
    got.update({"ownership." + k: p.grad for k, p in head.named_parameters()})
    assert set(got) == set(ref64) and len(got) == 24
    for k in ref64:
        check_bar(k, got[k], ref32[k], ref64[k])
    assert np.abs(ref64["ownership.conv.weight"]).max() > 0
    # the reported ownership loss: the float64 graph's, and the host twin's on the latents the step read
    check_bar("ownership_loss", tr.last["ownership_loss"] * B, own_total32, own_total)
    net0, head0 = before
    out = mzgo.unroll(net0, targets[0], targets[1], return_latents=True)
    host = mzgo.ownership_loss_host(out[3].detach().cpu().numpy(), head0.conv.weight.detach().cpu().numpy(),
                                    head0.conv.bias.detach().cpu().numpy(), own[0].cpu().numpy(), own[1].cpu().numpy(),
                                    WEIGHT)
    # device and host differ in libm's expf / log1pf (a few float32 ulp per cell term) and in the order of the f64
    # sums (1e-16): 1e-6 relative holds a margin of ten over both
    assert tr.last["ownership_loss"] == pytest.approx(host["total"] / B, rel=1e-6)
    # training_loss and the three totals are those of the loss without ownership
    assert tr.last["training_loss"] == pytest.approx(
        tr.last["value_loss"] + tr.last["policy_loss"] + tr.last["reward_loss"], rel=1e-5)


def run_steps(steps=3, **cfg):
    rp = build_store()
    fixed = not cfg.get("device_sampling")
    if fixed:
        fix_batch(rp)
    tr = build_trainer(fixed_batch=fixed, **cfg)
    stats = []
    for _ in range(steps):
        assert tr.train(rp, B) is not None
        stats.append(dict(tr.read_stats()))
    params = [p.detach().clone() for p in tr.net.parameters()]
    if tr.ownership_head is not None:
        params += [p.detach().clone() for p in tr.ownership_head.parameters()]
    return params, stats


@pytest.mark.parametrize("cfg", [dict(), dict(device_optimizer=True),
                                 dict(device_sampling=True, importance_beta=0.5, symmetries=True, sample_priorities=True,
                                      device_optimizer=True)],
                         ids=["host-index", "host-index-device-optimizer", "device-sampling"])
def test_two_trainers_stay_bit_equal(cfg):
    a, sa = run_steps(ownership_loss_weight=WEIGHT, **cfg)
    b, sb = run_steps(ownership_loss_weight=WEIGHT, **cfg)
    assert len(a) == len(b) == 24 and sa == sb
    start = mzgo.deterministic_state_dict(C, A, NET_SEED)
    for p, q, k in zip(a, b, list(start) + ["head.weight", "head.bias"]):
        assert torch.equal(p, q), k
        if k in start:
            assert not torch.equal(p.cpu(), start[k]), k    # and they trained
    assert all(np.isfinite(s["ownership_loss"]) and s["ownership_loss"] > 0 for s in sa)


@pytest.mark.parametrize("cfg", [dict(), dict(device_sampling=True, importance_beta=0.5, device_optimizer=True)],
                         ids=["host-index", "device-sampling"])
def test_weight_zero_is_the_configuration_without_the_field(cfg):
    a, sa = run_steps(ownership_loss_weight=0.0, **cfg)
    b, sb = run_steps(**cfg)
    assert len(a) == len(b) == 22 and sa == sb and "ownership_loss" not in sa[0]
    for p, q in zip(a, b):
        assert torch.equal(p, q)
    # and the ownership loss changes the step: it reaches the net through the latents
    c, _ = run_steps(ownership_loss_weight=WEIGHT, **cfg)
    assert not torch.equal(a[0], c[0])


def test_deferred_stats_read_nothing_until_asked():
    rp = build_store()
    tr = build_trainer(fixed_batch=False, ownership_loss_weight=WEIGHT, device_sampling=True, deferred_stats=True,
                       device_optimizer=True)
    out = tr.train(rp, B)
    assert isinstance(out, torch.Tensor) and out.is_cuda and tr.last == {}
    stats = tr.read_stats()
    assert stats["ownership_loss"] > 0 and np.isfinite(stats["training_loss"])


def test_the_ownership_loss_falls_on_a_fixed_batch():
    rp = fix_batch(build_store())
    tr = build_trainer(ownership_loss_weight=1.0, value_loss_weight=0.0, policy_loss_weight=0.0, reward_loss_weight=0.0,
                       learning_rate=3e-3, max_grad_norm=1.0)
    losses = []
    for _ in range(40):
        tr.train(rp, B)
        losses.append(tr.last["ownership_loss"])
    print("ownership loss", losses[0], "->", losses[-1])
    assert tr.last["training_loss"] == 0.0
    assert losses[-1] < 0.8 * losses[0]
