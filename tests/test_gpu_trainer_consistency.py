"""``TrainConfig.consistency_loss_weight`` in the batched step: one step's 26
gradients (the net's 22 and the consistency head's 4) against the same step
assembled from ``mzgo.unroll``, ``mzgo.unroll_loss``, ``mzgo.encode`` and the
torch head (float64 as the reference, float32 as ``check_bar``'s own term);
weight 0 as the configuration without the field; the option next to
``ownership_loss_weight``, to ``device_sampling`` + ``deferred_stats`` +
``device_optimizer`` and to ``unroll_precision="bf16"``.  N = 5, C = 32, B = 4,
K = 2, a store of host-added finished games with planted root values
(search-value targets: the library builds no engine for the bootstrap
inference at these sizes).
"""
import copy
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mzgo
from f64_reference import check_bar
from mzgo.trainer import MuZeroTrainer, TrainConfig
from oracle.make_golden import synthetic_trajectories
from test_consistency import loss_inputs, make_head

pytestmark = pytest.mark.gpu

N, C, P, B, K = 5, 32, 32, 4, 2
A = N * N + 1
NET_SEED, HEAD_SEED, WEIGHT = 0, 11, 0.5
STARTS = [0, 2, 1, 3]


def trajectories():
    out = []
    for i, t in enumerate(synthetic_trajectories(N, B, seed=9)):
        T = len(t["actions"])
        obs = [o.copy() for o in t["observations"]]
        for o in obs[T:]:
            o[5] = 1.0                                      # every game ended (the ownership option's condition)
        out.append(dict(t, observations=obs, root_values=[((7 * i + 3 * j) % 11 - 5) / 8.0 for j in range(T)]))
    return out


def build_store():
    rp = mzgo.DeviceReplay(N, B, int(1.5 * N * N), "cuda")
    for t in trajectories():
        rp.add(t)
    return rp


def build_trainer(fixed_batch=True, consistency_head=None, **cfg):
    net = mzgo.MuZeroNet(C, A).cuda()
    net.load_state_dict(mzgo.deterministic_state_dict(C, A, NET_SEED))
    cfg = dict(dict(learning_rate=1e-3, unroll_steps=K, fused_loss=True, fused_unroll=True, value_target="search",
                    max_grad_norm=1e9), **cfg)
    torch.manual_seed(HEAD_SEED)                            # the heads' initial weights
    starts = itertools.cycle(STARTS)
    return MuZeroTrainer(net, TrainConfig(**cfg), mode="batched", sample_seed=5, consistency_head=consistency_head,
                         start_index=(lambda T: min(next(starts), T - 1)) if fixed_batch else None)


def fix_batch(rp):
    rp.sample_indices = lambda n: np.arange(n)              # game b from STARTS[b], every step
    return rp


def far_head():
    """A head whose ReLU inputs stay far from 0 (``test_consistency.loss_inputs``' parameters)."""
    return make_head(*loss_inputs(N, C, P, B, K)[3:7]).cuda()


def torch_consistency(head, latents, targets, mask, dtype):
    """The loss of ``test_consistency.torch_loss`` on device tensors: (per [B] in ``dtype``, min |u|)."""
    u = head.project(latents[1:].reshape(K * B, C, N, N).to(dtype))
    p = head.predict(u).reshape(K * B, -1)
    z = head.project(targets.reshape(K * B, C, N, N).to(dtype)).detach().reshape(K * B, -1)
    cos = F.cosine_similarity(p, z, dim=1, eps=1e-8).view(K, B)
    return WEIGHT * (mask.to(dtype).t() * (1 - cos)).sum(dim=0), u.detach().abs().min().item()


def assembled(net, head, targets, window, dtype):
    """The step's gradients from ``mzgo.unroll``, ``mzgo.unroll_loss``, ``mzgo.encode`` and the torch head in
    ``dtype``: (grads by name, the consistency total, min |u|)."""
    obs0, acts, t_val, t_rew, t_pol = targets
    net, head = copy.deepcopy(net), copy.deepcopy(head).to(dtype)
    net.zero_grad()
    head.zero_grad()
    tgt = mzgo.encode(net, window[0].view(K * B, 6, N, N)).view(K, B, C, N, N)
    lgs, vals, rews, latents = mzgo.unroll(net, obs0, acts, return_latents=True)
    per, _ = mzgo.unroll_loss(lgs, vals, rews, t_pol, t_val, t_rew, value_loss_weight=1.0, policy_loss_weight=1.0,
                              reward_loss_weight=1.0, value_transform=True)
    per_cons, min_u = torch_consistency(head, latents, tgt, window[1], dtype)
    (per.to(dtype) + per_cons).sum().backward()
    grads = {k: p.grad.double().cpu().numpy() for k, p in net.named_parameters()}
    grads.update({"consistency." + k: p.grad.double().cpu().numpy() for k, p in head.named_parameters()})
    return grads, per_cons.detach().sum().item(), min_u


def test_one_steps_26_gradients_against_the_assembled_step():
    rp = fix_batch(build_store())
    tr = build_trainer(consistency_loss_weight=WEIGHT, consistency_head=far_head())
    head = tr.consistency_head
    assert isinstance(head, mzgo.ConsistencyHead) and head.proj.weight.is_cuda
    assert len(tr.optimizer.param_groups[0]["params"]) == 26
    targets = tr.device_targets(rp, np.arange(B), STARTS, None)
    window = rp.window_obs(np.arange(B), STARTS, K)
    assert 0 < window[1].sum().item()
    before = copy.deepcopy(tr.net), copy.deepcopy(head)
    ref32, total32, _ = assembled(*before, targets, window, torch.float32)
    ref64, total64, min_u = assembled(*before, targets, window, torch.float64)
    assert min_u >= 1e-3, min_u                            # no precision flips a ReLU of the head
    assert tr.train(rp, B) is not None
    got = {k: p.grad for k, p in tr.net.named_parameters()}
    got.update({"consistency." + k: p.grad for k, p in head.named_parameters()})
    assert set(got) == set(ref64) and len(got) == 26
    for k in ref64:
        check_bar(k, got[k], ref32[k], ref64[k])
    assert all(np.abs(ref64["consistency." + k]).max() > 0 for k, _ in head.named_parameters())
    for p, q in zip(head.parameters(), before[1].parameters()):
        assert not torch.equal(p, q)                        # the head's four parameters moved
    assert np.isfinite(tr.last["consistency_loss"]) and tr.last["consistency_loss"] > 0
    check_bar("consistency_loss", tr.last["consistency_loss"] * B, total32, total64)
    # training_loss and the three totals are those of the loss without the option
    assert tr.last["training_loss"] == pytest.approx(
        tr.last["value_loss"] + tr.last["policy_loss"] + tr.last["reward_loss"], rel=1e-5)


def run_steps(steps=2, **cfg):
    rp = build_store()
    fixed = not cfg.get("device_sampling")
    if fixed:
        fix_batch(rp)
    tr = build_trainer(fixed_batch=fixed, **cfg)
    stats = []
    for _ in range(steps):
        assert tr.train(rp, B) is not None
        stats.append(dict(tr.read_stats()))
    params = [p.detach().clone() for p in tr._parameters()]
    return params, stats


def test_weight_zero_is_the_configuration_without_the_field():
    a, sa = run_steps(consistency_loss_weight=0.0)
    b, sb = run_steps()
    assert len(a) == len(b) == 22 and sa == sb and "consistency_loss" not in sa[0]
    for p, q in zip(a, b):
        assert torch.equal(p, q)
    # and the option changes the step: it reaches the net through the latents; two such trainers stay bit-equal
    c, sc = run_steps(consistency_loss_weight=WEIGHT)
    d, sd = run_steps(consistency_loss_weight=WEIGHT)
    assert len(c) == 26 and not torch.equal(a[0], c[0]) and sc == sd
    for p, q in zip(c, d):
        assert torch.equal(p, q)


def test_next_to_the_ownership_loss_the_two_latent_gradients_add():
    rp = fix_batch(build_store())
    tr = build_trainer(consistency_loss_weight=WEIGHT, ownership_loss_weight=0.25)
    assert len(tr.optimizer.param_groups[0]["params"]) == 28
    obs0, acts, *_ = tr.device_targets(rp, np.arange(B), STARTS, None)
    own = rp.ownership(np.arange(B), STARTS, K)
    window = rp.window_obs(np.arange(B), STARTS, K)
    tgt = mzgo.encode(tr.net, window[0].view(K * B, 6, N, N)).view(K, B, C, N, N)

    def latent_gradient(with_own, with_cons):
        seen = []
        latents = mzgo.unroll(tr.net, obs0, acts, return_latents=True)[3]
        latents.register_hook(seen.append)
        per = 0
        if with_own:
            per = per + mzgo.ownership_loss(latents, tr.ownership_head, *own, weight=0.25)[0]
        if with_cons:
            per = per + mzgo.consistency_loss(latents, tgt, window[1], tr.consistency_head, WEIGHT)[0]
        per.sum().backward()
        return seen[0]

    g_own, g_cons, g_both = latent_gradient(True, False), latent_gradient(False, True), latent_gradient(True, True)
    assert g_own.abs().sum() > 0 and g_cons.abs().sum() > 0
    assert torch.equal(g_both, g_own + g_cons)
    for p in tr._parameters():
        p.grad = None
    assert tr.train(rp, B) is not None
    assert tr.last["consistency_loss"] > 0 and tr.last["ownership_loss"] > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in tr._parameters())


def test_with_device_sampling_deferred_stats_and_the_device_optimizer():
    rp = build_store()
    tr = build_trainer(fixed_batch=False, consistency_loss_weight=WEIGHT, device_sampling=True, deferred_stats=True,
                       device_optimizer=True, symmetries=True, importance_beta=0.5)
    before = [p.detach().clone() for p in tr.consistency_head.parameters()]
    out = tr.train(rp, B)
    assert isinstance(out, torch.Tensor) and out.is_cuda and tr.last == {}
    stats = tr.read_stats()
    assert np.isfinite(stats["consistency_loss"]) and stats["consistency_loss"] > 0
    assert np.isfinite(stats["training_loss"]) and "ownership_loss" not in stats
    for p, q in zip(tr.consistency_head.parameters(), before):
        assert not torch.equal(p, q)


def test_with_the_bf16_unroll():
    rp = fix_batch(build_store())
    tr = build_trainer(consistency_loss_weight=WEIGHT, unroll_precision="bf16")
    assert tr.train(rp, B) is not None
    assert np.isfinite(tr.last["consistency_loss"]) and tr.last["consistency_loss"] > 0
    assert np.isfinite(tr.last["training_loss"])
    assert all(torch.isfinite(p).all() and torch.isfinite(p.grad).all() for p in tr._parameters())


def test_a_host_buffer_is_refused():
    tr = build_trainer(consistency_loss_weight=WEIGHT)
    with pytest.raises(ValueError, match="consistency_loss_weight needs a DeviceReplay"):
        tr.train(mzgo.trainer.PrioritizedReplayBuffer(8), B)
