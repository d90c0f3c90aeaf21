"""The fused unroll loss on the GPU (mzgo.unroll_loss, csrc/mzgo_loss.hip;
TrainConfig.fused_loss / sample_priorities).

* the kernel against torch's autograd on the device, float32 and float64,
  at tests/test_loss.py's shapes, inputs and bars; bit-identical repeats; the
  host twin; a weighted backward;
* one ``_unroll_step`` with ``fused_loss`` on and off from the same weights and
  targets under learning_rate 0: loss and ``last``'s terms rel 1e-5, every
  parameter's ``.grad`` rtol 1e-3, atol 1e-5 * max(1, |g|.max())
  (test_hip_forward_autograd_matches_torch's bars);
* ``train`` on a ``DeviceReplay`` with ``sample_priorities``.

The engine has no 5x5 / latent_dim 32 build, so that step's value targets take
their bootstrap values from the torch forward (``device_targets``' own three
calls otherwise); the 5x5 / 96 and 6x6 / 64 steps use ``device_targets``.
"""
import functools

import numpy as np
import pytest
import torch

from test_loss import SHAPES, WEIGHTS, check_against_reference, check_close, make_inputs, torch_reference

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _refs(B, K, A, transform):
    inp = make_inputs(B, K, A)
    return (torch_reference(inp, torch.float32, "cuda", transform),
            torch_reference(inp, torch.float64, "cuda", transform))


def _device_loss(B, K, A, transform, wts=None):
    import mzgo
    inp = {k: torch.as_tensor(np.array(v)).cuda() for k, v in make_inputs(B, K, A).items()}
    leaves = [inp[k].requires_grad_() for k in ("logits", "value", "reward")]
    per, totals = mzgo.unroll_loss(inp["logits"], inp["value"], inp["reward"] if K else None, inp["t_pol"],
                                   inp["t_val"], inp["t_rew"] if K else None, value_transform=transform, **WEIGHTS)
    assert per.dtype == torch.float32 and per.shape == (B,) and per.requires_grad
    assert totals.dtype == torch.float64 and totals.shape == (4,) and not totals.requires_grad
    (per.sum() if wts is None else (per * wts).sum()).backward()
    cpu = lambda t: t.detach().cpu().numpy()
    return dict(per=cpu(per), totals=cpu(totals), g_logits=cpu(leaves[0].grad), g_value=cpu(leaves[1].grad),
                g_reward=cpu(leaves[2].grad) if K else None)


@pytest.mark.parametrize("transform", [True, False])
@pytest.mark.parametrize("B,K,A", SHAPES)
def test_kernel_matches_torch_autograd_and_host_twin(B, K, A, transform):
    import mzgo
    got = _device_loss(B, K, A, transform)
    check_against_reference(got, *_refs(B, K, A, transform))
    # two calls on the same inputs: the same bits
    again = _device_loss(B, K, A, transform)
    for k, v in got.items():
        if v is not None:
            np.testing.assert_array_equal(v.view(np.uint8), again[k].view(np.uint8), err_msg=k)
    # the host twin runs the same scalar functions; its row sums run in entry order
    inp = make_inputs(B, K, A)
    per, totals, g_logits, g_value, g_reward = mzgo.unroll_loss_host(
        inp["logits"], inp["value"], inp["reward"] if K else None, inp["t_pol"], inp["t_val"],
        inp["t_rew"] if K else None, value_transform=transform, **WEIGHTS)
    host = dict(per=per, totals=totals, g_logits=g_logits, g_value=g_value, g_reward=g_reward)
    check_close(got, {k: None if v is None else np.asarray(v, dtype=np.float64) for k, v in host.items()})


@pytest.mark.parametrize("B,K,A", [(5, 10, 82), (128, 10, 37)])
def test_weighted_backward(B, K, A):
    wts = np.random.default_rng(5).random(B).astype(np.float32) * 3 + 0.1
    got = _device_loss(B, K, A, True, torch.as_tensor(wts).cuda())
    ref = torch_reference(make_inputs(B, K, A), torch.float32, "cuda", True, wts)
    check_close(got, ref)
    plain = _refs(B, K, A, True)[0]
    assert np.abs(ref["g_logits"] - plain["g_logits"]).max() > 0.1       # (the weights do change the gradients)


def _trajs(N, B, seed=9):
    from oracle.make_golden import synthetic_trajectories
    return synthetic_trajectories(N, B, seed=seed)


def _targets(tr, rp, idx, starts, engine_bootstrap):
    if engine_bootstrap:
        return tr.device_targets(rp, idx, starts)
    from mzgo.replay import finish_values
    from mzgo.trainer import initial_inference_torch
    c, N = tr.config, tr.net.board_size
    bt = rp.batch(idx, starts, c.unroll_steps, c.discount, None)
    with torch.no_grad():
        _, v, _ = initial_inference_torch(tr.net, bt["boot_obs"].view(-1, 6, N, N))
    return bt["obs0"], bt["acts"], finish_values(bt["val"], bt["factor"], bt["has_boot"], v), bt["t_rew"], bt["t_pol"]


@pytest.mark.parametrize("N,C,B,K,hip_forward", [(5, 32, 7, 3, False), (6, 64, 16, 10, False), (5, 96, 7, 3, True)])
def test_unroll_step_fused_equals_torch_loss(N, C, B, K, hip_forward):
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    A = N * N + 1
    trajs = _trajs(N, B)
    rp = mzgo.DeviceReplay(N, B, int(1.5 * N * N), "cuda")
    for t in trajs:
        rp.add(t)
    net = mzgo.MuZeroNet(C, A).cuda()
    net.load_state_dict(mzgo.deterministic_state_dict(C, A, 6))
    before = {k: v.clone() for k, v in net.state_dict().items()}
    idx = list(range(B))
    starts = [len(t["actions"]) // 3 for t in trajs]
    res = {}
    for fused in (False, True):
        cfg = TrainConfig(learning_rate=0.0, unroll_steps=K, fused_loss=fused, **WEIGHTS)
        tr = MuZeroTrainer(net, cfg, mode="batched", hip_forward=hip_forward)
        targets = _targets(tr, rp, idx, starts, engine_bootstrap=C != 32)
        loss = tr._unroll_step(*targets, device_totals=True)
        res[fused] = (loss, dict(tr.last), {k: p.grad.detach().clone() for k, p in net.named_parameters()}, targets)
        for k, v in net.state_dict().items():
            assert torch.equal(before[k], v), k
    for a, b in zip(res[True][3], res[False][3]):
        assert torch.equal(a, b)
    print(res[True][0], res[False][0], res[True][1], res[False][1])
    assert res[True][0] == pytest.approx(res[False][0], rel=1e-5)
    for k in ("training_loss", "value_loss", "policy_loss", "reward_loss"):
        assert res[True][1][k] == pytest.approx(res[False][1][k], rel=1e-5), k
    for k, g in res[False][2].items():
        np.testing.assert_allclose(res[True][2][k].cpu().numpy(), g.cpu().numpy(), rtol=1e-3,
                                   atol=1e-5 * max(1.0, g.abs().max().item()), err_msg=k)


@pytest.mark.parametrize("fused", [False, True])
def test_train_sets_per_sample_priorities(fused):
    import mzgo
    from mzgo.trainer import (MuZeroTrainer, TrainConfig, initial_inference_torch, recurrent_inference_torch)
    N, C, G, B, K = 5, 96, 6, 4, 10
    A = N * N + 1
    trajs = _trajs(N, G)
    start = lambda T: T // 2
    for flag in (True, False):
        rp = mzgo.DeviceReplay(N, G, int(1.5 * N * N), "cuda")
        for t in trajs:
            rp.add(t)
        nets = []
        for _ in range(2):                                   # the one that trains, and its pre-step weights
            net = mzgo.MuZeroNet(C, A).cuda()
            net.load_state_dict(mzgo.deterministic_state_dict(C, A, 4))
            nets.append(net)
        cfg = TrainConfig(unroll_steps=K, fused_loss=fused, sample_priorities=flag, **WEIGHTS)
        tr = MuZeroTrainer(nets[0], cfg, mode="batched", start_index=start)
        seen = []
        draw = rp.ledger.sample_indices
        rp.sample_indices = lambda n: seen.append(draw(n)) or seen[-1]
        np.random.seed(8)
        avg = tr.train(rp, B)
        idx = [int(i) for i in seen[0]]
        assert len(set(idx)) == B
        for i in range(G):
            if i not in idx:
                assert rp.priorities[i] == 1.0
        if not flag:
            assert [rp.priorities[i] for i in idx] == [avg] * B
            continue
        # the step's per-sample losses again: torch's expressions on the pre-step weights and the same targets
        ref = MuZeroTrainer(nets[1], cfg, mode="batched", start_index=start)
        obs0, acts, t_val, t_rew, t_pol = ref.device_targets(rp, idx, [start(rp.lengths[i]) for i in idx])
        with torch.no_grad():
            latent, value, logits = initial_inference_torch(nets[1], obs0)
            lg, vs, rs = [logits], [value.squeeze(1)], []
            for k in range(K):
                latent, reward, value, logits = recurrent_inference_torch(nets[1], latent, acts[:, k])
                lg.append(logits)
                vs.append(value.squeeze(1))
                rs.append(reward.squeeze(1))
        inp = dict(logits=torch.stack(lg), value=torch.stack(vs), reward=torch.stack(rs), t_pol=t_pol, t_val=t_val,
                   t_rew=t_rew)
        want = torch_reference({k: v.cpu().numpy() for k, v in inp.items()}, torch.float32, "cuda", True)["per"]
        got = np.array([rp.priorities[i] for i in idx])
        print(got, want, avg)
        np.testing.assert_allclose(got, want, rtol=1e-4)
        assert got.min() > 0 and len(set(got.tolist())) == B
        assert got.mean() == pytest.approx(avg, rel=1e-5)
