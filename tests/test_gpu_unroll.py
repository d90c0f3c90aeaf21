"""The fused unroll on the GPU (``mzgo.unroll``, csrc/mzgo_unroll.hip;
``TrainConfig.fused_unroll``) against the all-torch graph
(``initial_inference_torch`` / ``recurrent_inference_torch`` on the same
parameters), against the per-layer HIP backward it is composed of, against
itself (repeats), and inside the trainer.

Bars: tests/test_gpu_trainer.py's HIP-against-torch ones
(``test_hip_forward_autograd_matches_torch``: loss rel 1e-5, every parameter
gradient rtol 1e-3 with atol 1e-5 * max(1, |ref|.max());
``test_conv3x3_layer_hip_matches_torch``: a layer's forward 1e-5 + 1e-5 |ref|;
``test_dyn_conv_backward_hip_matches_torch``: a weight gradient 1e-4 + 1e-4
|ref|).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

UNUSED_ROW = 1     # an action no sample ever takes: its embedding gradient is exactly 0
# (N, C, B, K, embedding rows): 6x6 has K B = 90 boards, a ragged last chunk of the 8-board weight pass;
# the last net is built with board_size=5 and a 37-row table (play.py:193)
CASES = [(5, 96, 7, 3, 26), (6, 128, 9, 10, 37), (9, 96, 2, 2, 82), (19, 96, 1, 1, 362), (5, 32, 1, 0, 26),
         (5, 32, 4, 2, 37)]


def _net(N, C, rows, seed=2):
    import mzgo
    net = mzgo.MuZeroNet(C, rows, board_size=N if rows != N * N + 1 else None).cuda()
    net.load_state_dict(mzgo.deterministic_state_dict(C, rows, seed))
    return net


@functools.lru_cache(maxsize=None)
def _inputs(N, B, K, rows):
    """``random_position`` observations; actions over the whole table (rows
    past the board's N*N + 1 included when there are any) except UNUSED_ROW,
    with the pass, one action twice within step 0 and again in step 1."""
    from oracle.positions import random_position
    A = N * N + 1
    obs = torch.as_tensor(np.stack([random_position(N, 3 * b, b) for b in range(B)]), dtype=torch.float32).cuda()
    r = np.random.default_rng(N + 10 * B + K)
    acts = r.integers(2, rows, size=(B, K))
    if K:
        acts[B - 1, K - 1] = A - 1                         # the pass
        acts[0, 0] = 3
    if K and B > 1:
        acts[1, 0] = 3                                     # twice within a step ...
    if K > 1:
        acts[0, 1] = 3                                     # ... and again in another step
    assert (acts != UNUSED_ROW).all()
    return obs, torch.as_tensor(acts, dtype=torch.int64).cuda()


def _mixed_loss(logits, value, reward):
    """``test_hip_forward_autograd_matches_torch``'s loss on the stacked head
    outputs (its 1e-3 |latent|^2 term has no counterpart: the fused unroll
    returns no latents)."""
    loss = (value[0] ** 2).sum() + logits[0].logsumexp(1).sum()
    for k in range(1, logits.shape[0]):
        loss = loss + (reward[k - 1] ** 2).sum() + (value[k] * 0.5).sum() + logits[k].logsumexp(1).sum()
    return loss


def _grads(net):
    return {k: None if p.grad is None else p.grad.detach().clone() for k, p in net.named_parameters()}


@functools.lru_cache(maxsize=None)
def _torch_reference(N, C, B, K, rows):
    """The all-torch graph once per case: (outputs, loss, gradients)."""
    from mzgo.trainer import initial_inference_torch, recurrent_inference_torch
    net = _net(N, C, rows)
    obs, acts = _inputs(N, B, K, rows)
    latent, value, logits = initial_inference_torch(net, obs)
    lgs, vals, rews = [logits], [value.squeeze(1)], []
    for k in range(1, K + 1):
        latent, reward, value, logits = recurrent_inference_torch(net, latent, acts[:, k - 1])
        lgs.append(logits)
        vals.append(value.squeeze(1))
        rews.append(reward.squeeze(1))
    out = (torch.stack(lgs), torch.stack(vals), torch.stack(rews) if rews else None)
    loss = _mixed_loss(*out)
    loss.backward()
    return tuple(None if o is None else o.detach() for o in out), loss.item(), _grads(net)


def _run_unroll(N, C, B, K, rows):
    import mzgo
    net = _net(N, C, rows)
    obs, acts = _inputs(N, B, K, rows)
    out = mzgo.unroll(net, obs, acts)
    loss = _mixed_loss(*out)
    loss.backward()
    return tuple(None if o is None else o.detach() for o in out), loss.item(), _grads(net)


@pytest.mark.parametrize("N,C,B,K,rows", CASES)
def test_unroll_matches_the_torch_graph(N, C, B, K, rows):
    """Outputs, loss and all 22 parameter gradients against the all-torch graph.

    Output tolerance: ``test_conv3x3_layer_hip_matches_torch``'s 1e-5 + 1e-5
    |ref| for every step, unscaled.  A scaling by the chain's depth is not
    needed: a layer maps an input error e to about e sqrt(fan_in) rms(w) =
    e / sqrt(3) for weights uniform in +-1/sqrt(fan_in) (the initialisation;
    ReLU is 1-Lipschitz), so the 4 + k layers behind step k's outputs shrink
    what they receive and the sum of their own errors stays below
    1 / (1 - 1/sqrt(3)) = 2.4 times one layer's -- and one layer's, fp32
    rounding over at most 9 x 128 terms of size <= 1, is some 1e-6, well inside
    the per-layer bar."""
    A = N * N + 1
    ref_out, ref_loss, ref_g = _torch_reference(N, C, B, K, rows)
    out, loss, g = _run_unroll(N, C, B, K, rows)
    assert out[0].shape == (K + 1, B, A) and out[1].shape == (K + 1, B)
    assert (out[2] is None and ref_out[2] is None) if K == 0 else out[2].shape == (K, B)
    for name, got, want, first in (("logits", out[0], ref_out[0], 0), ("value", out[1], ref_out[1], 0),
                                   ("reward", out[2], ref_out[2], 1)):
        if want is None:
            continue
        for i in range(want.shape[0]):
            err = (got[i] - want[i]).abs().max().item()
            print(f"{name}[{i + first}] max |diff| {err:.3g}, max |ref| {want[i].abs().max().item():.3g}")
            torch.testing.assert_close(got[i], want[i], atol=1e-5, rtol=1e-5, msg=lambda m: f"{name}[{i + first}]: {m}")
    print("loss", loss, ref_loss)
    assert loss == pytest.approx(ref_loss, rel=1e-5)
    assert set(g) == set(ref_g) and len(g) == 22
    for k, want in ref_g.items():
        if want is None:                                   # K = 0: the dynamics take no part, as autograd
            assert K == 0 and k.startswith("dynamics.") and g[k] is None, k
            continue
        assert g[k] is not None and g[k].shape == want.shape, k
        print(f"{k}: max |diff| {(g[k] - want).abs().max().item():.3g}, max |ref| {want.abs().max().item():.3g}")
        np.testing.assert_allclose(g[k].cpu().numpy(), want.cpu().numpy(), rtol=1e-3,
                                   atol=1e-5 * max(1.0, want.abs().max().item()), err_msg=k)
    if K:
        ge = g["dynamics.action_embedding.weight"]
        assert ge.shape == (rows, C)                       # a full-size gradient for a table larger than the board
        assert (ge[UNUSED_ROW] == 0).all() and (ref_g["dynamics.action_embedding.weight"][UNUSED_ROW] == 0).all()
        assert ge[3].abs().max().item() > 0
        used = set(_inputs(N, B, K, rows)[1].unique().tolist())
        unused = [row for row in range(rows) if row not in used]
        assert UNUSED_ROW in unused and (ge[unused] == 0).all()


def _dyn_forward_hip(x, act, emb, w, b):
    """relu(conv3x3(x + emb[act]) + b) on the kernel the unroll's chain runs."""
    from mzgo._lib import check, lib, ptr, stream_of
    B, C, N, _ = x.shape
    y = torch.empty_like(x)
    check(lib.mzgo_conv3x3_relu_forward(ptr(x), ptr(act), ptr(emb), ptr(w), ptr(b), B, C, C, N, ptr(y),
                                        stream_of(x.device)))
    return y


def test_dynamics_weight_gradient_is_the_sum_of_the_per_step_calls():
    """Composition: the dynamics conv's weight (and bias) gradient from the
    unroll's single pass over the K B = 90 boards (11 full 8-board chunks and
    a ragged one of 2) equals the sum of K ``dyn_conv_backward_hip`` calls on
    the per-step tensors -- the latents rebuilt on the same forward kernels,
    each step's latent gradient = its heads' part (torch autograd on the
    detached latent) + the next step's input gradient.  1e-4 + 1e-4 |ref|,
    the per-layer bar; not bit-equal, the chunk order differs."""
    from mzgo.trainer import (_prediction, conv3x3_forward_hip, dyn_conv_backward_hip)
    N, C, B, K, rows = CASES[1]
    assert (K * B) % 8 != 0
    _, _, g = _run_unroll(N, C, B, K, rows)
    net = _net(N, C, rows)
    obs, acts = _inputs(N, B, K, rows)
    r, d = net.representation, net.dynamics
    emb, w, bias = (t.detach() for t in (d.action_embedding.weight, d.conv.weight, d.conv.bias))
    x = conv3x3_forward_hip(obs, r.conv1.weight, r.conv1.bias)
    x = conv3x3_forward_hip(x, r.conv2.weight, r.conv2.bias)
    lat = [conv3x3_forward_hip(x, r.conv3.weight, r.conv3.bias)]
    for k in range(K):
        lat.append(_dyn_forward_hip(lat[-1], acts[:, k].contiguous(), emb, w, bias))
    heads = []
    for k, x in enumerate(lat):                           # each latent's gradient from its own heads
        x = x.clone().requires_grad_()
        value, logits = _prediction(net, x)
        loss = (value ** 2).sum() + logits.logsumexp(1).sum() if k == 0 else (value * 0.5).sum() + logits.logsumexp(1).sum()
        if k:
            rew = d.fc_reward_output(torch.relu(d.fc_reward_hidden(d.reward_conv(x).mean(dim=[2, 3]))))
            loss = loss + (rew ** 2).sum()
        heads.append(torch.autograd.grad(loss, x)[0])
    gw, gb, G = torch.zeros_like(w), torch.zeros_like(bias), heads[K]
    for s in range(K, 0, -1):
        gx, gw_s, gb_s = dyn_conv_backward_hip(G, lat[s], lat[s - 1], acts[:, s - 1].contiguous(), emb, w)
        gw += gw_s
        gb += gb_s
        G = heads[s - 1] + gx
    print("gw max |diff|", (g["dynamics.conv.weight"] - gw).abs().max().item(), "max |ref|", gw.abs().max().item())
    torch.testing.assert_close(g["dynamics.conv.weight"], gw, atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(g["dynamics.conv.bias"], gb, atol=1e-4, rtol=1e-4)


def test_repeats_are_bit_equal_and_calls_do_not_share_buffers():
    import mzgo
    N, C, B, K, rows = CASES[0]
    out_a, loss_a, g_a = _run_unroll(N, C, B, K, rows)
    out_b, loss_b, g_b = _run_unroll(N, C, B, K, rows)
    assert loss_a == loss_b
    for a, b in zip(out_a, out_b):
        assert torch.equal(a, b)
    assert len(g_a) == 22
    for k in g_a:
        assert torch.equal(g_a[k], g_b[k]), k
    # a second unroll (other inputs) between the first one's forward and its backward
    net = _net(N, C, rows)
    obs, acts = _inputs(N, B, K, rows)
    first = mzgo.unroll(net, obs, acts)
    second = mzgo.unroll(net, obs.flip(0).contiguous(), acts.roll(1, 1).contiguous())
    assert not torch.equal(second[0], first[0])
    _mixed_loss(*first).backward()
    g_c = _grads(net)
    for k in g_a:
        assert torch.equal(g_a[k], g_c[k]), k
    for a, b in zip(out_a, first):
        assert torch.equal(a, b.detach())
    net.zero_grad()
    _mixed_loss(*second).backward()                       # and the second one's own backward still runs
    assert not torch.equal(net.dynamics.conv.weight.grad, g_a["dynamics.conv.weight"])
    # the backward builds no graph: differentiating it again is an error, not silently graph-less gradients
    w = net.prediction.value_fc.weight
    (gw,) = torch.autograd.grad(_mixed_loss(*mzgo.unroll(net, obs, acts)), w, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gw.sum().backward()


# ---------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------
def _compare_steps(tr_on, tr_off):
    for k in ("training_loss", "value_loss", "policy_loss", "reward_loss"):
        print(k, tr_on.last[k], tr_off.last[k])
        assert tr_on.last[k] == pytest.approx(tr_off.last[k], rel=1e-5, abs=1e-7), k
    for (name, a), b in zip(tr_on.net.named_parameters(), tr_off.net.parameters()):
        assert a.grad is not None and b.grad is not None, name
        np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.cpu().numpy(), rtol=1e-3,
                                   atol=1e-5 * max(1.0, b.grad.abs().max().item()), err_msg=name)
        assert torch.equal(a.detach(), b.detach()), name               # learning rate 0


@pytest.mark.parametrize("fused_loss", [False, True])
@pytest.mark.parametrize("N,C", [(5, 32), (6, 64)])
def test_trainer_step_gradients_with_and_without_fused_unroll(N, C, fused_loss):
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    from test_gpu_replay import _net as net_of, _store, _trajs
    trajs = _trajs(N)
    rp = _store(N, trajs)
    idx = np.arange(len(trajs))
    starts = np.array([len(t["actions"]) // 3 for t in trajs])
    # the targets are data to the step; their bootstrap values come from an engine, which is built for 5x5 at
    # latent_dim 96 only, so a 96-wide net supplies them there
    helper = MuZeroTrainer(net_of(N, 96 if N == 5 else C), TrainConfig(unroll_steps=4), mode="batched")
    targets = helper.device_targets(rp, idx, starts)
    trs = []
    for on in (True, False):
        cfg = TrainConfig(unroll_steps=4, learning_rate=0.0, max_grad_norm=1e9, fused_loss=fused_loss, fused_unroll=on)
        tr = MuZeroTrainer(net_of(N, C), cfg, mode="batched")
        tr._unroll_step(*targets, device_totals=True)
        trs.append(tr)
    _compare_steps(*trs)


def test_trainer_step_gradients_with_importance_weights():
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    from test_gpu_replay import _net as net_of
    from test_gpu_replay_sample import _trainer_setup
    trs = []
    for on in (True, False):
        N, C, rp = _trainer_setup()                        # a store of its own: a step rewrites the priorities
        cfg = TrainConfig(unroll_steps=3, learning_rate=0.0, max_grad_norm=1e9, device_sampling=True,
                          importance_beta=0.5, fused_loss=True, fused_unroll=on)
        tr = MuZeroTrainer(net_of(N, C), cfg, mode="batched", sample_seed=9)
        assert rp.sample(8, seed=9, step=0, beta=0.5)["weight"].min().item() < 0.9
        assert tr.train(rp, 8) is not None
        trs.append(tr)
    _compare_steps(*trs)


def test_short_run_with_every_switch_on(monkeypatch):
    """Three steps of ``train`` from a ``DeviceReplay`` with device_sampling,
    deferred_stats, fused_loss, device_weights and fused_unroll on: finite
    losses, moving parameters, engines that see the new weights, and two
    trainers from the same state that stay bit-equal -- the raw gradients (as
    ``clip_grad_norm_`` receives them) at every step, and the parameters
    after the three steps."""
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig, initial_inference_torch
    from test_gpu_replay import _net as net_of
    from test_gpu_replay_sample import _trainer_setup
    clip = torch.nn.utils.clip_grad_norm_
    seen = []

    def recording_clip(params, **kw):
        params = list(params)
        seen[-1].append([p.grad.detach().clone() for p in params])
        return clip(params, **kw)

    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", recording_clip)
    runs = []
    for _ in range(2):
        N, C, rp = _trainer_setup()                        # 5x5 / 96: the engines are built for 5x5 at 96 only
        net = net_of(N, C)
        before = {k: v.clone() for k, v in net.state_dict().items()}
        cfg = TrainConfig(unroll_steps=5, device_sampling=True, deferred_stats=True, fused_loss=True,
                          device_weights=True, fused_unroll=True)
        tr = MuZeroTrainer(net, cfg, mode="batched", sample_seed=3)
        seen.append([])
        losses = []
        for _ in range(3):
            out = tr.train(rp, 8)
            assert isinstance(out, torch.Tensor) and out.is_cuda
            losses.append(tr.read_stats()["training_loss"])
        assert all(np.isfinite(x) for x in losses), losses
        assert any(not torch.equal(before[k], v) for k, v in net.state_dict().items())
        runs.append((net, losses))
    monkeypatch.undo()
    (net_a, losses_a), (net_b, losses_b) = runs
    # the engine's next inference runs the trained weights
    obs = _inputs(5, 7, 3, 26)[0]
    with torch.no_grad():
        _, v_hip, lg_hip = net_a.initial_inference(obs)
        _, v_t, lg_t = initial_inference_torch(net_a, obs)
        _, v_old, _ = initial_inference_torch(net_of(5, 96), obs)
    torch.testing.assert_close(v_hip, v_t, atol=1e-5, rtol=0)
    torch.testing.assert_close(lg_hip, lg_t, atol=1e-5, rtol=1e-5)
    assert not torch.allclose(v_t, v_old, atol=1e-5, rtol=0)
    # two trainers from the same state
    assert len(seen[0]) == len(seen[1]) == 3
    for step, (ga, gb) in enumerate(zip(*seen)):
        assert len(ga) == 22
        for (name, _), a, b in zip(net_a.named_parameters(), ga, gb):
            assert torch.equal(a, b), (step, name)
    assert losses_a == losses_b
    for (k, a), b in zip(net_a.state_dict().items(), net_b.state_dict().values()):
        assert torch.equal(a, b), k
