"""The fused unroll (``mzgo.unroll``, csrc/mzgo_unroll.hip) at the shapes its
kernels make special, against float64 (tests/f64_reference.py):

(a) outputs, loss and all 22 gradients of ``mixed_loss`` end to end under
    ``check_bar`` (tests/test_unroll.py's bar: 4x torch-float32's own distance
    to float64 plus 1e-6 * max(1, |ref|.max())), on boards smaller than one
    16-cell tile (2x2: k_unroll_heads' G = 64 groups, 48 of them empty at
    C = 16; 3x3), exactly one, four and sixteen tiles (4x4, 8x8, 16x16 -- 256
    cells, where G = max(1, 256 / CELLS) reaches 1), one cell short of sixteen
    tiles' worth of threads (15x15: 225 cells, G = 1 with idle threads), ragged
    tiles (7x7, 13x13) and a latent width that is no multiple of 64 (C = 160).
    End to end the ReLU masks are not inputs, so each case's seed was chosen on
    the CPU such that the float64 graph's smallest |pre-activation| is at least
    1e-5, ten times the 1e-6 layer error tests/test_gpu_unroll.py's docstring
    derives (tests/test_unroll_edge_cases.py asserts it).
(b) the dynamics conv's weight pass with more than 8 boards per chunk -- the
    path main.py's sizes take and no other test runs -- against the sum of
    the per-step ``dyn_conv_backward_hip`` calls, the construction and the bar
    (1e-4 + 1e-4 |ref|) of tests/test_gpu_unroll.py's
    ``test_dynamics_weight_gradient_is_the_sum_of_the_per_step_calls``.
(c) a loss that ignores the reward at K > 0: the six reward-head gradients
    and nothing else are exactly 0, the rest stay under the bar.
"""
import functools

import numpy as np
import pytest
import torch

from f64_reference import check_bar, loss_without_reward, mixed_loss, unroll_reference

pytestmark = pytest.mark.gpu

MIN_PRE = 1e-5
# (N, C, B, K, embedding rows, seed): the smallest seed >= 0 whose float64 graph keeps every ReLU input at least
# MIN_PRE from 0
CASES = [(2, 16, 1, 1, 5, 0), (3, 48, 3, 2, 12, 2), (4, 16, 2, 2, 17, 0), (8, 32, 1, 1, 65, 2), (7, 160, 1, 1, 50, 20),
         (13, 48, 1, 1, 170, 35), (16, 16, 1, 0, 257, 7), (15, 16, 1, 0, 226, 8)]
# (N, C, B, K, embedding rows): main.py's batch and width on 4-cell boards (1280 boards, 24 per chunk: 53 full
# chunks and one of 8), and 369 = 8 * 46 + 1 = 16 * 23 + 1 boards at 16 per chunk (a last chunk of one board)
WIDE_CASES = [(2, 128, 128, 10, 37), (2, 160, 41, 9, 37)]
NO_REWARD_CASE = CASES[1]
REWARD_HEAD = ("dynamics.reward_conv.weight", "dynamics.reward_conv.bias", "dynamics.fc_reward_hidden.weight",
               "dynamics.fc_reward_hidden.bias", "dynamics.fc_reward_output.weight", "dynamics.fc_reward_output.bias")


def build_net(N, C, rows, seed):
    import mzgo
    net = mzgo.MuZeroNet(C, rows, board_size=N if rows != N * N + 1 else None)
    net.load_state_dict(mzgo.deterministic_state_dict(C, rows, seed))
    return net


@functools.lru_cache(maxsize=None)
def make_inputs(N, B, K, rows, seed):
    """Observations (binary planes) and actions over the whole table, CPU
    tensors; where there is room (K B >= 2) the pass, the last row of a table
    larger than the board, and (K B >= 4) one action twice within a step or
    across steps."""
    gen = torch.Generator().manual_seed(1000 * seed + 10 * N + B + K)
    obs = (torch.rand(B, 6, N, N, generator=gen) < 0.3).float()
    if K == 0:
        return obs, None
    acts = torch.randint(0, rows, (B, K), generator=gen)
    if K * B >= 2:
        acts[B - 1, K - 1] = N * N                         # the pass
        if rows > N * N + 1:
            acts[0, 0] = rows - 1
    if K * B >= 4:
        flat = acts.view(-1)                               # (sample-major: [0, 1] when K > 1, else [1, 0])
        flat[1] = 3
        flat[2] = 3
    return obs, acts


@functools.lru_cache(maxsize=None)
def references(N, C, B, K, rows, seed, loss_fn=mixed_loss):
    """(torch float32, float64) on the CPU, once per case."""
    net = build_net(N, C, rows, seed)
    obs, acts = make_inputs(N, B, K, rows, seed)
    return tuple(unroll_reference(net, obs, acts, dtype, loss_fn) for dtype in (torch.float32, torch.float64))


def _run_unroll(N, C, B, K, rows, seed, loss_fn=mixed_loss):
    import mzgo
    net = build_net(N, C, rows, seed).cuda()
    obs, acts = make_inputs(N, B, K, rows, seed)
    out = mzgo.unroll(net, obs.cuda(), None if acts is None else acts.cuda())
    loss = loss_fn(*out)
    loss.backward()
    grads = {k: None if p.grad is None else p.grad.detach().clone() for k, p in net.named_parameters()}
    return out, loss.detach(), grads


def _check_against(ref32, ref64, out, loss, grads, K, zero=()):
    for name, got in zip(("logits", "value", "reward"), out):
        if ref64[name] is None:
            assert got is None and K == 0 and name == "reward"
            continue
        check_bar(name, got, ref32[name], ref64[name])
    check_bar("loss", loss, ref32["loss"], ref64["loss"])
    assert set(grads) == set(ref64["grads"]) and len(grads) == 22
    for k, want in ref64["grads"].items():
        if k in zero:
            continue
        if want is None:                                   # K = 0: the dynamics take no part, as autograd
            assert K == 0 and k.startswith("dynamics.") and grads[k] is None, k
            continue
        assert grads[k] is not None, k
        check_bar(k, grads[k], ref32["grads"][k], want)


@pytest.mark.parametrize("N,C,B,K,rows,seed", CASES)
def test_unroll_against_float64(N, C, B, K, rows, seed):
    ref32, ref64 = references(N, C, B, K, rows, seed)
    assert ref64["min_pre"] >= MIN_PRE, ref64["min_pre"]
    out, loss, grads = _run_unroll(N, C, B, K, rows, seed)
    A = N * N + 1
    assert out[0].shape == (K + 1, B, A) and out[1].shape == (K + 1, B)
    _check_against(ref32, ref64, out, loss, grads, K)
    if K:
        acts = make_inputs(N, B, K, rows, seed)[1]
        ge = grads["dynamics.action_embedding.weight"]
        assert ge.shape == (rows, C)
        unused = [r for r in range(rows) if r not in set(acts.view(-1).tolist())]
        assert (ge[unused] == 0).all() and (ge[acts.view(-1)].abs().amax(dim=1) > 0).all()


# ---------------------------------------------------------------------------
# (b) the wide weight pass
# ---------------------------------------------------------------------------
def dyn_chunk(B, K, C):
    """Boards per chunk of the dynamics' weight pass (mzgo.h, mzgo_unroll_backward (c)): 8, or the next multiple
    of 8 that keeps the ceil(K B / chunk) partials of C*C*9 floats within 32 MiB, at most all K B boards."""
    cb = 8
    while cb < K * B and -(-K * B // cb) * C * C * 36 > (32 << 20):
        cb += 8
    return cb


def work_bytes_at(B, K, C, N, cb):
    """``mzgo_unroll_workspace``'s work size if the dynamics' pass took ``cb`` boards per chunk."""
    pad64 = lambda n: (n + 63) // 64 * 64
    cells, S = N * N, K + 1
    partials = lambda boards, cin, cout, chunk: -(-boards // chunk) * cout * cin * 9
    conv = max(partials(B, 64, C, 8), partials(B, 64, 64, 8), partials(B, 6, 64, 8))
    if K:
        conv = max(conv, partials(K * B, C, C, cb))
    return 4 * (pad64(S * B * C * cells) + 2 * pad64(B * 64 * cells) + pad64(K * B * C * ((cells + 15) // 16)) +
                pad64(S * B * (3 * C + 64)) + pad64(conv))


def assert_wide(N, C, B, K, rows):
    """The shape's pass takes more than 8 boards per chunk, by the chunk formula and by the library's own size."""
    from mzgo.unroll import workspace_bytes
    cb = dyn_chunk(B, K, C)
    assert cb > 8 and cb < K * B
    work = workspace_bytes(B, K, C, N, rows)[1]
    assert work == work_bytes_at(B, K, C, N, cb) < work_bytes_at(B, K, C, N, 8)
    return cb


@pytest.mark.parametrize("N,C,B,K,rows", WIDE_CASES)
def test_wide_weight_pass_is_the_sum_of_the_per_step_calls(N, C, B, K, rows):
    from mzgo.trainer import _prediction, conv3x3_forward_hip, dyn_conv_backward_hip
    from test_gpu_conv_f64 import _forward_hip
    cb = assert_wide(N, C, B, K, rows)
    print("boards", K * B, "per chunk", cb, "last chunk", (K * B) % cb)
    if (N, C, B, K, rows) == WIDE_CASES[1]:
        assert (K * B) % 8 == 1 and (K * B) % cb == 1     # a ragged last chunk, of a single board
    _, _, g = _run_unroll(N, C, B, K, rows, 2)
    net = build_net(N, C, rows, 2).cuda()
    obs, acts = (t.cuda() for t in make_inputs(N, B, K, rows, 2))
    r, d = net.representation, net.dynamics
    emb, w, bias = (t.detach() for t in (d.action_embedding.weight, d.conv.weight, d.conv.bias))
    x = conv3x3_forward_hip(obs, r.conv1.weight, r.conv1.bias)
    x = conv3x3_forward_hip(x, r.conv2.weight, r.conv2.bias)
    lat = [conv3x3_forward_hip(x, r.conv3.weight, r.conv3.bias)]
    for k in range(K):
        lat.append(_forward_hip(lat[-1], w, bias, acts[:, k].contiguous(), emb))
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
    for name, got, want in (("gw", g["dynamics.conv.weight"], gw), ("gb", g["dynamics.conv.bias"], gb)):
        print(name, "max |diff|", (got - want).abs().max().item(), "max |ref|", want.abs().max().item())
        assert want.abs().max().item() > 0
        torch.testing.assert_close(got, want, atol=1e-4, rtol=1e-4)


# ---------------------------------------------------------------------------
# (c) a loss without the reward
# ---------------------------------------------------------------------------
def test_loss_that_ignores_the_reward():
    N, C, B, K, rows, seed = NO_REWARD_CASE
    assert K > 0
    ref32, ref64 = references(N, C, B, K, rows, seed, loss_without_reward)
    out, loss, grads = _run_unroll(N, C, B, K, rows, seed, loss_without_reward)
    for k in REWARD_HEAD:                                  # autograd gives the unused head no gradient at all
        assert ref64["grads"][k] is None, k
    _check_against(ref32, ref64, out, loss, grads, K, zero=REWARD_HEAD)
    for k, g in grads.items():
        if k in REWARD_HEAD:
            assert g is not None and (g == 0).all(), k
        else:
            assert np.count_nonzero(g.cpu().numpy()) > 0, k
