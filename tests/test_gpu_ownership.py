"""The ownership auxiliary target on the GPU: the store's targets
(``DeviceReplay.ownership`` / ``ownership_from``, csrc/mzgo_replay.hip
k_replay_ownership) against ``mzgo.ownership_targets_host`` bit for bit, and
the head's loss (``mzgo.ownership_loss``, csrc/mzgo_ownership.hip) against
``mzgo.ownership_loss_host`` under ``f64_reference.check_bar`` with torch
float32 as the bar's own term.
"""
import functools

import numpy as np
import pytest
import torch

import mzgo
from f64_reference import check_bar
from test_ownership import hand_boards, loss_inputs, spiral_board, torch_loss

pytestmark = pytest.mark.gpu

K = 2


def game(final, moves, ended=True, first_white=False):
    """A main.py-format trajectory of ``moves`` moves that ends on the board ``final`` (int8 [N, N]): the boards
    before it are empty, the colours alternate, and only the last position carries the done plane."""
    N = final.shape[0]
    A = N * N + 1
    obs = []
    for t in range(moves + 1):
        o = np.zeros((6, N, N))
        o[2] = (t + first_white) % 2
        if t == moves:
            o[0], o[1] = final == 1, final == 2
            o[5] = float(ended)
        obs.append(o)
    return dict(observations=obs + [obs[-1].copy()], actions=[N * N] * moves, policies=[np.full(A, 1.0 / A)] * moves,
                rewards=[0.0] * moves + [1.0 if ended else 0.0])


@functools.lru_cache(maxsize=None)
def store_games(N):
    """Four games (the store's capacity): the hand-made final boards, one of them unfinished."""
    rng = np.random.default_rng(N)
    if N == 5:
        b = hand_boards()
        finals = [b["dame"], b["one colour"], b["empty"], b["dame"]]
    else:
        rand = ((rng.random((N, N)) < 0.45) * rng.integers(1, 3, (N, N))).astype(np.int8)
        mouth = spiral_board(N)
        mouth[0, 0] = 2
        finals = [spiral_board(N), rand, mouth, rand]
    return [game(finals[0], 5), game(finals[1], 3, first_white=True), game(finals[2], 4),
            game(finals[3], 6, ended=False)]


def build_store(N):
    rp = mzgo.DeviceReplay(N, 4, 8, "cuda")
    for g in store_games(N):
        rp.add(g)
    return rp


def host_targets(N, index, start, sym):
    g = store_games(N)[index]
    T = len(g["actions"])
    stones, _, flags = mzgo.positions_from_planes(np.asarray(g["observations"][:T + 1]))
    return mzgo.ownership_targets_host(stones[T].numpy(), flags.numpy(), N, start, K, sym)


@pytest.mark.parametrize("N", [5, 19])
def test_store_targets_are_the_host_rule_bit_for_bit(N):
    rp = build_store(N)
    # every game; starts at the front, in the middle and with start + K past the final board; all eight symmetries
    indices = [0, 0, 1, 1, 2, 2, 3, 3]
    starts = [0, 4, 0, 2, 1, 3, 0, 5]
    syms = list(range(8))
    t_own, mask = rp.ownership(indices, starts, K, syms)
    assert t_own.shape == (8, K + 1, N * N) and mask.shape == (8, K + 1) and t_own.dtype == torch.float32
    want = [host_targets(N, i, s, y) for i, s, y in zip(indices, starts, syms)]
    want_t, want_m = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    np.testing.assert_array_equal(t_own.cpu().numpy(), want_t)
    np.testing.assert_array_equal(mask.cpu().numpy(), want_m)
    assert (want_m[6:] == 0).all() and (want_t[6:] == 0).all()          # the unfinished game
    np.testing.assert_array_equal(want_m[1], [1, 1, 0])                    # game 0 has 5 moves: 4, 5, then past the end
    assert np.abs(want_t[0]).sum() > 0 and (want_t[0, 0] == -want_t[0, 1]).all()
    if N == 19:
        assert (np.abs(want_t[0, 0]) == 1).all()                           # the corridor converged: all one colour's
        assert (want_t[4, 0] == 0).sum() > 150                             # and with a white mouth it is nobody's
    # identity symmetries by default, and the device items' path
    a, _ = rp.ownership(indices, starts, K)
    b, _ = rp.ownership(indices, starts, K, [0] * 8)
    assert torch.equal(a, b)
    size = 4
    items = torch.tensor([[i % size, s, y] for i, s, y in zip(indices, starts, syms)], dtype=torch.int32, device="cuda")
    t2, m2 = rp.ownership_from(dict(items=items), K)       # (nothing evicted: slot = logical index)
    assert torch.equal(t2, t_own) and torch.equal(m2, mask)
    t3, m3 = rp.ownership_from(items, K)
    assert torch.equal(t3, t_own) and torch.equal(m3, mask)


def test_store_targets_follow_the_sampler():
    rp = build_store(5)
    s = rp.sample(3, seed=3, step=0, symmetries=True)
    t_own, mask = rp.ownership_from(s, K)
    items = s["items"].cpu().numpy()
    for b, (slot, start, sym) in enumerate(items):
        want_t, want_m = host_targets(5, int(slot), int(start), int(sym))
        np.testing.assert_array_equal(t_own[b].cpu().numpy(), want_t)
        np.testing.assert_array_equal(mask[b].cpu().numpy(), want_m)


# ---------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------
LOSS_SHAPES = [(2, 16, 1, 0), (5, 48, 3, 2), (9, 128, 2, 1), (19, 16, 2, 1)]


def run_device(lat, w, bias, t_own, mask, g_per, weight):
    head = mzgo.OwnershipHead(w.numel()).cuda()
    with torch.no_grad():
        head.conv.weight.copy_(w.view(1, -1, 1, 1))
        head.conv.bias.copy_(bias)
    lat = lat.cuda().requires_grad_()
    per, total = mzgo.ownership_loss(lat, head, t_own.cuda(), mask.cuda(), weight)
    assert not total.requires_grad and total.dtype == torch.float64 and total.shape == (1,)
    (per * g_per.cuda()).sum().backward()
    return dict(per=per.detach(), total=total[0], g_latents=lat.grad, g_w=head.conv.weight.grad.view(-1),
                g_bias=head.conv.bias.grad)


@pytest.mark.parametrize("N,C,B,K", LOSS_SHAPES)
def test_loss_against_the_host_twin(N, C, B, K):
    weight = 0.7
    lat, w, bias, t_own, mask, g_per = loss_inputs(N, C, B, K)
    host = mzgo.ownership_loss_host(lat.numpy(), w.numpy(), bias.numpy(), t_own.numpy(), mask.numpy(), weight,
                                    g_per.numpy())
    ref32 = dict(zip(("per", "total", "g_latents", "g_w", "g_bias"),
                     torch_loss(lat, w, bias, t_own, mask, g_per, weight, torch.float32)))
    got = run_device(lat, w, bias, t_own, mask, g_per, weight)
    for k in ("per", "total", "g_latents", "g_w", "g_bias"):
        check_bar(k, got[k], ref32[k], np.asarray(host[k], dtype=np.float64).reshape(ref32[k].shape))
    again = run_device(lat, w, bias, t_own, mask, g_per, weight)
    for k in got:
        assert torch.equal(got[k], again[k]), k             # two calls give the same bits
    if B * (K + 1) > 1:                                     # the row without a target: exact zeros
        assert (got["g_latents"][K, B - 1] == 0).all()


def test_a_non_uniform_g_per_scales_each_sample():
    N, C, B, K = 5, 48, 3, 2
    lat, w, bias, t_own, mask, _ = loss_inputs(N, C, B, K)
    ones = run_device(lat, w, bias, t_own, mask, torch.ones(B), 1.0)
    g_per = torch.tensor([2.0, 0.0, -0.5])                  # powers of two: the scaling is exact in float32
    got = run_device(lat, w, bias, t_own, mask, g_per, 1.0)
    assert torch.equal(got["per"], ones["per"])
    for b in range(B):
        assert torch.equal(got["g_latents"][:, b], ones["g_latents"][:, b] * g_per[b]), b
    # the head's gradients are the samples' contributions under the same weights
    parts = [run_device(lat, w, bias, t_own, mask, torch.eye(B)[b], 1.0) for b in range(B)]
    for k in ("g_w", "g_bias"):
        want = sum(g_per[b].item() * parts[b][k].double() for b in range(B))
        torch.testing.assert_close(got[k].double(), want, rtol=1e-5, atol=1e-7)


def test_an_all_zero_mask_and_large_logits():
    N, C, B, K = 5, 16, 2, 1
    lat, w, bias, t_own, mask, g_per = loss_inputs(N, C, B, K, big=True)
    got = run_device(lat, w, bias, t_own, torch.zeros_like(mask), g_per, 1.0)
    assert got["total"].item() == 0.0
    for k in ("per", "g_latents", "g_w", "g_bias"):
        assert (got[k] == 0).all(), k
    got = run_device(lat, w, bias, t_own, mask, torch.ones(B), 0.5)
    host = mzgo.ownership_loss_host(lat.numpy(), w.numpy(), bias.numpy(), t_own.numpy(), mask.numpy(), 0.5)
    assert all(torch.isfinite(v).all() for v in got.values())
    # at logits of +-40 tanh is +-1 on both sides: sample 0's first row is the host's, bit for bit
    np.testing.assert_array_equal(got["g_latents"][0, 0].cpu().numpy(), host["g_latents"][0, 0])
