"""The ownership auxiliary target without a GPU: the owner map of a final
board (``mzgo.ownership_host``: the kernel's fixed-point rule) against a
numpy / ``scipy.ndimage.label`` flood fill and ``oracle.gogame.areas``; the
per-sample targets (``mzgo.ownership_targets_host``: turn bit, game end,
symmetries); the head's loss and gradients (``mzgo.ownership_loss_host``)
against torch autograd in float64 under ``f64_reference.check_bar``; and the
configurations the trainer and ``mzgo.unroll`` refuse.
"""
import numpy as np
import pytest
import torch
from scipy import ndimage

import mzgo
from f64_reference import check_bar
from mzgo.trainer import MuZeroTrainer, TrainConfig
from oracle import gogame


# ---------------------------------------------------------------------------
# the owner map
# ---------------------------------------------------------------------------
def owner_reference(stones):
    """0 / 1 / 2 per cell: a stone's colour; an empty region's one bordering colour, else 0."""
    stones = np.asarray(stones)
    owner = stones.astype(np.int8).copy()
    regions, n = ndimage.label(stones == 0)
    for lab in range(1, n + 1):
        region = regions == lab
        rim = ndimage.binary_dilation(region) & ~region
        colours = set(np.unique(stones[rim]).tolist()) - {0}
        owner[region] = colours.pop() if len(colours) == 1 else 0
    return owner


def oracle_counts(stones):
    state = np.zeros((6, *stones.shape))
    state[gogame.BLACK], state[gogame.WHITE] = stones == 1, stones == 2
    return tuple(int(x) for x in gogame.areas(state))


def spiral_board(N=19, wall=1):
    """A one-cell-wide corridor of empties spiralling to the centre, walled by one colour."""
    b = np.full((N, N), wall, np.int8)
    i, j, di, dj = 0, 0, 0, 1
    b[0, 0] = 0
    while True:
        for _ in range(4):                                # go on, or turn (at most three times) and go on
            ni, nj, fi, fj = i + di, j + dj, i + 2 * di, j + 2 * dj
            if 0 <= ni < N and 0 <= nj < N and b[ni, nj] and not (0 <= fi < N and 0 <= fj < N and b[fi, fj] == 0):
                break
            di, dj = dj, -di
        else:
            return b
        i, j = ni, nj
        b[i, j] = 0


def hand_boards():
    dame = np.zeros((5, 5), np.int8)
    dame[:, 1], dame[:, 3] = 1, 2                          # column 0: black's, column 2: touches both, column 4: white's
    one = np.zeros((5, 5), np.int8)
    one[2, 2] = 2
    return {"empty": np.zeros((5, 5), np.int8), "one colour": one, "dame": dame, "spiral": spiral_board()}


def check_owner(stones):
    N = stones.shape[0]
    got = mzgo.ownership_host(stones, N)
    assert got.dtype == np.int8 and got.shape == (N, N)
    np.testing.assert_array_equal(got, owner_reference(stones))
    assert ((got == 1).sum(), (got == 2).sum()) == oracle_counts(stones)
    return got


@pytest.mark.parametrize("N", [2, 3, 5, 9, 19])
def test_owner_map_on_random_boards(N):
    rng = np.random.default_rng(N)
    for density in (0.05, 0.2, 0.5, 0.8, 0.97):
        for _ in range(6):
            stones = (rng.random((N, N)) < density) * rng.integers(1, 3, (N, N))
            check_owner(stones.astype(np.int8))


def test_owner_map_on_hand_made_boards():
    boards = hand_boards()
    assert (check_owner(boards["empty"]) == 0).all()
    assert (check_owner(boards["one colour"]) == 2).all()
    dame = check_owner(boards["dame"])
    assert (dame[:, 0] == 1).all() and (dame[:, 2] == 0).all() and (dame[:, 4] == 2).all()
    spiral = boards["spiral"]
    regions, n = ndimage.label(spiral == 0)
    assert n == 1 and (spiral == 0).sum() > 150            # one corridor, far longer than the board is wide
    assert (check_owner(spiral) == 1).all()
    spiral[0, 0] = 2                                       # a white stone at the mouth: the corridor is nobody's
    got = check_owner(spiral)
    assert (got[spiral == 0] == 0).all()


# ---------------------------------------------------------------------------
# the targets of a sample
# ---------------------------------------------------------------------------
def test_targets_follow_the_turn_bit_and_the_game_end():
    N, K = 5, 3
    final = hand_boards()["dame"]
    owner = mzgo.ownership_host(final, N).reshape(-1)
    flags = np.array([0, 1, 0, 1, 0, 1, 4], np.uint8)      # L = 6; black moves first; the final row: ended
    L = len(flags) - 1
    t_own, mask = mzgo.ownership_targets_host(final, flags, N, 1, K)
    assert t_own.shape == (K + 1, N * N) and t_own.dtype == np.float32 and (mask == 1).all()
    for k in range(K + 1):
        mover = 1 + (flags[1 + k] & 1)
        want = np.where(owner == 0, 0.0, np.where(owner == mover, 1.0, -1.0))
        np.testing.assert_array_equal(t_own[k], want)
    np.testing.assert_array_equal(t_own[0], -t_own[1])     # the sign flips with the turn
    np.testing.assert_array_equal(t_own[1], -t_own[2])
    assert set(np.unique(t_own)) == {-1.0, 0.0, 1.0}
    # start + k past the final board: zeros with mask 0
    t_own, mask = mzgo.ownership_targets_host(final, flags, N, L - 1, K)
    np.testing.assert_array_equal(mask, [1, 1, 0, 0])
    assert (t_own[2:] == 0).all() and np.abs(t_own[:2]).sum() > 0
    # the final row's own turn bit is read at at = L
    flags_w = flags.copy()
    flags_w[L] |= 1
    a, _ = mzgo.ownership_targets_host(final, flags, N, L, 0)
    b, _ = mzgo.ownership_targets_host(final, flags_w, N, L, 0)
    np.testing.assert_array_equal(a, -b)
    # an unfinished game (the move cap): no target anywhere
    flags_cut = flags.copy()
    flags_cut[L] = 2
    t_own, mask = mzgo.ownership_targets_host(final, flags_cut, N, 0, K)
    assert (mask == 0).all() and (t_own == 0).all()


@pytest.mark.parametrize("N", [5, 19])
def test_targets_under_the_eight_symmetries(N):
    rng = np.random.default_rng(N)
    final = ((rng.random((N, N)) < 0.4) * rng.integers(1, 3, (N, N))).astype(np.int8)
    flags = np.array([0, 1, 0, 1 | 4], np.uint8)
    base, _ = mzgo.ownership_targets_host(final, flags, N, 0, 3, 0)
    assert np.abs(base).sum() > 0
    seen = set()
    for s in range(8):
        got, mask = mzgo.ownership_targets_host(final, flags, N, 0, 3, s)
        want = np.rot90(base.reshape(4, N, N), s & 3, axes=(-2, -1))
        if s & 4:
            want = np.flip(want, axis=-1)
        np.testing.assert_array_equal(got, want.reshape(4, -1))
        assert (mask == 1).all()
        seen.add(got.tobytes())
    assert len(seen) == 8


# ---------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------
def loss_inputs(N, C, B, K, seed=0, big=False):
    g = torch.Generator().manual_seed(seed + 100 * N + C)
    lat = torch.relu(torch.randn(K + 1, B, C, N, N, generator=g))
    w = torch.randn(C, generator=g) * (0.5 / C ** 0.5)
    bias = torch.randn(1, generator=g) * 0.1
    t_own = torch.randint(-1, 2, (B, K + 1, N * N), generator=g).float()
    mask = torch.ones(B, K + 1)
    if B * (K + 1) > 1:
        mask[-1, -1] = 0                                   # one row without a target
    g_per = torch.rand(B, generator=g) + 0.5
    if big:                                                # logits of +-40 in sample 0's first row
        lat[0, 0] = 0
        lat[0, 0, 0].view(-1)[0::2] = 1
        lat[0, 0, 1].view(-1)[1::2] = 1
        w[0], w[1], bias[0] = 40.0, -40.0, 0.0
    return lat, w, bias, t_own, mask, g_per


def torch_loss(lat, w, bias, t_own, mask, g_per, weight, dtype):
    """The head and the loss with torch ops under autograd in ``dtype``: (per, total, g_lat, g_w, g_bias)."""
    lat, w, bias = (x.detach().to(dtype).requires_grad_() for x in (lat, w, bias))
    K1, B, C, N, _ = lat.shape
    x = torch.nn.functional.conv2d(lat.view(K1 * B, C, N, N), w.view(1, C, 1, 1), bias).view(K1, B, N * N)
    t = t_own.to(dtype).transpose(0, 1)
    cell = torch.logaddexp(torch.zeros_like(x), 2 * x) - (1 + t) * x       # softplus(2x), without overflow
    per = weight * (mask.to(dtype).t() * cell.mean(dim=2)).sum(dim=0)
    (per * g_per.to(dtype)).sum().backward()
    return per.detach(), per.detach().sum(), lat.grad, w.grad, bias.grad


LOSS_SHAPES = [(2, 16, 1, 0), (5, 48, 3, 2), (19, 16, 2, 1)]


@pytest.mark.parametrize("N,C,B,K", LOSS_SHAPES)
def test_loss_host_against_float64(N, C, B, K):
    weight = 0.7
    lat, w, bias, t_own, mask, g_per = loss_inputs(N, C, B, K)
    got = mzgo.ownership_loss_host(lat.numpy(), w.numpy(), bias.numpy(), t_own.numpy(), mask.numpy(), weight,
                                   g_per.numpy())
    ref32 = torch_loss(lat, w, bias, t_own, mask, g_per, weight, torch.float32)
    ref64 = torch_loss(lat, w, bias, t_own, mask, g_per, weight, torch.float64)
    for name, g, r32, r64 in zip(("per", "total", "g_latents", "g_w", "g_bias"),
                                 (got["per"], got["total"], got["g_latents"], got["g_w"], got["g_bias"]), ref32, ref64):
        check_bar(name, g, r32, r64)
    # g_x is the derivative of per.sum() with respect to the logits: g_latents = g_per w g_x
    want = g_per.numpy()[None, :, None, None] * w.numpy()[None, None, :, None] * got["g_x"][:, :, None, :]
    np.testing.assert_allclose(got["g_latents"].reshape(K + 1, B, C, N * N), want, rtol=1e-6, atol=0)
    if B * (K + 1) > 1:                                    # the masked row: exact zeros
        assert (got["g_x"][K, B - 1] == 0).all() and (got["g_latents"][K, B - 1] == 0).all()


def test_loss_host_at_large_logits():
    N, C, B, K, weight = 5, 16, 2, 1, 0.5
    lat, w, bias, t_own, mask, g_per = loss_inputs(N, C, B, K, big=True)
    got = mzgo.ownership_loss_host(lat.numpy(), w.numpy(), bias.numpy(), t_own.numpy(), mask.numpy(), weight)
    x = (lat[0, 0].double() * w.double()[:, None, None]).sum(0).view(-1) + bias.double()
    assert set(x.abs().tolist()) == {40.0}
    assert np.isfinite(got["per"]).all() and np.isfinite(got["total"]) and np.isfinite(got["g_latents"]).all()
    # tanh(+-40) is +-1 in float32: the gradient is exactly (weight * mask / CELLS) (tanh(x) - t)
    scale = np.float32(np.float32(weight) * np.float32(1.0)) / np.float32(N * N)
    want = scale * (np.tanh(x.numpy()).astype(np.float32) - t_own[0, 0].numpy())
    np.testing.assert_array_equal(got["g_x"][0, 0], want)
    ref64 = torch_loss(lat, w, bias, t_own, mask, torch.ones(B), weight, torch.float64)
    ref32 = torch_loss(lat, w, bias, t_own, mask, torch.ones(B), weight, torch.float32)
    check_bar("per", got["per"], ref32[0], ref64[0])


def test_loss_host_with_an_all_zero_mask():
    N, C, B, K = 5, 16, 3, 2
    lat, w, bias, t_own, mask, g_per = loss_inputs(N, C, B, K)
    got = mzgo.ownership_loss_host(lat.numpy(), w.numpy(), bias.numpy(), t_own.numpy(), np.zeros_like(mask.numpy()), 1.0,
                                   g_per.numpy())
    assert got["total"] == 0.0
    for k in ("per", "g_x", "g_latents", "g_w", "g_bias"):
        assert (got[k] == 0).all(), k


def test_head_forward_is_tanh_of_the_conv():
    head = mzgo.OwnershipHead(16)
    assert [k for k, _ in head.named_parameters()] == ["conv.weight", "conv.bias"]
    assert tuple(head.conv.weight.shape) == (1, 16, 1, 1)
    x = torch.randn(2, 16, 5, 5)
    torch.testing.assert_close(head(x), torch.tanh(torch.nn.functional.conv2d(x, head.conv.weight, head.conv.bias)))
    # the net keeps the reference's 22 tensors
    assert len(list(mzgo.MuZeroNet(16, 26).parameters())) == 22


# ---------------------------------------------------------------------------
# what is refused
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs,mode,match", [
    (dict(), "reference", "ownership_loss_weight needs mode='batched'"),
    (dict(fused_loss=True), "batched", "ownership_loss_weight needs fused_unroll=True"),
    (dict(fused_unroll=True), "batched", "ownership_loss_weight needs fused_loss=True"),
    (dict(fused_unroll=True, fused_loss=True), "batched", "ownership_loss_weight needs the net on the GPU"),
])
def test_ownership_loss_weight_is_refused_without_its_requirements(kwargs, mode, match):
    net = mzgo.MuZeroNet(16, 26)
    with pytest.raises(ValueError, match=match):
        MuZeroTrainer(net, TrainConfig(ownership_loss_weight=0.5, **kwargs), mode=mode)


def test_other_refusals():
    net = mzgo.MuZeroNet(16, 26)
    assert TrainConfig().ownership_loss_weight == 0.0
    assert MuZeroTrainer(net, TrainConfig()).ownership_head is None
    with pytest.raises(ValueError, match="ownership_loss_weight must be finite and >= 0"):
        MuZeroTrainer(net, TrainConfig(ownership_loss_weight=-1.0))
    with pytest.raises(ValueError, match="ownership_head belongs to ownership_loss_weight"):
        MuZeroTrainer(net, TrainConfig(), ownership_head=mzgo.OwnershipHead(16))
    obs = torch.zeros(1, 6, 5, 5)
    with pytest.raises(ValueError, match="mzgo.unroll runs on the GPU"):
        mzgo.unroll(net, obs, None, return_latents=True)
    with pytest.raises(ValueError, match="ownership_loss runs on the GPU"):
        mzgo.ownership_loss(torch.zeros(1, 1, 16, 5, 5), mzgo.OwnershipHead(16), torch.zeros(1, 1, 25),
                            torch.ones(1, 1))
