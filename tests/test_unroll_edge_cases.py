"""The inputs of tests/test_gpu_conv_f64.py and tests/test_gpu_unroll_edges.py
checked without a GPU: that alone they keep the float64 references within the
conditions those tests rely on.

* every end-to-end unroll case keeps each ReLU input of the float64 graph at
  least 1e-5 from 0 (so no float32 rounding flips a mask and the gradients
  are comparable), and torch float32 is inside the bar against float64;
* the planted edges of the conv cases are in the generated inputs, and have
  the consequences in the float64 reference that the GPU tests assert of the
  kernels;
* the chunk arithmetic of the wide weight pass holds, against the library's
  own workspace size.
"""
import pytest
import torch

import test_gpu_conv_f64 as conv
import test_gpu_unroll_edges as edges
from f64_reference import check_bar, loss_without_reward, mixed_loss


@pytest.mark.parametrize("N,C,B,K,rows,seed", edges.CASES)
def test_unroll_cases_keep_their_relu_inputs_away_from_zero(N, C, B, K, rows, seed):
    ref32, ref64 = edges.references(N, C, B, K, rows, seed)
    print("smallest |pre-activation|", ref64["min_pre"])
    assert ref64["min_pre"] >= edges.MIN_PRE
    for name in ("logits", "value", "reward", "loss"):
        if ref64[name] is not None:
            check_bar(name, ref32[name], ref32[name], ref64[name])
    n = 0
    for k, want in ref64["grads"].items():
        if want is None:
            assert K == 0 and k.startswith("dynamics.") and ref32["grads"][k] is None
            continue
        check_bar(k, ref32["grads"][k], ref32["grads"][k], want)
        n += 1
    assert n == (22 if K else 13)
    obs, acts = edges.make_inputs(N, B, K, rows, seed)
    assert obs.shape == (B, 6, N, N) and set(obs.unique().tolist()) <= {0.0, 1.0}
    if K:
        assert acts.shape == (B, K) and 0 <= acts.min().item() and acts.max().item() < rows
        if K * B >= 2:
            assert (acts == N * N).any()                   # the pass
            assert rows == N * N + 1 or (acts == rows - 1).any()
        if K * B >= 4:
            assert acts.view(-1).unique().numel() < K * B  # one action twice


def test_the_case_table_covers_the_special_boards():
    cells = {N * N for N, *_ in edges.CASES}
    assert {4, 9} <= cells                                 # less than one 16-cell tile
    assert {16, 64, 256} <= cells                          # exactly 1, 4 and 16 tiles; 256: k_unroll_heads' G reaches 1
    assert 225 in cells and any(c % 16 for c in cells)     # G = 1 with idle threads; ragged tiles
    assert any(256 // (N * N) > C for N, C, *_ in edges.CASES)            # empty channel groups (2x2, C = 16)
    assert any(C % 64 for _, C, *_ in edges.CASES) and any(K == 0 for *_, K, _, _ in edges.CASES)
    assert any(rows > N * N + 1 for N, _, _, _, rows, _ in edges.CASES)
    assert edges.NO_REWARD_CASE[3] > 0


def test_mixed_loss_is_test_gpu_unroll_s():
    from test_gpu_unroll import _mixed_loss
    gen = torch.Generator().manual_seed(0)
    logits, value, reward = (torch.randn(s, generator=gen, dtype=torch.float64) for s in ((3, 2, 10), (3, 2), (2, 2)))
    assert mixed_loss(logits, value, reward).item() == _mixed_loss(logits, value, reward).item()
    assert mixed_loss(logits[:1], value[:1], None).item() == _mixed_loss(logits[:1], value[:1], None).item()
    assert loss_without_reward(logits, value, reward).item() == _mixed_loss(logits, value, reward * 0).item()


@pytest.mark.parametrize("N,Cin,Cout,B", conv.CASES)
def test_conv_cases_hold_their_planted_edges(N, Cin, Cout, B):
    c = conv.make_case(N, Cin, Cout, B)
    dead, zero_board, zero_chan = conv.planted(N, Cin, Cout, B)
    rows = N * N + 1 + conv.EXTRA_ROWS
    assert c["emb"].shape == (rows, Cin) and rows > N * N + 1
    assert c["bias"][dead].item() == conv.DEAD_BIAS
    assert (zero_board is None) == (B < 2) and (zero_chan is None) == (Cin < 2)
    if zero_board is not None:
        assert (c["x"][zero_board] == 0).all()
    if zero_chan is not None:
        assert (c["x"][:, zero_chan] == 0).all()
    assert (c["x"] > 0).any() and (c["x"] >= 0).all()
    act = c["action"]
    assert act.shape == (B,) and 0 <= act.min().item() and act.max().item() < rows
    if B >= 2:
        assert (act == N * N).any() and (act == rows - 1).any()
    else:
        assert act.item() == (rows - 1 if N == 2 else N * N)
    if B >= 3:
        assert act.unique().numel() < B
    # what the edges mean, in float64: the GPU tests assert the same of the kernels
    for with_emb in (False, True):
        out, ref32, ref64 = conv.references(N, Cin, Cout, B, with_emb)
        assert out.dtype == torch.float32 and torch.equal(out > 0, ref64["y"] > 0)     # rounding flips no mask
        assert (ref64["y"][:, dead] == 0).all() and (ref64["y"] > 0).any()
        assert (ref64["gw"][dead] == 0).all() and ref64["gb"][dead].item() == 0
        for name in ("y", "gx", "gw", "gb"):
            check_bar(name, ref32[name], ref32[name], ref64[name])
    _, _, ref64 = conv.references(N, Cin, Cout, B, False)
    if zero_chan is not None:
        assert (ref64["gw"][:, zero_chan] == 0).all()
    if zero_board is not None:
        want = c["bias"].double().relu()[:, None, None].expand(Cout, N, N)
        assert torch.equal(ref64["y"][zero_board], want)


def test_the_conv_case_table_is_the_issue_s():
    assert sorted(conv.CASES) == sorted([(2, 6, 16, 1), (2, 6, 16, 9), (2, 16, 16, 1), (2, 16, 16, 9), (3, 5, 17, 8),
                                         (4, 1, 48, 17), (4, 48, 48, 17), (7, 64, 160, 3), (8, 17, 5, 8),
                                         (13, 48, 48, 2), (16, 16, 16, 1)])
    assert {B for *_, B in conv.CASES} >= {1, 8, 9, 17}   # around the weight pass's chunk of 8 boards


def test_wide_pass_chunk_arithmetic():
    """The shapes of tests/test_gpu_unroll_edges.py (b) put the dynamics'
    weight pass on more than 8 boards per chunk -- by the formula of mzgo.h
    and by ``mzgo_unroll_workspace``'s size, which only that chunk explains --
    and the largest shape another test runs does not."""
    from mzgo.unroll import workspace_bytes
    (N, C, B, K, rows), second = edges.WIDE_CASES
    assert (N, C, B, K) == (2, 128, 128, 10)               # main.py's batch and width on 4-cell boards
    assert edges.assert_wide(N, C, B, K, rows) == 24
    # 1280 boards: 160 chunks of 8 would be 94 MB of partials, 80 of 16 47 MB, 54 of 24 31.9 MB
    assert 54 * C * C * 36 <= (32 << 20) < 80 * C * C * 36
    N, C, B, K, rows = second
    assert edges.assert_wide(N, C, B, K, rows) == 16
    assert (K * B) % 8 == 1 and (K * B) % 16 == 1 and K * B == 369
    # the example of 43 samples and 7 steps at C = 160 has 301 = 8 * 37 + 5 boards: not of the form 8 m + 1
    assert (43 * 7) % 8 == 5 and edges.dyn_chunk(43, 7, 160) == 16
    # tests/test_gpu_unroll.py's largest: 90 boards, 8 per chunk
    assert edges.dyn_chunk(9, 10, 128) == 8
    assert workspace_bytes(9, 10, 128, 6, 37)[1] == edges.work_bytes_at(9, 10, 128, 6, 8)
    assert edges.dyn_chunk(4, 5, 1024) == 24               # a wide C: 8, 16, then one chunk of all 20 boards
