"""The trainer's conv layer kernels (csrc/mzgo_train.hip: k_conv_fwd,
k_conv_bwd_input, k_conv_bwd_weight, k_conv_bwd_reduce, k_conv_bwd_bias)
through ``conv3x3_forward_hip``, ``conv3x3_backward_hip``,
``dyn_conv_backward_hip`` and the embedding form of
``mzgo_conv3x3_relu_forward``, against float64 (tests/f64_reference.py) at the
shapes the 16-cell / 16-channel MFMA tiles and the 8-board weight chunk make
special.

Bar (tests/test_unroll.py's, ``check_bar``): the kernel's distance to the
float64 result is at most 4x torch-float32's own distance (CPU, same float32
inputs) plus 1e-6 * max(1, |ref|.max()).  The backward takes the float64
output rounded to float32 as the saved output, so the kernel and both
references use the same ReLU mask.

Planted in every case where the shape has room: a dead output channel (bias
-1e3), a board of zeros (B >= 2), an input channel of zeros (Cin >= 2); in the
dynamics form the pass action, the last row of a table larger than N*N + 1 and
an action taken twice (all three from B >= 3; B = 2: pass and last row; B = 1:
the last row at N = 2, the pass otherwise).  tests/test_unroll_edge_cases.py
asserts them on the CPU; their exact consequences are asserted here.  One
more test fills the weight pass's LDS rows with NaN from an earlier call and
asks the ragged boards for the same bits afterwards.
"""
import functools

import pytest
import torch

from f64_reference import check_bar, layer_backward_reference, layer_reference

pytestmark = pytest.mark.gpu

# (N, Cin, Cout, B)
CASES = [(2, 6, 16, 1), (2, 6, 16, 9), (2, 16, 16, 1), (2, 16, 16, 9),   # 4 cells: less than a tile, all corners
         (3, 5, 17, 8),       # one interior cell; a ragged k-step, a ragged cout tile of 1
         (4, 1, 48, 17), (4, 48, 48, 17),                                   # exactly one tile
         (7, 64, 160, 3),     # three tiles plus one cell
         (8, 17, 5, 8),       # exactly four tiles
         (13, 48, 48, 2),     # ten tiles plus nine cells
         (16, 16, 16, 1)]     # 256 cells
EXTRA_ROWS = 3                # embedding rows past the board's N*N + 1 actions
DEAD_BIAS = -1e3


def planted(N, Cin, Cout, B):
    """Where the edges sit: (dead output channel, zero board or None, zero input channel or None)."""
    return Cout // 2, (B // 2 if B >= 2 else None), (Cin // 2 if Cin >= 2 else None)


@functools.lru_cache(maxsize=None)
def make_case(N, Cin, Cout, B):
    """Float32 CPU tensors of one layer call: x (ReLU'd normal), w, bias, emb,
    action, g, with the edges of the module docstring planted."""
    gen = torch.Generator().manual_seed(N * 1000 + Cin * 7 + Cout + B)
    rows = N * N + 1 + EXTRA_ROWS
    x = torch.randn(B, Cin, N, N, generator=gen).relu()
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) / (3 * Cin ** 0.5)
    bias = torch.randn(Cout, generator=gen) * 0.1
    emb = torch.randn(rows, Cin, generator=gen)
    g = torch.randn(B, Cout, N, N, generator=gen)
    action = torch.randint(0, N * N, (B,), generator=gen)
    dead, zero_board, zero_chan = planted(N, Cin, Cout, B)
    bias[dead] = DEAD_BIAS
    if zero_board is not None:
        x[zero_board] = 0.0
    if zero_chan is not None:
        x[:, zero_chan] = 0.0
    if B == 1:
        action[0] = rows - 1 if N == 2 else N * N
    else:
        action[0] = N * N                                  # the pass
        action[B - 1] = rows - 1                           # the table's last row
        if B >= 3:
            action[1] = action[0]                          # one action twice
    return dict(x=x, w=w, bias=bias, emb=emb, action=action, g=g)


@functools.lru_cache(maxsize=None)
def references(N, Cin, Cout, B, with_emb):
    """Forward and backward in float64 and in torch float32, once per case;
    ``out`` is the float64 output rounded to float32 (the saved output every
    backward gets)."""
    c = make_case(N, Cin, Cout, B)
    res = {}
    for dtype in (torch.float64, torch.float32):
        t = {k: v if k == "action" else v.to(dtype) for k, v in c.items()}
        act, emb = (t["action"], t["emb"]) if with_emb else (None, None)
        res[dtype] = dict(y=layer_reference(t["x"], t["w"], t["bias"], act, emb))
    out = res[torch.float64]["y"].float()
    for dtype in (torch.float64, torch.float32):
        t = {k: v if k == "action" else v.to(dtype) for k, v in c.items()}
        act, emb = (t["action"], t["emb"]) if with_emb else (None, None)
        gx, gw, gb = layer_backward_reference(t["g"], out.to(dtype), t["x"], t["w"], act, emb)
        res[dtype].update(gx=gx, gw=gw, gb=gb)
    return out, res[torch.float32], res[torch.float64]


def _forward_hip(x, w, bias, action=None, emb=None):
    """``mzgo_conv3x3_relu_forward`` with its optional embedding (``conv3x3_forward_hip`` passes none)."""
    from mzgo._lib import check, lib, ptr, stream_of
    B, Cin, N, _ = x.shape
    Cout = w.shape[0]
    y = torch.empty(B, Cout, N, N, device=x.device)
    check(lib.mzgo_conv3x3_relu_forward(ptr(x), ptr(action), ptr(emb), ptr(w), ptr(bias), B, Cin, Cout, N, ptr(y),
                                        stream_of(x.device)))
    return y


def _equal_bits(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("N,Cin,Cout,B", CASES)
def test_layer_against_float64(N, Cin, Cout, B):
    from mzgo.trainer import conv3x3_backward_hip, conv3x3_forward_hip
    c = {k: v.cuda() for k, v in make_case(N, Cin, Cout, B).items()}
    dead, zero_board, zero_chan = planted(N, Cin, Cout, B)
    out, ref32, ref64 = references(N, Cin, Cout, B, False)
    x, w, bias, g = c["x"], c["w"], c["bias"], c["g"]
    y = conv3x3_forward_hip(x, w, bias)
    check_bar("y", y, ref32["y"], ref64["y"])
    assert (y[:, dead] == 0).all() and (ref64["y"][:, dead] == 0).all()
    assert (y > 0).any()
    if zero_board is not None:                                                # 0 * w sums to 0: relu(bias), exactly
        assert torch.equal(y[zero_board], bias.relu()[:, None, None].expand(Cout, N, N))
    assert torch.equal(conv3x3_forward_hip(x, w, bias), y)                    # deterministic

    out = out.cuda()
    got = conv3x3_backward_hip(g, out, x, w)
    for name, v in zip(("gx", "gw", "gb"), got):
        check_bar(name, v, ref32[name], ref64[name])
    gx, gw, gb = got
    assert _equal_bits(conv3x3_backward_hip(g, out, x, w), got)               # deterministic
    none, gw2, gb2 = conv3x3_backward_hip(g, out, x, w, need_input_grad=False)
    assert none is None and torch.equal(gw2, gw) and torch.equal(gb2, gb)
    # the dead channel: no weight or bias gradient, and whatever gradient arrives at it changes nothing
    assert (gw[dead] == 0).all() and gb[dead].item() == 0
    assert (ref64["gw"][dead] == 0).all() and ref64["gb"][dead].item() == 0
    g2 = g.clone()
    g2[:, dead] = g[:, dead] * 3 + 1
    assert _equal_bits(conv3x3_backward_hip(g2, out, x, w), got)
    if zero_chan is not None:
        assert (gw[:, zero_chan] == 0).all() and (ref64["gw"][:, zero_chan] == 0).all()
        assert gx[:, zero_chan].abs().max().item() > 0
    if zero_board is not None:                            # its products are zeros: gw does not see its gradient; gb does
        g3 = g.clone()
        g3[zero_board] = g[zero_board] * 3 + 1
        _, gw3, gb3 = conv3x3_backward_hip(g3, out, x, w)
        assert torch.equal(gw3, gw)
        assert not torch.equal(gb3, gb) or not (out[zero_board] > 0).any()


def test_weight_gradient_ignores_what_an_earlier_call_left_in_lds():
    """k_conv_bwd_weight stages each gp row in LDS and pads its K (the cells)
    to a multiple of 4 with zeros; the pad meets a 0 from the x side, so only
    a non-finite leftover could show.  An earlier call on 19x19 boards whose
    every gradient is NaN leaves NaN in the rows' first 361 entries on every
    CU; the boards whose cell count is no multiple of 4 (9, 49, 169 cells)
    must give the same bits after it as before it."""
    from mzgo.trainer import conv3x3_backward_hip
    ragged = [c for c in CASES if (c[0] * c[0]) % 4]
    assert {c[0] for c in ragged} == {3, 7, 13}
    runs = []
    for N, Cin, Cout, B in ragged:
        c = {k: v.cuda() for k, v in make_case(N, Cin, Cout, B).items()}
        out = references(N, Cin, Cout, B, False)[0].cuda()
        runs.append((c["g"], out, c["x"], c["w"]))
    before = [conv3x3_backward_hip(*r) for r in runs]
    # 16 (co, ci) tiles x 64 chunks = 1024 workgroups of 52 KB of LDS: every CU, several times over
    Bp, Cp, Np = 512, 64, 19
    nan = torch.full((Bp, Cp, Np, Np), float("nan"), device="cuda")
    zeros = torch.zeros(Bp, Cp, Np, Np, device="cuda")
    _, gw, gb = conv3x3_backward_hip(nan, torch.ones_like(zeros), zeros, torch.zeros(Cp, Cp, 3, 3, device="cuda"),
                                     need_input_grad=False)
    assert gw.isnan().all() and gb.isnan().all()
    for r, want in zip(runs, before):
        got = conv3x3_backward_hip(*r)
        assert all(torch.isfinite(t).all() for t in got)
        assert _equal_bits(got, want)


@pytest.mark.parametrize("N,Cin,Cout,B", CASES)
def test_dynamics_form_against_float64(N, Cin, Cout, B):
    """x + emb[action] broadcast over the board as the layer's input: the
    embedding form of the forward and of the backward
    (``dyn_conv_backward_hip`` where Cin == Cout is a multiple of 16, the
    general entry point's otherwise and as well)."""
    from mzgo.trainer import conv3x3_backward_hip, conv3x3_forward_hip, dyn_conv_backward_hip
    c = {k: v.cuda() for k, v in make_case(N, Cin, Cout, B).items()}
    dead = planted(N, Cin, Cout, B)[0]
    out, ref32, ref64 = references(N, Cin, Cout, B, True)
    x, w, bias, g, emb, action = c["x"], c["w"], c["bias"], c["g"], c["emb"], c["action"]
    y = _forward_hip(x, w, bias, action, emb)
    check_bar("y", y, ref32["y"], ref64["y"])
    assert (y[:, dead] == 0).all() and (ref64["y"][:, dead] == 0).all()
    assert torch.equal(_forward_hip(x, w, bias, action, emb), y)              # deterministic
    # the kernel adds the row in float32 as it loads: the plain form on the sum formed here is the same arithmetic,
    # so a wrong row (the pass, the last row of the larger table) cannot hide in a tolerance
    xe = x + emb[action][:, :, None, None]
    assert torch.equal(y, conv3x3_forward_hip(xe, w, bias))

    out = out.cuda()
    got = conv3x3_backward_hip(g, out, x, w, action, emb)
    for name, v in zip(("gx", "gw", "gb"), got):
        check_bar(name, v, ref32[name], ref64[name])
    assert _equal_bits(conv3x3_backward_hip(g, out, x, w, action, emb), got)  # deterministic
    assert _equal_bits(conv3x3_backward_hip(g, out, xe, w), got)              # the same sum, formed here
    gx, gw, gb = got
    assert (gw[dead] == 0).all() and gb[dead].item() == 0
    g2 = g.clone()
    g2[:, dead] = g[:, dead] * 3 + 1
    assert _equal_bits(conv3x3_backward_hip(g2, out, x, w, action, emb), got)
    if Cin == Cout and Cin % 16 == 0:
        dyn = dyn_conv_backward_hip(g, out, x, action, emb, w)
        for name, v in zip(("gx", "gw", "gb"), dyn):
            check_bar("dyn " + name, v, ref32[name], ref64[name])
        assert _equal_bits(dyn, got)                                          # one set of kernels
        assert _equal_bits(dyn_conv_backward_hip(g, out, x, action, emb, w), dyn)
