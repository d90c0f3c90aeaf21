"""The bf16 conv layer kernels (csrc/mzgo_conv_bf16.hip: k_conv_bf16 forward
and input gradient, k_conv_bf16_wgrad, k_conv_bf16_pack) through
``mzgo_conv3x3_relu_forward_bf16`` / ``mzgo_conv3x3_backward_bf16`` against
float64 (tests/f64_reference.py) ON THE ROUNDED OPERANDS.

With R = ``t.bfloat16().float()``, the references get x' = R(x + emb[a]) (the
add in float32) as ``x`` with no embedding, w' = R(w) and, for the backward,
g' = R(g * [out > 0]): exactly what the kernels multiply.  Products of bf16
values are exact in float32, so only the float32 accumulation order is left and
the project's bar applies unchanged (``check_bar``): |got - f64| <= 4 |torch
float32 - f64| + 1e-6 max(1, |f64|.max()).  The bias gradient is checked on the
unrounded g * [out > 0].

``out`` is an input of the backward (the saved output): positive everywhere
but in one planted channel of zeros, whose mask both sides apply.

Shapes: the smallest at which these kernels can go wrong.  A forward / input
gradient workgroup owns G = max(1, 12 // ceil(N*N / 16)) boards (12 at N = 2
and 3, 4 at N = 6, 1 at N = 19) x 32 output channels and walks 32-channel K
slices; the weight pass takes chunks of 8 boards, staged min(384 // cells,
448 // (N + 2)^2) boards at a time (7 at N = 6) with K padded to 32.
"""
import ctypes
import functools

import pytest
import torch

from f64_reference import check_bar, layer_backward_reference, layer_reference

pytestmark = pytest.mark.gpu

# (N, Cin, Cout, B, with_emb)
CASES = [(2, 32, 32, 1, True),        # 4 cells: less than one tile; one K slice; B = 1
         (2, 32, 64, 11, False),      # B = G - 1; the transposition pair
         (2, 64, 32, 12, True),       # B = G
         (3, 32, 32, 13, True),       # 9 cells: a board's K under 32 (the zero pad); B = G + 1
         (3, 96, 96, 25, False),      # B = 2 G + 1; three K slices
         (6, 32, 64, 3, True),        # B = G - 1
         (6, 64, 32, 4, False),       # B = G
         (6, 96, 96, 5, True),        # B = G + 1
         (6, 160, 160, 9, True),      # B = 2 G + 1; five slices, five output tiles
         (6, 32, 32, 17, True),       # the weight pass's chunks 8 + 8 + 1, each staged 7 + 1 boards
         (19, 32, 32, 1, True),       # 361 cells: the LDS maximum, 22 tiles and 9 cells; G = 1
         (19, 32, 64, 2, True),       # B = G + 1
         (19, 64, 32, 3, False)]      # B = 2 G + 1
EXTRA_ROWS = 3
GUARD = 1024                          # floats of NaN either side of every output


def group(N):
    return max(1, 12 // ((N * N + 15) // 16))


def R(t):
    return t.bfloat16().float()


@functools.lru_cache(maxsize=None)
def make_case(N, Cin, Cout, B, with_emb):
    gen = torch.Generator().manual_seed(N * 1000 + Cin * 7 + Cout + B)
    rows = N * N + 1 + EXTRA_ROWS
    x = torch.randn(B, Cin, N, N, generator=gen).relu()
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) / (3 * Cin ** 0.5)
    bias = torch.randn(Cout, generator=gen) * 0.1
    emb = torch.randn(rows, Cin, generator=gen)
    g = torch.randn(B, Cout, N, N, generator=gen)
    action = torch.randint(0, N * N, (B,), generator=gen)
    action[0] = N * N                                      # the pass
    action[B - 1] = rows - 1                               # the table's last row
    out = torch.rand(B, Cout, N, N, generator=gen) + 0.1   # the backward's saved output
    out[:, Cout // 2] = 0.0                                # a dead channel
    if not with_emb:
        emb = action = None
    return dict(x=x, w=w, bias=bias, emb=emb, action=action, g=g, out=out)


@functools.lru_cache(maxsize=None)
def references(N, Cin, Cout, B, with_emb):
    """(float32, float64) results on the rounded operands, once per case."""
    c = make_case(N, Cin, Cout, B, with_emb)
    xr = R(c["x"] + c["emb"][c["action"]][:, :, None, None]) if with_emb else R(c["x"])     # the add in float32
    wr = R(c["w"])
    mask = (c["out"] > 0).float()
    gr = R(c["g"] * mask)
    res = []
    for dtype in (torch.float32, torch.float64):
        y = layer_reference(xr.to(dtype), wr.to(dtype), c["bias"].to(dtype))
        gx, gw, _ = layer_backward_reference(gr.to(dtype), c["out"].to(dtype), xr.to(dtype), wr.to(dtype), None, None)
        gb = (c["g"].to(dtype) * mask.to(dtype)).sum((0, 2, 3))
        res.append(dict(y=y, gx=gx, gw=gw, gb=gb))
    return res


def guarded(*shape):
    """A NaN-filled tensor of ``shape`` inside a larger NaN buffer; (view, buffer)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    return buf[GUARD:GUARD + n].view(*shape), buf


def guards_untouched(buf):
    return bool(buf[:GUARD].isnan().all() and buf[-GUARD:].isnan().all())


def forward(c):
    from mzgo._lib import check, lib, ptr, stream_of
    x = c["x"]
    B, Cin, N, _ = x.shape
    Cout = c["w"].shape[0]
    y, buf = guarded(B, Cout, N, N)
    check(lib.mzgo_conv3x3_relu_forward_bf16(ptr(x), ptr(c["action"]), ptr(c["emb"]), ptr(c["w"]), ptr(c["bias"]), B, Cin,
                                             Cout, N, ptr(y), stream_of(x.device)))
    torch.cuda.synchronize()
    assert guards_untouched(buf)
    return y.clone()


def backward(c, need_gx=True):
    from mzgo._lib import check, lib, ptr, stream_of
    x = c["x"]
    B, Cin, N, _ = x.shape
    Cout = c["w"].shape[0]
    ws = ctypes.c_int64()
    check(lib.mzgo_conv3x3_backward_bf16_workspace(B, Cin, Cout, ctypes.byref(ws)))
    wsf = (ws.value + 3) // 4
    work, wbuf = guarded(wsf)
    outs = [guarded(B, Cin, N, N) if need_gx else (None, None), guarded(Cout, Cin, 3, 3), guarded(Cout)]
    check(lib.mzgo_conv3x3_backward_bf16(ptr(c["g"]), ptr(c["out"]), ptr(x), ptr(c["action"]), ptr(c["emb"]), ptr(c["w"]),
                                         B, Cin, Cout, N, ptr(outs[0][0]), ptr(outs[1][0]), ptr(outs[2][0]), ptr(work),
                                         wsf * 4, stream_of(x.device)))
    torch.cuda.synchronize()
    assert guards_untouched(wbuf)
    for v, buf in outs:
        assert buf is None or guards_untouched(buf)
    return [None if v is None else v.clone() for v, _ in outs]


def test_cases_cover_the_edges():
    Ns = {c[0] for c in CASES}
    assert Ns == {2, 3, 6, 19}
    assert {(c[1], c[2]) for c in CASES} >= {(32, 32), (32, 64), (64, 32), (96, 96), (160, 160)}
    assert [group(N) for N in (2, 3, 6, 19)] == [12, 12, 4, 1]
    for G in (12, 4, 1):
        assert {c[3] for c in CASES if group(c[0]) == G} >= {G - 1, G, G + 1, 2 * G + 1} - {0}
    assert {1, 17} <= {c[3] for c in CASES} and {c[4] for c in CASES} == {True, False}


@pytest.mark.parametrize("N,Cin,Cout,B,with_emb", CASES)
def test_layer_against_float64_on_rounded_operands(N, Cin, Cout, B, with_emb):
    case = make_case(N, Cin, Cout, B, with_emb)
    c = {k: None if v is None else v.cuda() for k, v in case.items()}
    ref32, ref64 = references(N, Cin, Cout, B, with_emb)
    y = forward(c)
    check_bar("y", y, ref32["y"], ref64["y"])
    assert (y > 0).any()
    assert torch.equal(forward(c), y)                                         # the same bits again

    gx, gw, gb = backward(c)
    check_bar("gx", gx, ref32["gx"], ref64["gx"])
    check_bar("gw", gw, ref32["gw"], ref64["gw"])
    check_bar("gb", gb, ref32["gb"], ref64["gb"])
    dead = Cout // 2
    assert (gw[dead] == 0).all() and gb[dead].item() == 0                     # the mask, from the saved output
    again = backward(c)
    assert all(torch.equal(p, q) for p, q in zip(again, (gx, gw, gb)))        # the same bits again
    none, gw2, gb2 = backward(c, need_gx=False)                               # gx = NULL is accepted
    assert none is None and torch.equal(gw2, gw) and torch.equal(gb2, gb)
    if with_emb:
        # the kernels add the row in float32 before they round: the plain form on the sum formed here is the
        # same arithmetic, so a wrong row cannot hide in a tolerance
        plain = dict(c, x=c["x"] + c["emb"][c["action"]][:, :, None, None], emb=None, action=None)
        assert torch.equal(forward(plain), y)
        assert all(torch.equal(p, q) for p, q in zip(backward(plain), (gx, gw, gb)))
