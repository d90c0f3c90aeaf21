"""``mzgo.unroll(..., precision="bf16")`` (csrc/mzgo_unroll.hip on the kernels
of csrc/mzgo_conv_bf16.hip): what the mode leaves bit for bit alone, its
determinism, and its whole graph against float64.

The reference is a torch CPU graph in which the dynamics conv is ONE
``autograd.Function`` with the mode's semantics (mzgo.h): with R =
``t.bfloat16().float()`` applied through float32,

    forward    y  = relu(conv3x3(R(x + emb[a]), R(W)) + b), the add in float32
    backward   gx = conv3x3^T(R(gp), R(W)), gw = corr(R(gp), R(x + emb[a])),
               gb = sum gp, gp = g [y > 0]; no gradient of R

and everything else is ``initial_inference_torch`` / ``recurrent_inference_torch``'s
text.  It is evaluated in float64 and in float32.  Latents feed the next
step's rounding, so an element near a rounding boundary may round to the
neighbouring bf16 value in one evaluation and not in another
(tests/test_gpu_tower.py documents the same effect): the bar cannot be derived,
it is measured -- ``check_bar(got, emulation in float32, emulation in float64)``,
the project's 4x bar, whose "own" term already holds the float32 emulation's
own flips.  The inputs must make that bar meaningful:
``test_reference_sits_inside_its_own_bar`` (CPU) evaluates the emulation a
second time in float32 with another summation order (the conv as unfold +
matmul) and asks err / bound <= 0.5 of every output and gradient class.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from f64_reference import check_bar, mixed_loss

gpu = pytest.mark.gpu

# (N, C, B, K, seed): the smallest seed >= 0 that meets test_reference_sits_inside_its_own_bar (seed 0 of the first
# case gives 0.52 there; seed 1 gives 0.25 and 0.24)
F64_CASES = [(6, 64, 9, 4, 1), (9, 32, 5, 3, 1)]
MODE_CASE = F64_CASES[0]
# the weight pass at more than 8 boards per chunk: 369 = 16 * 23 + 1 boards of 2x2 at C = 160 take 16 per chunk
# (the partials' 32 MiB cap, mzgo.h), so the last chunk is one board; seeds 0 and 3 fail the reference's condition
WIDE_CASE = (2, 160, 41, 9, 1)


def R(t):
    return t.float().bfloat16().float()


class _DynConvBf16(torch.autograd.Function):
    """The dynamics conv in bf16 mode, in the dtype of ``latent``; ``matmul``: the three products as unfold + matmul."""

    @staticmethod
    def forward(ctx, latent, row, w, b, matmul):
        D = latent.dtype
        xr = R(latent.float() + row.float()[:, :, None, None]).to(D)       # the add in float32, then R
        wr = R(w).to(D)
        if matmul:
            B, C, N, _ = xr.shape
            cols = F.unfold(xr, 3, padding=1)                              # [B, C 9, cells]
            pre = (wr.view(wr.shape[0], -1) @ cols).view(B, -1, N, N) + b[None, :, None, None]
        else:
            pre = F.conv2d(xr, wr, b, padding=1)
        y = pre.relu()
        ctx.save_for_backward(xr, wr, y)
        ctx.matmul = matmul
        return y

    @staticmethod
    def backward(ctx, g):
        xr, wr, y = ctx.saved_tensors
        D = y.dtype
        gp = g * (y > 0).to(D)
        gpr = R(gp).to(D)
        if ctx.matmul:
            B, C, N, _ = xr.shape
            gf = gpr.view(B, -1, N * N)
            cols = F.unfold(xr, 3, padding=1)
            gw = torch.einsum("bol,bkl->ok", gf, cols).view_as(wr)
            gx = F.fold(wr.view(wr.shape[0], -1).t() @ gf, (N, N), 3, padding=1)
        else:
            gx = torch.nn.grad.conv2d_input(xr.shape, wr, gpr, padding=1)
            gw = torch.nn.grad.conv2d_weight(xr, wr.shape, gpr, padding=1)
        return gx, gx.sum((2, 3)), gw, gp.sum((0, 2, 3)), None


def build_net(N, C, seed):
    import mzgo
    A = N * N + 1
    net = mzgo.MuZeroNet(C, A)
    net.load_state_dict(mzgo.deterministic_state_dict(C, A, seed))
    return net


@functools.lru_cache(maxsize=None)
def make_inputs(N, B, K, seed):
    gen = torch.Generator().manual_seed(1000 * seed + 10 * N + B + K)
    obs = (torch.rand(B, 6, N, N, generator=gen) < 0.3).float()
    if K == 0:
        return obs, None
    acts = torch.randint(0, N * N + 1, (B, K), generator=gen)
    acts[B - 1, K - 1] = N * N                              # the pass
    return obs, acts


def emulate(N, C, B, K, seed, dtype, matmul=False):
    """The bf16 mode's graph in ``dtype`` on the CPU: a dict of float64 numpy arrays (outputs, loss, grads)."""
    import copy

    from mzgo.trainer import _prediction, initial_inference_torch
    net = copy.deepcopy(build_net(N, C, seed)).to(dtype)
    obs, acts = make_inputs(N, B, K, seed)
    latent, value, logits = initial_inference_torch(net, obs.to(dtype))
    lgs, vals, rews = [logits], [value.squeeze(1)], []
    d = net.dynamics
    for k in range(1, K + 1):                               # recurrent_inference_torch, with the conv replaced
        row = d.action_embedding(acts[:, k - 1])
        latent = _DynConvBf16.apply(latent, row, d.conv.weight, d.conv.bias, matmul)
        reward = d.fc_reward_output(F.relu(d.fc_reward_hidden(d.reward_conv(latent).mean(dim=[2, 3]))))
        value, logits = _prediction(net, latent)
        lgs.append(logits)
        vals.append(value.squeeze(1))
        rews.append(reward.squeeze(1))
    out = (torch.stack(lgs), torch.stack(vals), torch.stack(rews) if rews else None)
    loss = mixed_loss(*out)
    loss.backward()
    np64 = lambda a: None if a is None else a.detach().double().numpy()
    return dict(logits=np64(out[0]), value=np64(out[1]), reward=np64(out[2]), loss=np64(loss),
                grads={k: np64(p.grad) for k, p in net.named_parameters()})


@functools.lru_cache(maxsize=None)
def references(N, C, B, K, seed):
    return emulate(N, C, B, K, seed, torch.float32), emulate(N, C, B, K, seed, torch.float64)


def classes(res):
    """name -> array over every output and gradient class of a result."""
    out = {k: res[k] for k in ("logits", "value", "reward", "loss")}
    out.update(res["grads"])
    return out


@pytest.mark.parametrize("N,C,B,K,seed", F64_CASES + [WIDE_CASE])
def test_reference_sits_inside_its_own_bar(N, C, B, K, seed):
    """The condition on the inputs (CPU): another float32 evaluation, with another summation order, is within
    half the bar everywhere.  Otherwise the seed is a bad one: pick another."""
    ref32, ref64 = references(N, C, B, K, seed)
    other = classes(emulate(N, C, B, K, seed, torch.float32, matmul=True))
    c32, c64 = classes(ref32), classes(ref64)
    assert len(c64) == 26
    worst = max(check_bar("reference: " + k, other[k], c32[k], c64[k]) for k in c64)
    assert worst <= 0.5, worst
    # and the rounding is in the graph: its float64 result is not float64 of the plain network
    from f64_reference import unroll_reference
    plain = unroll_reference(build_net(N, C, seed), *make_inputs(N, B, K, seed), torch.float64)
    assert np.abs(plain["logits"][1:] - ref64["logits"][1:]).max() > 1e-4
    assert np.array_equal(plain["logits"][0], ref64["logits"][0])


def run_unroll(N, C, B, K, seed, precision):
    import mzgo
    net = build_net(N, C, seed).cuda()
    obs, acts = make_inputs(N, B, K, seed)
    out = mzgo.unroll(net, obs.cuda(), None if acts is None else acts.cuda(), precision=precision)
    loss = mixed_loss(*out)
    loss.backward()
    grads = {k: None if p.grad is None else p.grad.detach().clone() for k, p in net.named_parameters()}
    return out, loss.detach(), grads


def same_bits(a, b):
    (oa, la, ga), (ob, lb, gb) = a, b
    assert len(ga) == len(gb) == 22
    for p, q in zip(oa, ob):
        assert (p is None and q is None) or torch.equal(p, q)
    assert torch.equal(la, lb)
    for k in ga:
        assert (ga[k] is None and gb[k] is None) or torch.equal(ga[k], gb[k]), k


@gpu
def test_k0_is_the_float32_mode_bit_for_bit():
    same_bits(run_unroll(5, 32, 3, 0, 1, "bf16"), run_unroll(5, 32, 3, 0, 1, "fp32"))


@gpu
def test_step_0_keeps_the_float32_bits_and_repeats_are_identical():
    a = run_unroll(5, 32, 3, 2, 1, "bf16")
    f = run_unroll(5, 32, 3, 2, 1, "fp32")
    assert torch.equal(a[0][0][0], f[0][0][0]) and torch.equal(a[0][1][0], f[0][1][0])     # logits[0], value[0]
    assert not torch.equal(a[0][0][1:], f[0][0][1:])
    same_bits(a, run_unroll(5, 32, 3, 2, 1, "bf16"))
    assert all(g is not None and torch.isfinite(g).all() for g in a[2].values())


@gpu
def test_two_bf16_trainers_stay_bit_equal():
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    from oracle.make_golden import synthetic_trajectories
    N, C, B, K = 5, 32, 4, 2
    A = N * N + 1
    nets, losses = [], []
    for _ in range(2):
        rp = mzgo.DeviceReplay(N, B, int(1.5 * N * N), "cuda")
        for i, t in enumerate(synthetic_trajectories(N, B, seed=9)):
            # search-value targets from planted root values: network targets would need an engine for the
            # bootstrap inference, and the library builds none at 5x5 with C = 32
            T = len(t["actions"])
            rp.add(dict(t, root_values=[((7 * i + 3 * j) % 11 - 5) / 8.0 for j in range(T)]))
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 6))
        cfg = TrainConfig(learning_rate=1e-3, unroll_steps=K, fused_loss=True, fused_unroll=True, device_sampling=True,
                          device_optimizer=True, unroll_precision="bf16", value_target="search")
        tr = MuZeroTrainer(net, cfg, mode="batched", sample_seed=5)
        run = []
        for _ in range(3):
            assert tr.train(rp, B) is not None
            run.append(dict(tr.read_stats())["training_loss"])
        nets.append(net)
        losses.append(run)
    assert all(np.isfinite(v) for v in losses[0]) and losses[0] == losses[1]
    start = mzgo.deterministic_state_dict(C, A, 6)
    for (k, p), q in zip(nets[0].named_parameters(), nets[1].parameters()):
        assert torch.equal(p, q), k
        assert not torch.equal(p.detach().cpu(), start[k]), k                  # and they trained


def test_wide_case_takes_16_boards_per_chunk():
    N, C, B, K, _ = WIDE_CASE
    cb = 8
    while cb < K * B and -(-K * B // cb) * C * C * 36 > (32 << 20):
        cb += 8
    assert cb == 16 and (K * B) % cb == 1


@gpu
@pytest.mark.parametrize("N,C,B,K,seed", F64_CASES + [WIDE_CASE])
def test_bf16_unroll_against_float64(N, C, B, K, seed):
    ref32, ref64 = references(N, C, B, K, seed)
    out, loss, grads = run_unroll(N, C, B, K, seed, "bf16")
    got = dict(zip(("logits", "value", "reward"), out), loss=loss, **grads)
    c32, c64 = classes(ref32), classes(ref64)
    assert set(got) == set(c64) and len(got) == 26
    ratios = {k: check_bar(k, got[k], c32[k], c64[k]) for k in c64}
    print("worst err/bound", max(ratios.values()))


@gpu
def test_the_mode_is_on():
    """The bf16 outputs leave the float32 mode's by more than the float32 mode's own bar, and the distance of
    the loss and the gradients is printed (recorded in DESIGN, not asserted against a number)."""
    from f64_reference import unroll_reference
    N, C, B, K, seed = MODE_CASE
    net = build_net(N, C, seed)
    obs, acts = make_inputs(N, B, K, seed)
    p32, p64 = (unroll_reference(net, obs, acts, dt) for dt in (torch.float32, torch.float64))
    b_out, b_loss, b_grads = run_unroll(N, C, B, K, seed, "bf16")
    f_out, f_loss, f_grads = run_unroll(N, C, B, K, seed, "fp32")
    for name, b, f in zip(("logits", "value", "reward"), b_out, f_out):
        check_bar("fp32 mode " + name, f, p32[name], p64[name])               # the float32 mode is inside its bar
        err = np.abs(b.detach().cpu().double().numpy() - p64[name]).max()
        bound = 4 * np.abs(p32[name] - p64[name]).max() + 1e-6 * max(1.0, np.abs(p64[name]).max())
        print(f"bf16 mode {name}: distance to the plain float64 graph {err:.3g}, the float32 bar {bound:.3g}")
        assert err > bound, name
    rel = lambda b, f: ((b - f).norm() / f.norm()).item()
    print(f"loss: fp32 {f_loss.item():.6f} bf16 {b_loss.item():.6f} relative {abs(b_loss.item() / f_loss.item() - 1):.3g}")
    for k in b_grads:
        print(f"{k}: relative distance {rel(b_grads[k], f_grads[k]):.3g}")
