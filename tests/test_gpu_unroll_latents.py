"""``mzgo.unroll(..., return_latents=True)`` (csrc/mzgo_unroll.hip:
``mzgo_unroll_latents``, ``mzgo_unroll_backward_l``): the latents it hands out
and the gradient it takes on them, against the float64 graph of
``initial_inference_torch`` / ``recurrent_inference_torch`` under
``f64_reference.check_bar``; what the flag leaves bit for bit alone; and the
same in bf16 mode through tests/test_gpu_unroll_bf16.py's emulation with the
loss extended by the latent term.

The latent term is ``(latents * R).sum()`` with a fixed random R, so every
latent element gets its own gradient.  End to end the ReLU masks are not
inputs: each fp32 case's seed is the smallest whose float64 graph keeps every
ReLU input at least 1e-5 from 0 (``unroll_reference``'s ``min_pre``, as
tests/test_gpu_unroll_edges.py), and the bf16 case's seed the smallest for
which a second float32 evaluation of the emulation in another summation order
sits inside half its own bar (both asserted on the CPU below).
"""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from f64_reference import RELU_INPUTS, check_bar, mixed_loss
from test_gpu_unroll_bf16 import _DynConvBf16

gpu = pytest.mark.gpu

MIN_PRE = 1e-5
# (N, C, B, K, seed)
CASES = [(5, 16, 1, 0, 0), (5, 16, 3, 2, 0), (9, 48, 2, 1, 41)]
BF16_CASE = (5, 32, 2, 2, 0)
MODES = ("heads+latents", "latents")


def build_net(N, C, seed):
    import mzgo
    A = N * N + 1
    net = mzgo.MuZeroNet(C, A)
    net.load_state_dict(mzgo.deterministic_state_dict(C, A, seed))
    return net


@functools.lru_cache(maxsize=None)
def make_inputs(N, C, B, K, seed):
    """Observations, actions (None at K = 0) and the latent term's R, CPU tensors."""
    gen = torch.Generator().manual_seed(1000 * seed + 10 * N + B + K)
    obs = (torch.rand(B, 6, N, N, generator=gen) < 0.3).float()
    acts = None
    if K > 0:
        acts = torch.randint(0, N * N + 1, (B, K), generator=gen)
        acts[B - 1, K - 1] = N * N                          # the pass
    R = torch.randn(K + 1, B, C, N, N, generator=gen)
    return obs, acts, R


def full_loss(mode, heads, latents, R):
    term = (latents * R.to(latents.dtype).to(latents.device)).sum()
    return term if mode == "latents" else mixed_loss(*heads) + term


def reference(N, C, B, K, seed, dtype, mode, bf16=False, matmul=False):
    """The unroll's graph in ``dtype`` on the CPU, returning its latents too: a dict of float64 numpy arrays
    (``latents`` [K+1, B, C, N, N], ``loss``, ``grads``) and ``min_pre``.  ``bf16``: the dynamics conv is
    tests/test_gpu_unroll_bf16.py's Function (``matmul``: its other summation order)."""
    from mzgo.trainer import _prediction, initial_inference_torch, recurrent_inference_torch
    net = copy.deepcopy(build_net(N, C, seed)).to(dtype)
    obs, acts, R = make_inputs(N, C, B, K, seed)
    pre = []
    modules = dict(net.named_modules())
    hooks = [modules[name].register_forward_hook(lambda m, i, o: pre.append(o.detach().abs().min().item()))
             for name in RELU_INPUTS]
    latent, value, logits = initial_inference_torch(net, obs.to(dtype))
    lats, lgs, vals, rews = [latent], [logits], [value.squeeze(1)], []
    d = net.dynamics
    for k in range(1, K + 1):
        if bf16:
            latent = _DynConvBf16.apply(latent, d.action_embedding(acts[:, k - 1]), d.conv.weight, d.conv.bias, matmul)
            reward = d.fc_reward_output(F.relu(d.fc_reward_hidden(d.reward_conv(latent).mean(dim=[2, 3]))))
            value, logits = _prediction(net, latent)
        else:
            latent, reward, value, logits = recurrent_inference_torch(net, latent, acts[:, k - 1])
        lats.append(latent)
        lgs.append(logits)
        vals.append(value.squeeze(1))
        rews.append(reward.squeeze(1))
    for h in hooks:
        h.remove()
    latents = torch.stack(lats)
    loss = full_loss(mode, (torch.stack(lgs), torch.stack(vals), torch.stack(rews) if rews else None), latents, R)
    loss.backward()
    np64 = lambda a: None if a is None else a.detach().double().numpy()
    return dict(latents=np64(latents), loss=np64(loss), grads={k: np64(p.grad) for k, p in net.named_parameters()},
                min_pre=min(pre))


@functools.lru_cache(maxsize=None)
def references(N, C, B, K, seed, mode, bf16=False):
    return tuple(reference(N, C, B, K, seed, dt, mode, bf16) for dt in (torch.float32, torch.float64))


def classes(res):
    out = {"latents": res["latents"], "loss": res["loss"]}
    out.update({k: g for k, g in res["grads"].items() if g is not None})
    return out


@pytest.mark.parametrize("N,C,B,K,seed", CASES)
def test_seeds_keep_the_relu_inputs_away_from_zero(N, C, B, K, seed):
    """The condition on the fp32 cases' inputs (CPU), and that ``seed`` is the smallest that meets it."""
    assert references(N, C, B, K, seed, MODES[0])[1]["min_pre"] >= MIN_PRE
    for s in range(seed):
        assert reference(N, C, B, K, s, torch.float64, MODES[0])["min_pre"] < MIN_PRE, s


def test_bf16_reference_sits_inside_its_own_bar():
    """The condition on the bf16 case's inputs (CPU), as tests/test_gpu_unroll_bf16.py requires of its seeds."""
    N, C, B, K, seed = BF16_CASE
    ref32, ref64 = references(N, C, B, K, seed, MODES[0], True)
    other = classes(reference(N, C, B, K, seed, torch.float32, MODES[0], True, matmul=True))
    c32, c64 = classes(ref32), classes(ref64)
    assert len(c64) == 24
    worst = max(check_bar("reference: " + k, other[k], c32[k], c64[k]) for k in c64)
    assert worst <= 0.5, worst


def run_unroll(N, C, B, K, seed, mode, precision="fp32", return_latents=True, g_latent="R"):
    """``mzgo.unroll`` and a backward on the GPU -> (latents or None, loss, grads).  ``mode`` None: ``mixed_loss``
    of the heads alone (no gradient reaches the latents); ``g_latent="zero"``: the latent term with R = 0."""
    import mzgo
    net = build_net(N, C, seed).cuda()
    obs, acts, R = make_inputs(N, C, B, K, seed)
    out = mzgo.unroll(net, obs.cuda(), None if acts is None else acts.cuda(), precision=precision,
                      return_latents=return_latents)
    assert len(out) == (4 if return_latents else 3)
    latents = out[3] if return_latents else None
    if mode is None:
        loss = mixed_loss(*out[:3])
    else:
        loss = full_loss(mode, out[:3], latents, R if g_latent == "R" else torch.zeros_like(R))
    loss.backward()
    grads = {k: None if p.grad is None else p.grad.detach().clone() for k, p in net.named_parameters()}
    return latents, loss.detach(), grads


def check_against(ref32, ref64, latents, loss, grads, K):
    check_bar("latents", latents, ref32["latents"], ref64["latents"])
    check_bar("loss", loss, ref32["loss"], ref64["loss"])
    assert len(grads) == 22
    for k, want in ref64["grads"].items():
        if want is None:                                    # K = 0: the dynamics take no part, as autograd
            assert K == 0 and k.startswith("dynamics.") and grads[k] is None, k
            continue
        assert grads[k] is not None, k
        check_bar(k, grads[k], ref32["grads"][k], want)


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,C,B,K,seed", CASES)
def test_latents_and_their_gradient_against_float64(N, C, B, K, seed, mode):
    ref32, ref64 = references(N, C, B, K, seed, mode)
    latents, loss, grads = run_unroll(N, C, B, K, seed, mode)
    assert latents.shape == (K + 1, B, C, N, N) and latents.dtype == torch.float32 and latents.requires_grad
    if mode == "latents" and K > 0:                         # the heads got no gradient: autograd gives them none
        for k in ("prediction.value_fc.weight", "prediction.pass_logit", "dynamics.fc_reward_output.bias"):
            assert ref64["grads"][k] is None and (grads[k] == 0).all(), k
        ref32 = dict(ref32, grads={k: g for k, g in ref32["grads"].items() if ref64["grads"][k] is not None})
        ref64 = dict(ref64, grads={k: g for k, g in ref64["grads"].items() if g is not None})
        assert len(ref64["grads"]) == 9                     # the representation's six and the dynamics conv's three
    elif mode == "latents":
        ref64 = dict(ref64, grads={k: g for k, g in ref64["grads"].items() if g is not None})
        assert len(ref64["grads"]) == 6
    check_against(ref32, ref64, latents, loss, grads, K if mode == MODES[0] else -1)


def same_grads(a, b, bits=True):
    assert len(a) == len(b) == 22
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        elif bits:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
        else:
            assert torch.equal(a[k], b[k]), k


@gpu
@pytest.mark.parametrize("N,C,B,K,seed,precision", [c + ("fp32",) for c in CASES[1:]] + [BF16_CASE + ("bf16",)])
def test_the_flag_leaves_the_backward_alone(N, C, B, K, seed, precision):
    """Without the flag, and with it when no gradient reaches the latents, the 22 gradients are the bits of the
    call without the flag (``mzgo_unroll_backward_p``, which the parent ran); an all-zero latent gradient gives
    equal values (x + 0 = x, up to the sign of a zero)."""
    _, loss0, plain = run_unroll(N, C, B, K, seed, None, precision, return_latents=False)
    latents, loss1, unused = run_unroll(N, C, B, K, seed, None, precision)
    assert torch.equal(loss0, loss1)
    same_grads(plain, unused)
    _, _, again = run_unroll(N, C, B, K, seed, None, precision, return_latents=False)
    same_grads(plain, again)
    _, _, zero = run_unroll(N, C, B, K, seed, MODES[0], precision, g_latent="zero")
    same_grads(plain, zero, bits=False)
    assert np.count_nonzero(latents.detach().cpu().numpy()) > 0


@gpu
def test_latents_are_a_view_that_must_not_be_written():
    import mzgo
    N, C, B, K, seed = CASES[1]
    net = build_net(N, C, seed).cuda()
    obs, acts, R = make_inputs(N, C, B, K, seed)
    logits, value, reward, latents = mzgo.unroll(net, obs.cuda(), acts.cuda(), return_latents=True)
    with pytest.raises(RuntimeError):
        latents.mul_(2.0)
        (latents * R.cuda()).sum().backward()


@gpu
def test_bf16_latents_and_their_gradient_against_float64():
    N, C, B, K, seed = BF16_CASE
    ref32, ref64 = references(N, C, B, K, seed, MODES[0], True)
    latents, loss, grads = run_unroll(N, C, B, K, seed, MODES[0], "bf16")
    got = dict(latents=latents, loss=loss, **grads)
    c32, c64 = classes(ref32), classes(ref64)
    assert set(got) == set(c64) and len(got) == 24
    ratios = {k: check_bar(k, got[k], c32[k], c64[k]) for k in c64}
    print("worst err/bound", max(ratios.values()))
