"""Float64 references of the trainer's HIP kernels (csrc/mzgo_train.hip,
csrc/mzgo_unroll.hip), written with torch on the CPU, and the bar the tests
hold the kernels to.  A plain module: tests/test_gpu_conv_f64.py,
tests/test_gpu_unroll_edges.py and tests/test_unroll_edge_cases.py import it.

Every function takes CPU tensors and computes in the dtype it is given (the
layer functions: the dtype of their arguments), so the same text gives the
float64 truth and torch-float32's own result on the same float32 inputs.
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

# the modules whose output feeds a ReLU in initial_inference_torch / recurrent_inference_torch
RELU_INPUTS = ("representation.conv1", "representation.conv2", "representation.conv3", "dynamics.conv",
               "dynamics.fc_reward_hidden")


def _with_embedding(x, action, emb):
    if emb is None:
        return x
    return x + emb[action][:, :, None, None]


def layer_reference(x, w, b, action=None, emb=None):
    """relu(conv2d(x (+ emb[action] broadcast over the board), w, b, padding=1))."""
    return F.relu(F.conv2d(_with_embedding(x, action, emb), w, b, padding=1))


def layer_backward_reference(g, out, x, w, action, emb):
    """The layer's backward from the saved output ``out`` AS GIVEN: gp = g *
    (out > 0) -- the kernels' mask, an input here, so no precision can flip
    it.  Returns (conv2d_input, conv2d_weight, gp.sum((0, 2, 3)))."""
    gp = g * (out > 0).to(g.dtype)
    xin = _with_embedding(x, action, emb)
    gx = torch.nn.grad.conv2d_input(xin.shape, w, gp, padding=1)
    gw = torch.nn.grad.conv2d_weight(xin, w.shape, gp, padding=1)
    return gx, gw, gp.sum((0, 2, 3))


def mixed_loss(logits, value, reward):
    """tests/test_gpu_unroll.py's ``_mixed_loss`` (restated: importing that
    module from here would make a cycle of test modules)."""
    loss = (value[0] ** 2).sum() + logits[0].logsumexp(1).sum()
    for k in range(1, logits.shape[0]):
        loss = loss + (reward[k - 1] ** 2).sum() + (value[k] * 0.5).sum() + logits[k].logsumexp(1).sum()
    return loss


def loss_without_reward(logits, value, reward):
    """``mixed_loss`` without its reward term: the reward head gets no gradient."""
    loss = (value[0] ** 2).sum() + logits[0].logsumexp(1).sum()
    for k in range(1, logits.shape[0]):
        loss = loss + (value[k] * 0.5).sum() + logits[k].logsumexp(1).sum()
    return loss


def unroll_reference(net, obs, acts, dtype, loss_fn=mixed_loss):
    """The graph of ``initial_inference_torch`` / ``recurrent_inference_torch``
    on a copy of ``net`` in ``dtype`` on the CPU, from ``obs`` [B, 6, N, N] and
    ``acts`` i64 [B, K] (None or [B, 0]: K = 0).  Returns a dict of float64
    numpy arrays: ``logits`` [K+1, B, A], ``value`` [K+1, B], ``reward``
    [K, B] (None at K = 0), ``loss``, ``grads`` (all 22 parameters by name; None
    where autograd gives none) and ``min_pre``, the smallest |pre-activation|
    over every ReLU input of the graph (forward hooks on RELU_INPUTS)."""
    from mzgo.trainer import initial_inference_torch, recurrent_inference_torch
    net = copy.deepcopy(net).cpu().to(dtype)
    net.zero_grad()
    pre = []
    modules = dict(net.named_modules())
    hooks = [modules[name].register_forward_hook(lambda m, i, o: pre.append(o.detach().abs().min().item()))
             for name in RELU_INPUTS]
    obs = obs.detach().cpu().to(dtype)
    K = 0 if acts is None else acts.shape[1]
    latent, value, logits = initial_inference_torch(net, obs)
    lgs, vals, rews = [logits], [value.squeeze(1)], []
    for k in range(1, K + 1):
        latent, reward, value, logits = recurrent_inference_torch(net, latent, acts[:, k - 1].cpu())
        lgs.append(logits)
        vals.append(value.squeeze(1))
        rews.append(reward.squeeze(1))
    for h in hooks:
        h.remove()
    assert len(pre) == 3 + 2 * K
    out = (torch.stack(lgs), torch.stack(vals), torch.stack(rews) if rews else None)
    loss = loss_fn(*out)
    loss.backward()
    np64 = lambda a: None if a is None else a.detach().double().numpy()
    return dict(logits=np64(out[0]), value=np64(out[1]), reward=np64(out[2]), loss=np64(loss),
                grads={k: np64(p.grad) for k, p in net.named_parameters()}, min_pre=min(pre))


def check_bar(name, got, ref32, ref64):
    """tests/test_unroll.py's bar: |got - f64| <= 4 |torch_f32 - f64| + 1e-6
    max(1, |f64|.max()), with ``ref32`` torch float32's result from the same
    inputs.  Prints err, own and bound; returns err / bound."""
    as64 = lambda a: (a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor)
                      else np.asarray(a, dtype=np.float64))
    got, ref32, ref64 = as64(got), as64(ref32), as64(ref64)
    assert got.shape == ref64.shape == ref32.shape, (name, got.shape, ref32.shape, ref64.shape)
    assert np.isfinite(got).all(), name
    err, own = np.abs(got - ref64).max(), np.abs(ref32 - ref64).max()
    bound = 4 * own + 1e-6 * max(1.0, np.abs(ref64).max())
    print(f"{name}: max |ref| {np.abs(ref64).max():.4g}  err {err:.3g}  own {own:.3g}  bound {bound:.3g}  "
          f"err/bound {err / bound:.3f}")
    assert err <= bound, f"{name}: err {err:.3g} > bound {bound:.3g} (own {own:.3g})"
    return err / bound
