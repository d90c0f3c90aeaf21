"""Where the batched trainer step spends what is not the network: the loss
arithmetic of the K + 1 unroll steps on torch ops against the fused kernel
(``mzgo.unroll_loss``, ``TrainConfig.fused_loss``), and Adam + the gradient
clip on their own -- the split DESIGN §4 ("The device replay store") left open.
main.py's configuration, scripts/replay_timing.py's protocol: 6x6 board,
latent_dim 128, batch 128 x unroll 10; the same games, starts and initial
weights for every leg; the legs of a pair alternate in one process; best of
REPS and the median, every value kept.

* step_torch_ms / step_fused_ms -- the whole step (``train`` on a
  ``DeviceReplay``), wall time over STEPS steps;
* loss_torch_* / loss_fused_* -- the loss part alone, forward + backward, from
  fixed detached head outputs made leaves: ``_unroll_step``'s expressions
  (with its device totals), and ``torch.stack`` x 3 + ``unroll_loss``; by
  perf_counter around synchronised calls (_wall_ms) and by HIP events on the
  stream (_events_ms);
* adam_clip_* -- ``clip_grad_norm_`` + ``optimizer.step`` alone on the
  gradients of one step.

Usage (GPU box): python scripts/loss_timing.py [out.json] -> one JSON line
(also written to out.json when given).
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "muzero-go_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def torch_loss(tr, heads, t_val, t_rew, t_pol):
    """``MuZeroTrainer._unroll_step``'s loss lines (device totals included) on
    given head outputs; returns the loss and the stacked totals."""
    c = tr.config
    lgs, vals, rews = heads
    tot = lambda x: x.detach().sum().double()
    kl = lambda lg, tp: F.kl_div(F.log_softmax(lg, dim=1), tp, reduction="none").sum(dim=1)
    v_l = c.value_loss_weight * tr._value_loss(vals[0].squeeze(1), t_val[:, 0])
    p_l = c.policy_loss_weight * kl(lgs[0], t_pol[:, 0])
    per = v_l + p_l
    tot_v, tot_p, tot_r = tot(v_l), tot(p_l), 0.0
    for k in range(1, len(lgs)):
        r_l = c.reward_loss_weight * F.mse_loss(rews[k - 1].squeeze(1), t_rew[:, k - 1], reduction="none")
        v_l = c.value_loss_weight * tr._value_loss(vals[k].squeeze(1), t_val[:, k])
        p_l = c.policy_loss_weight * kl(lgs[k], t_pol[:, k])
        per = per + r_l + v_l + p_l
        tot_r += tot(r_l)
        tot_v += tot(v_l)
        tot_p += tot(p_l)
    loss = per.sum()
    return loss, torch.stack([loss.detach().double(), tot_v, tot_p, tot_r])


def fused_loss(tr, heads, t_val, t_rew, t_pol):
    import mzgo
    c = tr.config
    lgs, vals, rews = heads
    per, totals = mzgo.unroll_loss(torch.stack(lgs), torch.stack([v.squeeze(1) for v in vals]),
                                   torch.stack([r.squeeze(1) for r in rews]), t_pol, t_val, t_rew,
                                   value_loss_weight=c.value_loss_weight, policy_loss_weight=c.policy_loss_weight,
                                   reward_loss_weight=c.reward_loss_weight, value_transform=c.use_value_transform)
    return per.sum(), totals


def timed(fn, steps):
    """(wall ms, HIP-event ms) per call of ``fn`` over ``steps`` calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, e0.elapsed_time(e1) / steps


def main():
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig, initial_inference_torch, recurrent_inference_torch
    from oracle.make_golden import synthetic_trajectories
    N, C, B, K = 6, 128, 128, 10
    A = N * N + 1
    steps, reps = int(os.environ.get("STEPS", 30)), int(os.environ.get("REPS", 5))
    trajs = synthetic_trajectories(N, B, seed=11)
    replay = mzgo.DeviceReplay(N, B, int(1.5 * N * N), "cuda")
    for t in trajs:
        replay.add(t)
    replay.sample_indices = lambda n: np.arange(n)            # the first n games, every step
    start = lambda T: T // 3
    trainers = {}
    for name in ("torch", "fused"):
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 7))
        trainers[name] = MuZeroTrainer(net, TrainConfig(fused_loss=name == "fused"), mode="batched",
                                       start_index=start)
    losses = {}
    for name, tr in trainers.items():                         # warmup (MIOpen picks its kernels here)
        losses[name] = [tr.train(replay, B) for _ in range(2)]
    torch.cuda.synchronize()
    step = {"torch": [], "fused": []}
    for _ in range(reps):
        for name, tr in trainers.items():
            step[name].append(timed(lambda: tr.train(replay, B), steps)[0])

    # the loss part alone: one forward's head outputs, detached and made leaves
    tr = trainers["torch"]
    idx = list(range(B))
    obs0, acts, t_val, t_rew, t_pol = tr.device_targets(replay, idx, [start(len(t["actions"])) for t in trajs])
    with torch.no_grad():
        latent, value, logits = initial_inference_torch(tr.net, obs0)
        lgs, vals, rews = [logits], [value], []
        for k in range(K):
            latent, reward, value, logits = recurrent_inference_torch(tr.net, latent, acts[:, k])
            lgs.append(logits)
            vals.append(value)
            rews.append(reward)
    heads = tuple([t.detach().clone().requires_grad_() for t in ts] for ts in (lgs, vals, rews))
    leaves = [t for ts in heads for t in ts]

    def loss_leg(fn):
        for t in leaves:
            t.grad = None
        loss, totals = fn(tr, heads, t_val, t_rew, t_pol)
        loss.backward()
        return totals

    agree = {name: loss_leg(fn).tolist() for name, fn in (("torch", torch_loss), ("fused", fused_loss))}
    part = {"torch": [], "fused": []}
    for _ in range(2):
        loss_leg(torch_loss), loss_leg(fused_loss)
    for _ in range(reps):
        for name, fn in (("torch", torch_loss), ("fused", fused_loss)):
            part[name].append(timed(lambda: loss_leg(fn), steps))

    # Adam + the clip alone, on the gradients the last step left
    params = list(tr.net.parameters())
    max_norm = tr.config.max_grad_norm

    def adam_clip():
        torch.nn.utils.clip_grad_norm_(params, max_norm=max_norm)
        tr.optimizer.step()

    adam_clip()
    adam = [timed(adam_clip, steps) for _ in range(reps)]

    best = lambda xs: min(xs)
    med = lambda xs: statistics.median(xs)
    out = {"what": "the batched trainer step from a DeviceReplay with the torch loss vs TrainConfig.fused_loss; the "
                   "loss part alone (forward + backward from detached head outputs) on torch ops vs "
                   "mzgo.unroll_loss; Adam + clip_grad_norm_ alone; ms per step, best of REPS runs of STEPS steps "
                   "and the median, all runs kept",
           "config": {"board_size": N, "latent_dim": C, "batch": B, "unroll": K, "steps": steps, "reps": reps},
           "step_torch_ms": best(step["torch"]), "step_fused_ms": best(step["fused"]),
           "step_torch_median_ms": med(step["torch"]), "step_fused_median_ms": med(step["fused"]),
           "step_torch_all_ms": step["torch"], "step_fused_all_ms": step["fused"],
           "warmup_losses": losses, "loss_totals_torch": agree["torch"], "loss_totals_fused": agree["fused"]}
    for name in ("torch", "fused"):
        wall, ev = [w for w, _ in part[name]], [e for _, e in part[name]]
        out.update({f"loss_{name}_wall_ms": best(wall), f"loss_{name}_events_ms": best(ev),
                    f"loss_{name}_wall_median_ms": med(wall), f"loss_{name}_events_median_ms": med(ev),
                    f"loss_{name}_wall_all_ms": wall, f"loss_{name}_events_all_ms": ev})
    wall, ev = [w for w, _ in adam], [e for _, e in adam]
    out.update({"adam_clip_wall_ms": best(wall), "adam_clip_events_ms": best(ev),
                "adam_clip_wall_median_ms": med(wall), "adam_clip_events_median_ms": med(ev),
                "adam_clip_wall_all_ms": wall, "adam_clip_events_all_ms": ev})
    out["step_speedup_fused_over_torch"] = out["step_torch_ms"] / out["step_fused_ms"]
    out["loss_speedup_fused_over_torch_wall"] = out["loss_torch_wall_ms"] / out["loss_fused_wall_ms"]
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
