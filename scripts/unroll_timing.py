"""The batched trainer step with ``TrainConfig.fused_unroll`` off and on
(``mzgo.unroll``: the whole K-step unroll as one autograd node, one HIP
forward call and one backward call), at main.py's sizes: 6x6, C = 128, batch
128 x unroll 10.  The baseline is the per-step torch graph (the parent path)
run in this same process; the legs alternate.

EXPECTATION, written before the first run (DESIGN §4 "The whole unroll as one
node"): the torch path enqueues about 640 launches for the network part of a
step (per unroll step some 17 forward -- embedding lookup, add, conv + bias,
relu, three 1x1 convs, two means, three linears, relu, cat -- and some 45
backward, the parameter gradients' accumulation included; the representation
and step 0's heads about 25), the fused path 42 (K + 5 forward, K + 17
backward) from two calls.  At the 5.3 us per eager launch of
profiles/loss_timing.json that is 3.4 ms against 0.2 ms of enqueueing.  If the
9.7 ms network part is host-bound as DESIGN §4 says, the saving is at most the
whole gap between the host's 9.7 ms and the GPU time of the fused path's own
kernels, and at least those 3.2 ms of launches; so: network part 9.7 -> about
6.5 ms or less, whole step 11.4 -> about 8 ms.  What could undo it: the 3x3
convs run on the one-wave-per-tile fp32 MFMA kernels of mzgo_train.hip, which
measured 8 % slower than MIOpen's inside ``hip_forward``; with the launches
gone, their GPU time (net_gpu_ms below, never measured alone before) is the
new floor.

Figures, each best / median / spread (max - min) over REPS alternating
windows after a warm-up of both legs:

* step_off_ms / step_on_ms       the whole ``train`` step from a ``DeviceReplay``
                                 with device_sampling + deferred_stats +
                                 fused_loss + device_weights, wall time over
                                 STEPS steps ending in a synchronise;
* net_wall_off_ms / net_wall_on_ms    forward + backward of the network part
                                 alone from fixed targets (the head outputs,
                                 ``unroll_loss``, ``backward``), wall time over
                                 STEPS passes ending in a synchronise;
* net_event_off_ms / net_event_on_ms  the same window by HIP events;
* net_gpu_off_ms / net_gpu_on_ms      the same window enqueued behind a long
                                 matmul, so that the events see the kernels
                                 back to back without the host (for the torch
                                 leg only as far as its enqueueing outlasts the
                                 matmul);
* backward_event_off_ms / backward_event_on_ms  events around ``backward()``
                                 alone: with fused_unroll the one
                                 ``mzgo_unroll_backward`` call (and
                                 ``unroll_loss``'s three multiplies).

Before timing, the two legs' losses and gradients at the same weights are
compared (fp32 tolerance).

Usage (GPU box): python scripts/unroll_timing.py [out.json] -> one JSON line
(also written to out.json when given).
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "muzero-go_amd")]

import torch  # noqa: E402

EXPECTATION = {
    "torch_path_launches_network_part": 640,
    "fused_path_launches": {"forward": "K + 5 = 15", "backward": "K + 17 = 27"},
    "eager_launch_us": 5.3,
    "launch_time_saved_ms": 3.2,
    "network_part_ms": "9.7 -> about 6.5 or less",
    "whole_step_ms": "11.4 -> about 8",
    "risk": "the fp32 MFMA conv kernels' own GPU time (8 % slower than MIOpen inside hip_forward) is the new floor",
}


def _summary(xs):
    return {"best": min(xs), "median": statistics.median(xs), "spread": max(xs) - min(xs), "all": xs}


def main():
    import mzgo
    from mzgo.loss import unroll_loss
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    from oracle.make_golden import synthetic_trajectories
    steps, reps = (int(os.environ.get(k, d)) for k, d in (("STEPS", 10), ("REPS", 7)))
    N, C, B, K = 6, 128, 128, 10
    A = N * N + 1
    trajs = synthetic_trajectories(N, B, seed=11)
    legs = ("off", "on")
    trainers, stores = {}, {}
    for name in legs:
        rp = mzgo.DeviceReplay(N, B, int(1.5 * N * N), "cuda")
        for tr in trajs:
            rp.add(tr)
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 7))
        cfg = TrainConfig(unroll_steps=K, device_sampling=True, deferred_stats=True, fused_loss=True,
                          device_weights=True, fused_unroll=(name == "on"))
        trainers[name], stores[name] = MuZeroTrainer(net, cfg, mode="batched", sample_seed=3), rp

    # -- the network part alone, from fixed targets (before any step: both nets hold the same weights) --
    s = stores["off"].sample_batch(B, K, 0.99, seed=3, step=0)
    obs0, acts, t_rew, t_pol = s["obs0"], s["acts"], s["t_rew"], s["t_pol"]
    t_val = s["val"].clone()
    c = trainers["off"].config

    def net_part(name, events=None):
        tr = trainers[name]
        tr.net.zero_grad(set_to_none=True)
        if name == "on":
            lgs, vals, rews = mzgo.unroll(tr.net, obs0, acts)
        else:
            lgs, vals, rews = [], [], []
            for reward, value, logits in tr._head_outputs(obs0, acts):
                lgs.append(logits)
                vals.append(value)
                if reward is not None:
                    rews.append(reward)
            lgs, vals, rews = torch.stack(lgs), torch.stack(vals), torch.stack(rews)
        per, _ = unroll_loss(lgs, vals, rews, t_pol, t_val, t_rew, value_loss_weight=c.value_loss_weight,
                             policy_loss_weight=c.policy_loss_weight, reward_loss_weight=c.reward_loss_weight,
                             value_transform=c.use_value_transform)
        loss = per.sum()
        if events:
            events[0].record()
        loss.backward()
        if events:
            events[1].record()
        return loss

    check = {}
    for name in legs:                                       # warm-up, and the two legs compared
        for _ in range(3):
            loss = net_part(name)
        check[name] = (loss.item(), {k: p.grad.clone() for k, p in trainers[name].net.named_parameters()})
    worst = max(((check["on"][1][k] - g).abs().max() / g.abs().max().clamp_min(1.0)).item()
                for k, g in check["off"][1].items())
    agree = {"loss_off": check["off"][0], "loss_on": check["on"][0], "worst_grad_diff_over_max1": worst}
    assert abs(check["on"][0] - check["off"][0]) <= 1e-5 * abs(check["off"][0]) and worst <= 1e-3, agree

    t = {f"{k}_{n}_ms": [] for k in ("step", "net_wall", "net_event", "net_gpu", "backward_event") for n in legs}
    big = torch.randn(8192, 8192, device="cuda")
    big_out = torch.empty_like(big)
    ev = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    for name in legs:                                       # warm-up of the whole step
        for _ in range(3):
            trainers[name].train(stores[name], B)
    torch.mm(big, big, out=big_out)
    torch.cuda.synchronize()
    for _ in range(reps):
        for name in legs:
            tr = trainers[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.train(stores[name], B)
            torch.cuda.synchronize()
            t[f"step_{name}_ms"].append((time.perf_counter() - t0) / steps * 1e3)
        for name in legs:
            e0, e1 = ev()
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for _ in range(steps):
                net_part(name)
            e1.record()
            torch.cuda.synchronize()
            t[f"net_wall_{name}_ms"].append((time.perf_counter() - t0) / steps * 1e3)
            t[f"net_event_{name}_ms"].append(e0.elapsed_time(e1) / steps)
        for name in legs:
            e0, e1 = ev()
            torch.cuda.synchronize()
            for _ in range(4):
                torch.mm(big, big, out=big_out)
            e0.record()
            for _ in range(steps):
                net_part(name)
            e1.record()
            torch.cuda.synchronize()
            t[f"net_gpu_{name}_ms"].append(e0.elapsed_time(e1) / steps)
        for name in legs:
            pairs = [ev() for _ in range(steps)]
            torch.cuda.synchronize()
            for p in pairs:
                net_part(name, p)
            torch.cuda.synchronize()
            t[f"backward_event_{name}_ms"].append(sum(a.elapsed_time(b) for a, b in pairs) / steps)
    out = {"what": "the batched trainer step and its network part with TrainConfig.fused_unroll off (the per-step "
                   "torch graph, the parent path) and on (mzgo.unroll), ms per step / pass over windows of STEPS; "
                   "best / median / spread (max - min) over REPS alternating windows",
           "config": {"board_size": N, "latent_dim": C, "batch": B, "unroll": K, "steps": steps, "reps": reps},
           "expectation_before_first_run": EXPECTATION, "legs_agree": agree}
    out.update({k: _summary(v) for k, v in t.items()})
    med = lambda k: out[k]["median"]
    out["step_on_over_off"] = med("step_on_ms") / med("step_off_ms")
    out["net_wall_on_over_off"] = med("net_wall_on_ms") / med("net_wall_off_ms")
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
