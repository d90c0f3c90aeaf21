"""The fused unroll with ``precision="fp32"`` and ``"bf16"``
(``TrainConfig.unroll_precision``: the dynamics conv's forward, input gradient
and weight gradient on bf16 MFMA, csrc/mzgo_conv_bf16.hip) at main.py's sizes:
6x6, C = 128, batch 128 x unroll 10.  One process; the fp32 leg is the parent
path, unchanged, and the yardstick; the legs alternate.

EXPECTATION, written before the first run (DESIGN §4 "bf16 for the dynamics
conv"): of the fused unroll's 4.65 ms of kernels about 4.3 ms are the dynamics
conv's 21 matrix products (41 of 43 GFLOP at the 9 TFLOP/s of the one-wave
fp32 kernels: 0.15 ms per forward conv or chain step, 1.4 ms for the weight
pass).  The bf16 kernels are not MFMA-bound at these sizes (1.36 GFLOP per conv
is 0.5 us of the matrix cores' bf16 rate): a forward or chain launch is 128
workgroups on 256 CUs, each staging 4 slices of 4 boards behind two barriers,
so about 10-20 us per launch by its load latencies, 0.2-0.4 ms for the 20 of
them; the weight pass gathers its B fragments with 16-bit LDS reads (8 per
MFMA), so it is LDS-bound: 830 k MFMAs over 1024 SIMDs at some 100 cycles each
is 35 us, with staging perhaps 0.1 ms.  So: the network part's kernels 4.65 ->
about 0.8-1.0 ms (the representation's fp32 convs, 0.3 ms, and the heads are
what is left), several-fold as the issue's arithmetic says.  The whole step
cannot follow all the way: with 4 ms of kernels gone the host's enqueueing of a
step (sampling, targets with the bootstrap inference, loss, optimizer, weight
hand-off: about 1.5-2 ms of Python and launches) becomes the limit, so whole
step 4.8 -> about 2 ms.  What could undo it: LDS bank conflicts of the 16-bit
gathers and of the 2-byte staging writes in the weight pass; then it, not the
convs, is the new floor.

Figures, each best / median / spread (max - min) over REPS alternating windows
after a warm-up of both legs:

* step_fp32_ms / step_bf16_ms            the whole ``train`` step from a
                                         ``DeviceReplay`` with device_sampling +
                                         deferred_stats + fused_loss + fused_unroll
                                         + device_optimizer + device_weights
                                         (network value targets), wall time over
                                         STEPS steps ending in a synchronise;
* net_event_fp32_ms / net_event_bf16_ms  forward + backward of the network part
                                         alone from fixed targets (``mzgo.unroll``,
                                         ``unroll_loss``, ``backward``) by HIP
                                         events over STEPS passes;
* net_gpu_fp32_ms / net_gpu_bf16_ms      the same window enqueued behind a long
                                         matmul: the kernels back to back without
                                         the host.

Both legs' losses at the same weights and targets, and the relative distance
of their gradients, are recorded (``legs``), as are the three step losses of
each trainer's warm-up.

Usage (GPU box): python scripts/unroll_bf16_timing.py [out.json] -> one JSON
line (also written to out.json when given).
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
    "fp32_network_part_kernels_ms": 4.65,
    "of_which_dynamics_conv_ms": 4.3,
    "bf16_forward_or_chain_launch_us": "10-20 (latency-bound: 128 workgroups, 4 staged slices each)",
    "bf16_weight_pass_ms": "about 0.1 (LDS-bound: 8 16-bit reads per MFMA)",
    "network_part_ms": "4.65 -> about 0.8-1.0",
    "whole_step_ms": "4.8 -> about 2 (the host's enqueueing becomes the limit)",
    "risk": "LDS bank conflicts of the weight pass's 16-bit gathers and 2-byte staging writes",
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
    legs = ("fp32", "bf16")
    trainers, stores = {}, {}
    for name in legs:
        rp = mzgo.DeviceReplay(N, B, int(1.5 * N * N), "cuda")
        for tr in trajs:
            rp.add(tr)
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 7))
        cfg = TrainConfig(unroll_steps=K, device_sampling=True, deferred_stats=True, fused_loss=True,
                          device_weights=True, fused_unroll=True, device_optimizer=True, unroll_precision=name)
        trainers[name], stores[name] = MuZeroTrainer(net, cfg, mode="batched", sample_seed=3), rp

    # -- the network part alone, from fixed targets (before any step: both nets hold the same weights) --
    s = stores["fp32"].sample_batch(B, K, 0.99, seed=3, step=0)
    obs0, acts, t_rew, t_pol = s["obs0"], s["acts"], s["t_rew"], s["t_pol"]
    t_val = s["val"].clone()
    c = trainers["fp32"].config

    def net_part(name):
        tr = trainers[name]
        tr.net.zero_grad(set_to_none=True)
        lgs, vals, rews = mzgo.unroll(tr.net, obs0, acts, precision=name)
        per, _ = unroll_loss(lgs, vals, rews, t_pol, t_val, t_rew, value_loss_weight=c.value_loss_weight,
                             policy_loss_weight=c.policy_loss_weight, reward_loss_weight=c.reward_loss_weight,
                             value_transform=c.use_value_transform)
        loss = per.sum()
        loss.backward()
        return loss

    check = {}
    for name in legs:                                       # warm-up, and the two legs compared
        for _ in range(3):
            loss = net_part(name)
        check[name] = (loss.item(), {k: p.grad.clone() for k, p in trainers[name].net.named_parameters()})
    rel = {k: ((check["bf16"][1][k] - g).norm() / g.norm().clamp_min(1e-30)).item() for k, g in check["fp32"][1].items()}
    agree = {"loss_fp32": check["fp32"][0], "loss_bf16": check["bf16"][0],
             "loss_relative_distance": abs(check["bf16"][0] / check["fp32"][0] - 1),
             "grad_relative_distance_worst": max(rel.values()), "grad_relative_distance": rel}

    t = {f"{k}_{n}_ms": [] for k in ("step", "net_event", "net_gpu") for n in legs}
    big = torch.randn(8192, 8192, device="cuda")
    big_out = torch.empty_like(big)
    ev = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    step_losses = {name: [] for name in legs}
    for name in legs:                                       # warm-up of the whole step; its losses
        for _ in range(3):
            trainers[name].train(stores[name], B)
            step_losses[name].append(float(dict(trainers[name].read_stats())["training_loss"]))
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
            for _ in range(steps):
                net_part(name)
            e1.record()
            torch.cuda.synchronize()
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
        step_losses[name].append(float(dict(trainers[name].read_stats())["training_loss"]))
    out = {"what": "the batched trainer step and its network part on mzgo.unroll with precision fp32 (the parent "
                   "path) and bf16 (the dynamics conv's three products on bf16 MFMA), ms per step / pass over "
                   "windows of STEPS; best / median / spread (max - min) over REPS alternating windows",
           "config": {"board_size": N, "latent_dim": C, "batch": B, "unroll": K, "steps": steps, "reps": reps,
                      "value_target": "network"},
           "expectation_before_first_run": EXPECTATION, "legs": agree,
           "step_losses_warmup_then_last": step_losses}
    out.update({k: _summary(v) for k, v in t.items()})
    med = lambda k: out[k]["median"]
    out["step_bf16_over_fp32"] = med("step_bf16_ms") / med("step_fp32_ms")
    out["net_event_bf16_over_fp32"] = med("net_event_bf16_ms") / med("net_event_fp32_ms")
    out["net_gpu_bf16_over_fp32"] = med("net_gpu_bf16_ms") / med("net_gpu_fp32_ms")
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
