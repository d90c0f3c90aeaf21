"""The ownership auxiliary target's cost at main.py's sizes (6x6, latent_dim
128, batch 128, unroll 10), one process, every device switch on
(``device_sampling``, ``deferred_stats``, ``device_weights``, ``fused_unroll``,
``fused_loss``, ``device_optimizer``):

* step_off_ms / step_own_ms   the whole ``trainer.train`` step with
                              ``ownership_loss_weight`` 0 and 0.5: wall time
                              over a window of STEPS steps, synchronised at the
                              window's ends only.
* own_hip_*_ms / own_torch_*_ms
                              the ownership part alone on latents the unroll
                              returned (detached): the head, the loss, the sum
                              and the backward to the latents and the head's two
                              parameters -- on ``mzgo.ownership_loss`` (two
                              launches each way) and written with torch ops
                              (``conv2d``, ``logaddexp``, ...) under autograd.
                              ``event``: between two events on an idle stream
                              (the host's enqueueing included); ``gpu``: the
                              same window enqueued behind a long matmul (the
                              kernels back to back without the host).
* targets_event_ms            ``DeviceReplay.ownership_from`` alone.

The two ownership legs' losses and gradients at the same inputs are recorded
(``agree``).  Every stored game carries the done bit, so every row inside a
game has a target (a row past the final board is masked, as in training).

Usage (GPU box): python scripts/ownership_timing.py [--out profiles/ownership_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "muzero-go_amd")]

import torch  # noqa: E402

# written before the first run (DESIGN §4 quotes it next to the measurement)
EXPECTATION = {
    "latents_MB": 25.9,
    "traffic_MB": "about 156: the forward reads the latents (26), the backward reads them and writes g_lat (52), "
                  "the add reads two and writes one (78)",
    "ownership_kernels_gpu_ms": "0.06-0.12: 156 MB at 2-3 TB/s reached by launches this small is 0.05-0.08 ms, plus "
                                "six launches (targets, 2 forward, 2 backward, the add) of a few us each",
    "torch_ops_gpu_ms": "0.3-0.5: a 1x1 conv through MIOpen forward and twice backward, and some ten elementwise "
                        "passes each way",
    "step_ms": "4.8 -> 5.0-5.2 (+4-8 %): the step is bound by the host's enqueueing, and the feature adds two "
               "autograd nodes, three library calls and seven allocations to it",
    "risk": "k_ownership_loss_bwd's wave-per-channel loop at 36 cells uses 36 of 64 lanes per load",
}


def _summary(xs):
    return {"best": min(xs), "median": statistics.median(xs), "spread": max(xs) - min(xs), "all": xs}


def main():
    import torch.nn.functional as F

    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    from oracle.make_golden import synthetic_trajectories
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ownership_timing.json"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    steps, reps = args.steps, args.reps
    N, C, B, K, W = 6, 128, 128, 10, 0.5
    A = N * N + 1
    trajs = []
    for t in synthetic_trajectories(N, B, seed=11):
        T = len(t["actions"])
        obs = [o.copy() for o in t["observations"]]
        for o in obs[T:]:
            o[5] = 1.0                                      # the game ended: its final board has owners
        trajs.append(dict(t, observations=obs))
    legs = {"off": 0.0, "own": W}
    trainers, stores = {}, {}
    for name, weight in legs.items():
        rp = mzgo.DeviceReplay(N, B, int(1.5 * N * N), "cuda")
        for tr in trajs:
            rp.add(tr)
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 7))
        torch.manual_seed(1)
        cfg = TrainConfig(unroll_steps=K, device_sampling=True, deferred_stats=True, fused_loss=True,
                          device_weights=True, fused_unroll=True, device_optimizer=True, ownership_loss_weight=weight)
        trainers[name], stores[name] = MuZeroTrainer(net, cfg, mode="batched", sample_seed=3), rp

    # -- the ownership part alone, on fixed latents and targets --
    rp = stores["own"]
    s = rp.sample_batch(B, K, 0.99, seed=3, step=0)
    t_own, mask = rp.ownership_from(s, K)
    with torch.no_grad():
        latents = mzgo.unroll(trainers["own"].net, s["obs0"], s["acts"], return_latents=True)[3].clone()
    head = mzgo.OwnershipHead(C).cuda()
    t_steps = t_own.transpose(0, 1).contiguous()            # [K+1, B, CELLS]: the torch leg's layout, made once
    m_steps = mask.t().contiguous()

    def own_hip():
        lat = latents.requires_grad_()
        lat.grad = None
        head.zero_grad(set_to_none=True)
        per, _ = mzgo.ownership_loss(lat, head, t_own, mask, W)
        loss = per.sum()
        loss.backward()
        return loss, lat.grad

    def own_torch():
        lat = latents.requires_grad_()
        lat.grad = None
        head.zero_grad(set_to_none=True)
        x = head.conv(lat.view(-1, C, N, N)).view(K + 1, B, N * N)
        cell = torch.logaddexp(torch.zeros_like(x), 2 * x) - (1 + t_steps) * x
        per = W * (m_steps * cell.mean(dim=2)).sum(dim=0)
        loss = per.sum()
        loss.backward()
        return loss, lat.grad

    parts = {"hip": own_hip, "torch": own_torch}
    check = {}
    for name, fn in parts.items():
        for _ in range(3):
            loss, g = fn()
        check[name] = (loss.item(), g.clone(), head.conv.weight.grad.clone())
    rel = lambda a, b: ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
    agree = {"loss_hip": check["hip"][0], "loss_torch": check["torch"][0],
             "g_latents_relative_distance": rel(check["hip"][1], check["torch"][1]),
             "g_w_relative_distance": rel(check["hip"][2], check["torch"][2]),
             "masked_rows": int((mask == 0).sum().item()), "rows": mask.numel()}

    t = {f"step_{n}_ms": [] for n in legs}
    t.update({f"own_{n}_{k}_ms": [] for n in parts for k in ("event", "gpu")})
    t["targets_event_ms"] = []
    big = torch.randn(8192, 8192, device="cuda")
    big_out = torch.empty_like(big)
    ev = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    step_losses = {n: [] for n in legs}
    for name in legs:                                       # warm-up of the whole step; its losses
        for _ in range(3):
            trainers[name].train(stores[name], B)
            step_losses[name].append({k: float(v) for k, v in trainers[name].read_stats().items()})
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
        for name, fn in parts.items():
            for kind in ("event", "gpu"):
                e0, e1 = ev()
                torch.cuda.synchronize()
                if kind == "gpu":
                    for _ in range(4):
                        torch.mm(big, big, out=big_out)
                e0.record()
                for _ in range(steps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                t[f"own_{name}_{kind}_ms"].append(e0.elapsed_time(e1) / steps)
        e0, e1 = ev()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            rp.ownership_from(s, K)
        e1.record()
        torch.cuda.synchronize()
        t["targets_event_ms"].append(e0.elapsed_time(e1) / steps)
    out = {"what": "the batched trainer step with ownership_loss_weight 0 (the parent path) and 0.5, and the ownership "
                   "head + loss alone on mzgo.ownership_loss and on torch ops, ms per step / pass over windows of "
                   "STEPS; best / median / spread (max - min) over REPS alternating windows",
           "config": {"board_size": N, "latent_dim": C, "batch": B, "unroll": K, "steps": steps, "reps": reps,
                      "ownership_loss_weight": W, "value_target": "network"},
           "expectation_before_first_run": EXPECTATION, "agree": agree, "step_stats_warmup": step_losses}
    out.update({k: _summary(v) for k, v in t.items()})
    med = lambda k: out[k]["median"]
    out["step_own_over_off"] = med("step_own_ms") / med("step_off_ms")
    out["step_own_minus_off_ms"] = med("step_own_ms") - med("step_off_ms")
    out["own_hip_over_torch_gpu"] = med("own_hip_gpu_ms") / med("own_torch_gpu_ms")
    out["own_hip_over_torch_event"] = med("own_hip_event_ms") / med("own_torch_event_ms")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
