"""The latent consistency loss's cost at main.py's sizes (6x6, latent_dim 128,
batch 128, unroll 10, proj_dim 32), one process, every device switch on
(``device_sampling``, ``deferred_stats``, ``device_weights``, ``fused_unroll``,
``fused_loss``, ``device_optimizer``):

* step_off_ms / step_cons_ms  the whole ``trainer.train`` step with
                              ``consistency_loss_weight`` 0 and 0.5: wall time
                              over a window of STEPS steps, synchronised at the
                              window's ends only.
* cons_hip_*_ms / cons_torch_*_ms
                              the head + loss + backward alone on latents the
                              unroll returned (detached) and fixed targets: on
                              ``mzgo.consistency_loss`` (two launches each way)
                              and written with torch ops (two ``conv2d``,
                              ``relu``, ``F.cosine_similarity``) under
                              autograd, the same tensors in, the same five
                              gradients out.  ``event``: between two events on
                              an idle stream (the host's enqueueing included);
                              ``gpu``: the same window enqueued behind a long
                              matmul (the kernels back to back without the
                              host).
* encode_*_ms                 ``mzgo.encode`` of the K B real boards alone.
* window_obs_event_ms         ``DeviceReplay.window_obs_from`` alone.

The two legs' losses and gradients at the same inputs are recorded (``agree``).

Usage (GPU box): python scripts/consistency_timing.py [--out profiles/consistency_timing.json]
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
    "latents_MB": "23.6 each for latents[1:] and the targets (1280 rows x 128 x 36 floats)",
    "traffic_MB": "about 150: the forward reads both (47) and writes u, p, z (18); the backward reads the latents and "
                  "u, p, z (41, the latter several times through L1 / L2), writes g_latents (26) and the partials "
                  "(427 chunks x 20 KB = 9), the reduce reads them (9)",
    "consistency_kernels_gpu_ms": "0.08-0.15: 150 MB at 2-3 TB/s is 0.05-0.08 ms; the backward's MFMAs (every wave "
                                  "forms g_r for every tile) are about 14 us spread over the CUs, next to it",
    "torch_ops_gpu_ms": "0.5-1.0: three 1x1 convs forward and four matrix products backward through the library, a "
                        "slice backward that zero-fills and copies 26 MB, and some fifteen elementwise / reduction "
                        "passes over [1280, 1152] or larger",
    "encode_gpu_ms": "0.3-0.6: three 3x3 convs of 1280 boards; 64 -> 128 channels at 36 cells is 0.7 GFLOP x ~9 "
                     "= the larger cost, as the issue supposes",
    "step_ms": "the step is bound by the host's enqueueing; the option adds three library calls, one autograd node and "
               "about ten allocations: +5-10 %",
    "risk": "the backward's strided 16-byte loads for the weight gradients' cell contraction; 25 % of the MFMA work "
            "at 36 cells is padding (3 tiles of 16)",
}


def _summary(xs):
    return {"best": min(xs), "median": statistics.median(xs), "spread": max(xs) - min(xs), "all": xs}


def main():
    import torch.nn.functional as F

    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    from oracle.make_golden import synthetic_trajectories
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_timing.json"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    steps, reps = args.steps, args.reps
    N, C, P, B, K, W = 6, 128, 32, 128, 10, 0.5
    A = N * N + 1
    trajs = list(synthetic_trajectories(N, B, seed=11))
    legs = {"off": 0.0, "cons": W}
    trainers, stores = {}, {}
    for name, weight in legs.items():
        rp = mzgo.DeviceReplay(N, B, int(1.5 * N * N), "cuda")
        for tr in trajs:
            rp.add(tr)
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 7))
        torch.manual_seed(1)
        cfg = TrainConfig(unroll_steps=K, device_sampling=True, deferred_stats=True, fused_loss=True,
                          device_weights=True, fused_unroll=True, device_optimizer=True,
                          consistency_loss_weight=weight)
        trainers[name], stores[name] = MuZeroTrainer(net, cfg, mode="batched", sample_seed=3), rp

    # -- the head + loss + backward alone, on fixed latents and targets --
    rp, net = stores["cons"], trainers["cons"].net
    s = rp.sample_batch(B, K, 0.99, seed=3, step=0)
    obs_k, mask = rp.window_obs_from(s, K)
    boards = obs_k.view(K * B, 6, N, N)
    targets = mzgo.encode(net, boards).view(K, B, C, N, N)
    with torch.no_grad():
        latents = mzgo.unroll(net, s["obs0"], s["acts"], return_latents=True)[3].clone()
    head = mzgo.ConsistencyHead(C, P).cuda()
    m_steps = mask.t().contiguous()                         # [K, B]: the torch leg's layout, made once
    t_flat = targets.view(K * B, C, N, N)

    def cons_hip():
        lat = latents.requires_grad_()
        lat.grad = None
        head.zero_grad(set_to_none=True)
        per, _ = mzgo.consistency_loss(lat, targets, mask, head, W)
        loss = per.sum()
        loss.backward()
        return loss, lat.grad

    def cons_torch():
        lat = latents.requires_grad_()
        lat.grad = None
        head.zero_grad(set_to_none=True)
        u = F.conv2d(lat[1:].reshape(K * B, C, N, N), head.proj.weight, head.proj.bias)
        p = F.conv2d(F.relu(u), head.pred.weight, head.pred.bias).view(K * B, -1)
        with torch.no_grad():
            z = F.conv2d(t_flat, head.proj.weight, head.proj.bias).view(K * B, -1)
        cos = F.cosine_similarity(p, z, dim=1, eps=1e-8).view(K, B)
        per = W * (m_steps * (1 - cos)).sum(dim=0)
        loss = per.sum()
        loss.backward()
        return loss, lat.grad

    parts = {"hip": cons_hip, "torch": cons_torch}
    check = {}
    for name, fn in parts.items():
        for _ in range(3):
            loss, g = fn()
        check[name] = (loss.item(), g.clone(), [p.grad.clone() for p in head.parameters()])
    rel = lambda a, b: ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
    agree = {"loss_hip": check["hip"][0], "loss_torch": check["torch"][0],
             "g_latents_relative_distance": rel(check["hip"][1], check["torch"][1]),
             "masked_rows": int((mask == 0).sum().item()), "rows": mask.numel()}
    for k, a, b in zip(("proj_w", "proj_b", "pred_w", "pred_b"), check["hip"][2], check["torch"][2]):
        agree[f"g_{k}_relative_distance"] = rel(a, b)

    t = {f"step_{n}_ms": [] for n in legs}
    t.update({f"cons_{n}_{k}_ms": [] for n in parts for k in ("event", "gpu")})
    t.update({"encode_event_ms": [], "encode_gpu_ms": [], "window_obs_event_ms": []})
    big = torch.randn(8192, 8192, device="cuda")
    big_out = torch.empty_like(big)
    ev = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))

    def window(fn, kind):
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
        return e0.elapsed_time(e1) / steps

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
                t[f"cons_{name}_{kind}_ms"].append(window(fn, kind))
        for kind in ("event", "gpu"):
            t[f"encode_{kind}_ms"].append(window(lambda: mzgo.encode(net, boards), kind))
        t["window_obs_event_ms"].append(window(lambda: rp.window_obs_from(s, K), "event"))
    out = {"what": "the batched trainer step with consistency_loss_weight 0 (the parent path) and 0.5; the consistency "
                   "head + loss + backward alone on mzgo.consistency_loss and on torch ops; mzgo.encode of the K B "
                   "boards; ms per step / pass over windows of STEPS; best / median / spread (max - min) over REPS "
                   "alternating windows",
           "config": {"board_size": N, "latent_dim": C, "proj_dim": P, "batch": B, "unroll": K, "steps": steps,
                      "reps": reps, "consistency_loss_weight": W, "value_target": "network"},
           "expectation_before_first_run": EXPECTATION, "agree": agree, "step_stats_warmup": step_losses}
    out.update({k: _summary(v) for k, v in t.items()})
    med = lambda k: out[k]["median"]
    out["step_cons_over_off"] = med("step_cons_ms") / med("step_off_ms")
    out["step_cons_minus_off_ms"] = med("step_cons_ms") - med("step_off_ms")
    out["cons_hip_over_torch_gpu"] = med("cons_hip_gpu_ms") / med("cons_torch_gpu_ms")
    out["cons_hip_over_torch_event"] = med("cons_hip_event_ms") / med("cons_torch_event_ms")
    out["cons_torch_minus_hip_gpu_ms"] = med("cons_torch_gpu_ms") - med("cons_hip_gpu_ms")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("step_stats_warmup", "expectation_before_first_run")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
