"""What position-level prioritized replay (``TrainConfig.position_priorities``;
DESIGN §4 "Position-level prioritized replay") costs the device-sampled
trainer step against the game-level sampler, at main.py's sizes: 6x6, C = 128,
batch 128 x unroll 10, stores of 512 and of 5000 games (128 distinct synthetic
games with made-up root values, repeated; ``max_moves`` 54, one chunk a game).
No speed-up is claimed: the new build kernel reads ``cap x M x 8`` bytes where
the old one read ``cap x 8``, and the draw descends two more levels.

Two legs alternate in one process, each on its own store and net:

* (a) game   -- the parent's step: ``device_sampling`` + ``sample_priorities``
  (the per-game ledger, uniform starts);
* (b) position -- the same step with ``position_priorities``.

Both with ``deferred_stats``, ``fused_loss``, ``fused_unroll``,
``device_optimizer``, ``device_weights`` and search-value targets, so that
``train`` makes no synchronising call.  Per store size, each figure as best /
median / spread (max - min) over REPS alternating windows after a warm-up of
every leg:

* sampler_<leg>_events_ms / _wall_ms -- the sampler's two launches alone
  (``sample`` / ``sample_positions``), CALLS calls a window, by HIP events on
  the stream and by wall time ending in a synchronise;
* step_<leg>_ms -- the whole ``train`` step, STEPS steps a window, wall time
  ending in a synchronise.

Before timing, leg (b)'s first draw is compared with the host twin's.

Usage (GPU box): python scripts/position_sample_timing.py [out.json] -> one
JSON line (also written to out.json when given).
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


def _summary(xs):
    return {"best": min(xs), "median": statistics.median(xs), "spread": max(xs) - min(xs), "all": xs}


def _window(fn, n):
    """(wall ms, HIP-event ms) per call of ``fn(i)`` over n calls, ending in a synchronise."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, e0.elapsed_time(e1) / n


def measure(games, size, steps, reps, calls):
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    N, C, B, K, discount = 6, 128, 128, 10, 0.99
    A = N * N + 1
    legs = {"game": {}, "position": dict(position_priorities=True)}
    stores, trainers = {}, {}
    for name, extra in legs.items():
        rp = mzgo.DeviceReplay(N, size, int(1.5 * N * N), "cuda")
        for k in range(size):
            rp.add(games[k % len(games)])
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 7))
        cfg = TrainConfig(unroll_steps=K, discount=discount, device_sampling=True, sample_priorities=True,
                          deferred_stats=True, fused_loss=True, fused_unroll=True, device_optimizer=True,
                          device_weights=True, value_target="search", **extra)
        stores[name], trainers[name] = rp, MuZeroTrainer(net, cfg, mode="batched", sample_seed=3)
    stores["position"].enable_position_priorities(K, discount)      # (what the trainer's first step would do)
    got = stores["position"].sample_positions(B, seed=3, step=0)["items"].cpu().numpy()
    assert np.array_equal(got, stores["position"].sample_positions_host(B, seed=3, step=0)["items"])

    samplers = {"game": lambda i: stores["game"].sample(B, seed=5, step=i),
                "position": lambda i: stores["position"].sample_positions(B, seed=5, step=i)}
    for name, tr in trainers.items():                        # warm-up
        for _ in range(5):
            tr.train(stores[name], B)
        for i in range(20):
            samplers[name](i)
    torch.cuda.synchronize()
    t = {f"{kind}_{name}": [] for kind in ("sampler_wall", "sampler_events", "step") for name in legs}
    for _ in range(reps):
        for name in legs:
            wall, ev = _window(samplers[name], calls)
            t[f"sampler_wall_{name}"].append(wall)
            t[f"sampler_events_{name}"].append(ev)
        for name, tr in trainers.items():
            t[f"step_{name}"].append(_window(lambda i: tr.train(stores[name], B), steps)[0])
    out = {"games": size, "mean_game_length": float(np.mean(stores["game"].lengths)),
           "last_training_loss": {name: tr.read_stats().get("training_loss") for name, tr in trainers.items()},
           "skipped_updates": {name: rp.skipped_updates() for name, rp in stores.items()}}
    out.update({f"{k}_ms": _summary(v) for k, v in t.items()})
    med = lambda k: out[f"{k}_ms"]["median"]
    out["sampler_position_minus_game_ms"] = med("sampler_events_position") - med("sampler_events_game")
    out["step_position_minus_game_ms"] = med("step_position") - med("step_game")
    out["step_difference_exceeds_spread"] = bool(abs(out["step_position_minus_game_ms"]) >
                                                 max(out["step_game_ms"]["spread"], out["step_position_ms"]["spread"]))
    for rp in stores.values():
        rp.close()
    return out


def main():
    from oracle.make_golden import synthetic_trajectories
    if not torch.cuda.is_available():
        raise SystemExit("position_sample_timing: no GPU (timings are taken on the device only)")
    steps, reps, calls = (int(os.environ.get(k, d)) for k, d in (("STEPS", 100), ("REPS", 7), ("CALLS", 500)))
    sizes = [int(x) for x in os.environ.get("SIZES", "512,5000").split(",")]
    r = np.random.default_rng(11)
    games = [dict(g, root_values=[float(x) for x in r.uniform(-1, 1, len(g["actions"]))])
             for g in synthetic_trajectories(6, 128, seed=11)]
    out = {"what": "the device-sampled trainer step with the game-level sampler (a) and with position-level "
                   "prioritized replay (b), and each sampler's two launches alone, from stores of 512 and of 5000 "
                   "games; ms per step or call, best / median / spread (max - min) over REPS alternating windows",
           "config": {"board_size": 6, "latent_dim": 128, "batch": 128, "unroll": 10, "td_steps": 10, "max_moves": 54,
                      "steps": steps, "reps": reps, "calls": calls,
                      "step_flags": "device_sampling sample_priorities deferred_stats fused_loss fused_unroll "
                                    "device_optimizer device_weights value_target=search"},
           "stores": [measure(games, size, steps, reps, calls) for size in sizes]}
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
