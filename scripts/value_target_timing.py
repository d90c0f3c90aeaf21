"""Search-value targets (``DeviceReplay.sample_batch_values``,
``TrainConfig.value_target="search"``) against network targets at main.py's
sizes: 6x6, C = 128, batch 128 x unroll 10, a store filled by
``play_games_into``.  The legs alternate in one process, as
scripts/replay_timing.py's do.

EXPECTATION, written before the first run (DESIGN §4 "Search-value targets"):
nobody has timed the bootstrap on its own.  The network path writes B (K + 1)
= 1408 bootstrap observations (1.2 MB of f32), runs one ``initial_inference``
over them and one finishing launch; the search path does none of that and its
plane loop covers one row instead of K + 2.  With ``device_weights`` the
inference needs one pack launch after each optimizer step; without it the 22
tensors go through the host.  No speed-up is promised and no threshold is set.

Figures, each best / median / spread (max - min) over REPS alternating windows
after a warm-up of every leg, wall time ending in a synchronise, per call:

* targets_network_ms   ``sample_batch`` + ``initial_inference`` over the
                       bootstrap rows + ``finish_values`` (the weights already
                       in the engine: no reload in this leg);
* targets_search_ms    ``sample_batch_values``;
* step_<network|search>_dw<0|1>_ms   the whole ``train`` step with
                       device_sampling + deferred_stats + fused_loss +
                       fused_unroll + device_optimizer under each
                       ``value_target``, with ``device_weights`` on (1) and
                       off (0), over STEPS steps.

Before timing, the search leg's ``t_val`` is compared bit for bit with
``value_targets_host`` on the exported games.

Usage (GPU box): python scripts/value_target_timing.py [out.json] -> one JSON
line (also written to out.json when given).
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

EXPECTATION = {
    "bootstrap_rows": 1408,
    "network_path": "sample_batch + one initial_inference over 1408 rows + finish_values",
    "search_path": "sample_batch_values alone; the plane loop covers 1 row instead of 12",
    "speed_up": "not promised: the bootstrap has never been timed on its own",
    "threshold": None,
}


def _summary(xs):
    return {"best": min(xs), "median": statistics.median(xs), "spread": max(xs) - min(xs), "all": xs}


def main():
    import mzgo
    from mzgo.replay import finish_values
    from mzgo.trainer import MainSelfPlay, MuZeroTrainer, TrainConfig
    steps, reps, calls = (int(os.environ.get(k, d)) for k, d in (("STEPS", 100), ("REPS", 9), ("CALLS", 1000)))
    N, C, B, K = 6, 128, 128, 10
    A, games, play_sims, discount = N * N + 1, 256, 32, 0.99
    if not torch.cuda.is_available():
        raise SystemExit("value_target_timing: no GPU (timings are taken on the device only)")

    def make_net():
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 7))
        return net

    def filled_store():                                     # the same games every time
        msp = MainSelfPlay(make_net().eval(), 128, play_sims, seed=17)
        rp = mzgo.DeviceReplay(N, games, msp.max_moves, "cuda")
        msp.play_games_into(rp, games)
        return rp

    rp = filled_store()
    net = make_net().eval()
    draw = lambda step: dict(seed=3, step=step)

    def targets_network(step):
        s = rp.sample_batch(B, K, discount, **draw(step))
        with torch.no_grad():
            _, v, _ = net.initial_inference(s["boot_obs"].view(-1, 6, N, N))
        return finish_values(s["val"], s["factor"], s["has_boot"], v)

    def targets_search(step):
        return rp.sample_batch_values(B, K, K, discount, **draw(step))["t_val"]

    # the search leg is the rule: its t_val equals the host twin's on the exported games
    s = rp.sample_batch_values(B, K, K, discount, **draw(0))
    items = s["items"].cpu().numpy()
    exported = {int(g): rp.export(int(g)) for g in items[:, 0]}        # (slot = logical index: the ring has not wrapped)
    want = np.stack([mzgo.value_targets_host(exported[int(g)]["rewards"], exported[int(g)]["root_values"], int(st), K, K,
                                             discount) for g, st, _ in items])
    assert np.array_equal(s["t_val"].cpu().numpy().view(np.uint32), want.view(np.uint32))
    bootstrap_rows = int(rp.sample_batch(B, K, discount, **draw(0))["has_boot"].sum().item())

    trainers, stores = {}, {}
    for vt in ("network", "search"):
        for dw in (1, 0):
            name = f"step_{vt}_dw{dw}"
            cfg = TrainConfig(unroll_steps=K, device_sampling=True, deferred_stats=True,
                              fused_loss=True, fused_unroll=True, device_optimizer=True, device_weights=bool(dw),
                              value_target=vt)
            trainers[name] = MuZeroTrainer(make_net(), cfg, mode="batched", sample_seed=3)
            stores[name] = filled_store()

    legs = {"targets_network": targets_network, "targets_search": targets_search}
    t = {f"{k}_ms": [] for k in (*legs, *trainers)}
    for fn in legs.values():                                # warm-up
        for i in range(5):
            fn(i)
    for name, tr in trainers.items():
        for _ in range(5):
            tr.train(stores[name], B)
    torch.cuda.synchronize()
    for rep in range(reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(calls):
                fn(rep * calls + i)
            torch.cuda.synchronize()
            t[f"{name}_ms"].append((time.perf_counter() - t0) / calls * 1e3)
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.train(stores[name], B)
            torch.cuda.synchronize()
            t[f"{name}_ms"].append((time.perf_counter() - t0) / steps * 1e3)
    losses = {name: tr.read_stats().get("training_loss") for name, tr in trainers.items()}

    out = {"what": "value-target production (sample_batch + bootstrap initial_inference + finish_values against "
                   "sample_batch_values) and the whole device-sampled trainer step under value_target='network' and "
                   "'search', with device_weights on and off; ms per call or step, best / median / spread (max - "
                   "min) over REPS alternating windows",
           "config": {"board_size": N, "latent_dim": C, "batch": B, "unroll": K, "td_steps": K, "stored_games": games,
                      "fill_simulations": play_sims, "steps": steps, "reps": reps, "calls": calls,
                      "step_flags": "device_sampling deferred_stats fused_loss fused_unroll device_optimizer"},
           "expectation_before_first_run": EXPECTATION,
           "bootstrap_rows_with_a_position": bootstrap_rows, "bootstrap_rows_evaluated": B * (K + 1),
           "mean_game_length": float(np.mean(rp.lengths)), "last_training_loss": losses}
    out.update({k: _summary(v) for k, v in t.items()})
    med = lambda k: out[k]["median"]
    out["targets_search_over_network"] = med("targets_search_ms") / med("targets_network_ms")
    for dw in (1, 0):
        out[f"step_search_minus_network_dw{dw}_ms"] = med(f"step_search_dw{dw}_ms") - med(f"step_network_dw{dw}_ms")
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
