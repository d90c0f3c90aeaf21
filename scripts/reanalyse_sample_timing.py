"""Reanalysis of a sampled batch's windows (``DeviceReplay.reanalyse_sample``,
``TrainConfig.reanalyse_sample``) at main.py's sizes: 6x6, C = 128, batch 128 x
unroll 10, 256 simulations, a store filled by ``play_games_into``.  The legs
alternate in one process, as scripts/unroll_timing.py's do.

EXPECTATION, written before the first run (DESIGN §4 "Reanalysis of the
sampled windows"): a batch's windows hold at most B (K + 1) = 1408 positions,
about 360 k simulations; at the 9x9 queue's 135 M simulations/s that would be
under 3 ms, but the 6x6 reanalysis rate has never been measured.  Against the
parent's offer (copy the indices back, search every position of the sampled
games) the window call should win by about the ratio of positions searched;
against the staging path on the same item list it should be within a few
percent; the whole step grows from 5.4 ms by the searches' time.  No threshold.

Figures, each best / median / spread (max - min) over REPS alternating windows
after a warm-up of every leg, wall time of one call ending in a synchronise:

* window_ms        ``reanalyse_sample`` on a drawn sample's device items;
* whole_games_ms   what the parent commit offers for the same batch: the
                   sample's indices copied to the host, then
                   ``DeviceReplay.reanalyse(games=indices)``;
* staging_ms       the same item list through ``Engine.reanalyse`` from
                   gathered buffers (gathered once, outside the timing: the
                   staging path less its gather and scatter launches);
* first_256_ms / last_256_ms   the list's first 256 items (the latest moves,
                   one per CU) and its last 256 through ``Engine.reanalyse``:
                   every CU busy with one search;
* first_256_each_ms   each of those first 256 items alone, once: the median
                   and the largest single search, and its move;
* item_move_<t>_ms  one item of move t alone through ``Engine.reanalyse``, for
                   a few t from the list's last (move 0) to its first (the
                   latest move): one search on one CU, and the launch's floor;
* step_off_ms / step_on_ms   the whole ``train`` step with device_sampling +
                   deferred_stats + fused_loss + device_weights + fused_unroll,
                   ``reanalyse_sample`` off and on, over STEPS steps.

Before timing, the window leg's rows are compared bit for bit with the
whole-game leg's on a second store with the same games.

Usage (GPU box): python scripts/reanalyse_sample_timing.py [out.json] -> one
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

EXPECTATION = {
    "window_positions_at_most": 1408,
    "simulations_at_most": 360448,
    "at_the_9x9_queue_rate_ms": "under 3 (135 M simulations/s; the 6x6 reanalysis rate was never measured)",
    "against_whole_games": "faster by about the ratio of positions searched",
    "against_staging": "within a few percent",
    "whole_step_ms": "5.4 + the searches' time",
    "threshold": None,
}


def _summary(xs):
    return {"best": min(xs), "median": statistics.median(xs), "spread": max(xs) - min(xs), "all": xs}


def main():
    import mzgo
    from mzgo.reanalyse import Reanalyser, positions_from_planes
    from mzgo.trainer import MainSelfPlay, MuZeroTrainer, TrainConfig
    steps, reps = (int(os.environ.get(k, d)) for k, d in (("STEPS", 5), ("REPS", 7)))
    N, C, B, K, S = 6, 128, 128, 10, 256
    A, games, play_sims = N * N + 1, 256, 32

    def make_net():
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 7))
        return net

    def filled_store():                                     # the same games every time
        msp = MainSelfPlay(make_net().eval(), 128, play_sims, seed=17)
        rp = mzgo.DeviceReplay(N, games, msp.max_moves, "cuda")
        msp.play_games_into(rp, games)
        return rp

    rp, rp2 = filled_store(), filled_store()
    lengths = np.array(rp.lengths)
    net = make_net().eval()
    ra = Reanalyser(net, S)
    s = rp.sample(B, seed=3, step=0)
    idx = s["index"].cpu().numpy()
    items = rp.window_items_host(s, K)

    # the staging leg's buffers: the item list's positions, gathered on the host once
    pos = {}
    for g in sorted(set(items[:, 0].tolist())):             # (slot = logical index: the ring has not wrapped)
        e = rp.export(g)
        pos[g] = positions_from_planes(np.asarray(e["observations"][:len(e["actions"])])), e["key_gid"]
    st, iv, fl = (torch.stack([pos[g][0][j][t] for g, t in items.tolist()]).cuda() for j in range(3))
    ids = torch.tensor([(pos[g][1], t) for g, t in items.tolist()], dtype=torch.int32).cuda()

    def window():
        return rp.reanalyse_sample(ra, s, K)

    def whole_games():
        rp2.reanalyse(ra, games=s["index"].cpu().numpy())

    def staging():
        return ra.engine.reanalyse(st, iv, fl, ids)

    # the legs agree: inside the windows the same bits
    n = window()
    whole_games()
    _, _, pol = staging()
    torch.cuda.synchronize()
    assert n.item() == len(items), (n.item(), len(items))
    for g in pos:
        a, b = rp.export(g), rp2.export(g)
        for t in items[items[:, 0] == g][:, 1]:
            assert np.array_equal(a["policies"][t], b["policies"][t]), (g, t)
    first = items[0].tolist()
    assert np.array_equal(pol[0].cpu().numpy(), rp.export(first[0])["policies"][first[1]])

    trainers, stores = {}, {"off": rp2, "on": filled_store()}
    for name in ("off", "on"):
        tnet = make_net()
        cfg = TrainConfig(unroll_steps=K, device_sampling=True, deferred_stats=True, fused_loss=True,
                          device_weights=True, fused_unroll=True, reanalyse_sample=(name == "on"))
        trainers[name] = MuZeroTrainer(tnet, cfg, mode="batched", sample_seed=3,
                                       reanalyser=Reanalyser(tnet, S) if name == "on" else None)

    one = lambda i: (lambda: ra.engine.reanalyse(st[i:i + 1], iv[i:i + 1], fl[i:i + 1], ids[i:i + 1]))
    part = lambda a, b: (lambda: ra.engine.reanalyse(st[a:b], iv[a:b], fl[a:b], ids[a:b]))
    legs = {"window": window, "whole_games": whole_games, "staging": staging, "first_256": part(0, 256),
            "last_256": part(len(items) - 256, len(items))}
    for t_move in sorted({0, 5, 10, 20, 30, 40, int(items[0, 1])}):
        at = np.flatnonzero(items[:, 1] == t_move)
        if len(at):
            legs[f"item_move_{t_move}"] = one(int(at[0]))
    t = {f"{k}_ms": [] for k in (*legs, "step_off", "step_on")}
    for fn in legs.values():                                # warm-up
        fn()
    for name in trainers:
        for _ in range(3):
            trainers[name].train(stores[name], B)
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[f"{name}_ms"].append((time.perf_counter() - t0) * 1e3)
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.train(stores[name], B)
            torch.cuda.synchronize()
            t[f"step_{name}_ms"].append((time.perf_counter() - t0) / steps * 1e3)

    each = []
    for i in range(min(256, len(items))):                   # (after the timed windows; one pass)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one(i)()
        torch.cuda.synchronize()
        each.append((time.perf_counter() - t0) * 1e3)
    whole = int(lengths[idx].sum())
    out = {"what": "reanalysis of a sampled batch's windows in the store (reanalyse_sample) against whole-game "
                   "reanalysis of the sampled games from host indices (the parent's offer) and against the same item "
                   "list through Engine.reanalyse from gathered buffers; the whole trainer step with "
                   "TrainConfig.reanalyse_sample off and on; ms, best / median / spread (max - min) over REPS "
                   "alternating windows",
           "config": {"board_size": N, "latent_dim": C, "batch": B, "unroll": K, "simulations": S,
                      "stored_games": games, "fill_simulations": play_sims, "steps": steps, "reps": reps,
                      "reanalyser_slots": ra.engine.G},
           "expectation_before_first_run": EXPECTATION,
           "window_positions": int(len(items)), "whole_game_positions": whole,
           "items_per_move": np.bincount(items[:, 1]).tolist(),
           "first_256_each_ms": {"median": statistics.median(each), "max": max(each),
                                 "max_item": items[int(np.argmax(each))].tolist(),
                                 "over_20_ms": int(sum(x > 20.0 for x in each)), "sum": sum(each)},
           "mean_game_length": float(lengths.mean())}
    out.update({k: _summary(v) for k, v in t.items()})
    med = lambda k: out[k]["median"]
    out["window_simulations_per_s"] = len(items) * S / (med("window_ms") * 1e-3)
    out["whole_games_simulations_per_s"] = whole * S / (med("whole_games_ms") * 1e-3)
    out["window_over_whole_games"] = med("window_ms") / med("whole_games_ms")
    out["window_over_staging"] = med("window_ms") / med("staging_ms")
    out["step_on_minus_off_ms"] = med("step_on_ms") - med("step_off_ms")
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
