"""Reanalysis rate against the two other ways to search the same positions.

On 9x9 with 256 games and 200 simulations (bench.py's flagship shape):

1. ``epoch``     play one move-parallel epoch with launch timing on and keep
                 every recorded position; the epoch's own k_search_queue time
                 is the yardstick (the same searches, the same schedule);
2. ``reanalyse`` run all recorded positions through ``Engine.reanalyse``
                 (k_reanalyse_queue) with the records' keys, policy included
                 (and, to place a gap: without the policy, and with the items
                 latest move first, k_search_queue's order);
3. ``search``    push the same positions through ``Engine.search`` 256 at a
                 time -- the only way to search stored positions before.

Writes positions/s and simulations/s of all three, and the reanalysis /
queue ratio, to profiles/reanalyse_timing.json.  Every step is a fresh child
process under its own time limit; the first one that fails ends the script.

    python scripts/reanalyse_timing.py [--out profiles/reanalyse_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "muzero-go_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

STEP_LIMIT_S = {"epoch": 180, "reanalyse": 180, "search": 180}


def _net(N):
    import torch

    import mzgo
    net = mzgo.MuZeroNet(96, N * N + 1).to("cuda:0").eval()
    net.load_state_dict(mzgo.deterministic_state_dict(96, N * N + 1, 0))
    torch.cuda.synchronize()
    return net


def _selfplay(args):
    import mzgo
    return mzgo.SelfPlay(_net(args.board_size), args.games, args.simulations, seed=args.seed)


def _timed(fn, repeats):
    """ms of each of ``repeats`` runs of fn() after one warm-up (HIP events)."""
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def step_epoch(args):
    import numpy as np

    from mzgo.reanalyse import record_ids
    sp = _selfplay(args)
    eng = sp.engine
    sp.reset()
    sp.move(sp.max_moves)                       # warm-up epoch (weights upload, first launches)
    eng.counters()
    boards, queue = [], []
    for k in range(args.repeats):
        eng.launch_timing(True)
        sp.reset(epoch=1 + k)
        sp.move(sp.max_moves)
        assert eng.counters()["playing"] == 0
        b, q = eng.launch_timing(False)
        assert len(b) == 1, "the epoch did not run as one move-parallel launch pair"
        boards.append(b[0])
        queue.append(q[0])
    recs = [eng.record(g) for g in range(args.games)]
    lens = [int(r["length"]) for r in recs]
    ids = np.concatenate([record_ids(0, g, args.repeats, np.arange(L)) for g, L in enumerate(lens)])
    np.savez(os.path.join(args.work, "positions.npz"), stones=np.concatenate([r["stones"] for r in recs]),
             invd=np.concatenate([r["invd"] for r in recs]), flags=np.concatenate([r["flags"] for r in recs]),
             ids=ids, value=np.concatenate([r["value"] for r in recs]))
    return dict(positions=int(sum(lens)), boards_ms=boards, queue_ms=queue)


def step_reanalyse(args):
    import numpy as np
    import torch

    from mzgo.reanalyse import latest_first
    z = np.load(os.path.join(args.work, "positions.npz"))
    eng = _selfplay(args).engine                # the epoch's engine shape: a tree slot per game (256 = the CU count)
    dev = eng.device
    t = [torch.from_numpy(z[k]).to(dev) for k in ("stones", "invd", "flags", "ids")]
    out = {}

    def run(items=t, want_policy=True):
        out["r"] = eng.reanalyse(*items, want_policy=want_policy)
    ms = _timed(run, args.repeats)
    value = out["r"][1].cpu().numpy()
    # where a gap to the epoch's queue comes from: the policy rows (one wave per
    # item), and the item order -- the records' (game after game) against
    # latest moves first (mzgo.reanalyse.latest_first, what SelfPlay.reanalyse
    # and Reanalyser.run queue; k_search_queue's order up to the games' lengths)
    ms_nopol = _timed(lambda: run(want_policy=False), args.repeats)
    ids = z["ids"]
    order = torch.from_numpy(latest_first(ids)).to(dev)
    tq = [x[order] for x in t]
    ms_latest = _timed(lambda: run(items=tq), args.repeats)
    # one search per slot, every game's position at move m: the launch lasts as long as its slowest search
    wave = {}
    for m in range(0, int(ids[:, 1].max()) + 1, 10):
        sel = torch.from_numpy(np.flatnonzero(ids[:, 1] == m)).to(dev)
        tm = [x[sel] for x in t]
        wave[str(m)] = dict(positions=int(len(sel)), ms=round(min(_timed(lambda: run(items=tm), args.repeats)), 4))
    return dict(positions=int(len(value)), ms=ms, ms_without_policy=ms_nopol, ms_latest_first=ms_latest, slots=eng.G,
                one_search_per_slot_at_move=wave,
                values_equal_records=bool(value.tobytes() == z["value"].tobytes()))


def step_search(args):
    import numpy as np
    import torch

    from mzgo.trainer import _planes
    z = np.load(os.path.join(args.work, "positions.npz"))
    N = args.board_size
    eng = _selfplay(args).engine
    obs = np.stack([_planes(z["stones"][i], z["invd"][i], int(z["flags"][i]), N) for i in range(len(z["flags"]))])
    obs = torch.from_numpy(obs).to(eng.device, torch.float32)
    G = args.games

    def run():
        for at in range(0, obs.shape[0], G):
            eng.search(obs[at:at + G], move_index=at // G)
    ms = _timed(run, args.repeats)
    return dict(positions=int(obs.shape[0]), ms=ms, launches=-(-obs.shape[0] // G))


STEPS = {"epoch": step_epoch, "reanalyse": step_reanalyse, "search": step_search}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reanalyse_timing.json"))
    ap.add_argument("--board-size", type=int, default=9)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--simulations", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="(internal) run one step in this process")
    ap.add_argument("--work", default=None, help="(internal) the steps' shared directory")
    args = ap.parse_args()
    if args.step:
        res = STEPS[args.step](args)
        with open(os.path.join(args.work, args.step + ".json"), "w") as f:
            json.dump(res, f)
        return 0

    res = {}
    with tempfile.TemporaryDirectory() as work:
        for step in ("epoch", "reanalyse", "search"):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--work", work,
                   "--board-size", str(args.board_size), "--games", str(args.games),
                   "--simulations", str(args.simulations), "--seed", str(args.seed), "--repeats", str(args.repeats)]
            try:
                rc = subprocess.run(cmd, timeout=STEP_LIMIT_S[step]).returncode
            except subprocess.TimeoutExpired:
                print(f"step {step}: no result within {STEP_LIMIT_S[step]} s; stopping", file=sys.stderr)
                return 124
            if rc != 0:
                print(f"step {step} failed (exit {rc}); stopping", file=sys.stderr)
                return rc
            with open(os.path.join(work, step + ".json")) as f:
                res[step] = json.load(f)

    S = args.simulations

    def rate(n, ms):
        best = min(ms)
        return dict(ms=[round(x, 3) for x in ms], best_ms=round(best, 3), positions_per_s=round(n / best * 1e3, 1),
                    simulations_per_s=round(n * S / best * 1e3, 1))
    n = res["epoch"]["positions"]
    out = dict(board_size=args.board_size, games=args.games, simulations=S, positions=n,
               reanalyse_slots=res["reanalyse"]["slots"],
               epoch_search_queue=rate(n, res["epoch"]["queue_ms"]),
               epoch_boards_ms=[round(x, 3) for x in res["epoch"]["boards_ms"]],
               reanalyse=rate(n, res["reanalyse"]["ms"]),
               reanalyse_without_policy=rate(n, res["reanalyse"]["ms_without_policy"]),
               reanalyse_latest_first=rate(n, res["reanalyse"]["ms_latest_first"]),
               reanalyse_one_search_per_slot_at_move=res["reanalyse"]["one_search_per_slot_at_move"],
               reanalyse_values_equal_records=res["reanalyse"]["values_equal_records"],
               search_256_at_a_time=dict(rate(n, res["search"]["ms"]), launches=res["search"]["launches"]))
    out["reanalyse_over_queue_rate"] = round(out["reanalyse"]["positions_per_s"] /
                                             out["epoch_search_queue"]["positions_per_s"], 4)
    out["reanalyse_over_search_rate"] = round(out["reanalyse"]["positions_per_s"] /
                                              out["search_256_at_a_time"]["positions_per_s"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
