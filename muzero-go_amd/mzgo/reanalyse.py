"""Reanalysis (MuZero Reanalyse): search stored positions again under the
current weights and return fresh training targets.

The reference has no counterpart: its trainer (main.py:381-522) only ever
trains on the policies recorded when a game was played.  Here any list of n
stored positions runs through one device work queue (``Engine.reanalyse``,
``k_reanalyse_queue``: a persistent workgroup per tree slot claims positions
until none is left) and comes back as root child visit counts, root values and
visit-count policy targets.

* ``positions_from_planes`` / ``record_ids`` -- observations and RNG keys in
  the engine's record format (``observation_planes``: a record back to its
  observation); ``latest_first`` -- the order to queue them in;
* ``SelfPlay.reanalyse()`` (mzgo.selfplay) -- every recorded move of the
  current games, with the records' own keys;
* ``Reanalyser`` -- main.py-format trajectories in, trajectories with fresh
  ``policies`` (and ``root_values``) out.
"""
import numpy as np
import torch

from .engine import Engine, EngineConfig


# record flags bit 3: the move was searched with the fast budget of playout cap
# randomization (csrc/mzgo_move.hpp kFlagFast); bits 0-2 are the board's
FLAG_FAST = 8


def positions_from_planes(obs):
    """GoEnv observations [n, 6, N, N] (black, white, turn, invalid, passed,
    done) -> (stones int8 [n, N*N]: 0 / 1 black / 2 white, invd uint8
    [n, N*N], flags uint8 [n]: bit0 turn, bit1 passed, bit2 done): the
    engine's record format, the inverse of ``observation_planes``.  Takes a
    tensor, an array or a sequence of [6, N, N] arrays; returns torch tensors
    on the input's device (the CPU unless ``obs`` is a CUDA tensor)."""
    if not isinstance(obs, torch.Tensor):
        obs = torch.from_numpy(np.array(obs))           # (a copy: read-only arrays too)
    if obs.dim() != 4 or obs.shape[1] != 6 or obs.shape[2] != obs.shape[3]:
        raise ValueError(f"observations must be [n, 6, N, N], got {tuple(obs.shape)}")
    n = obs.shape[0]
    on = obs > 0
    stones = (on[:, 0].to(torch.int8) + 2 * on[:, 1].to(torch.int8)).reshape(n, -1)
    invd = on[:, 3].to(torch.uint8).reshape(n, -1)
    bit = [on[:, c].reshape(n, -1).any(dim=1).to(torch.uint8) for c in (2, 4, 5)]
    flags = bit[0] | (bit[1] << 1) | (bit[2] << 2)
    return stones.contiguous(), invd.contiguous(), flags.contiguous()


def observation_planes(stones, invd, flags, N):
    """One stored position (stones [N*N]: 0 / 1 black / 2 white, invd [N*N],
    flags: bit0 turn, bit1 passed, bit2 done) -> its GoEnv observation, float64
    [6, N, N]: the inverse of ``positions_from_planes`` and the host form of
    the store's plane rule (csrc/mzgo_replay.hpp ``observation_plane``)."""
    flags = int(flags)
    o = np.zeros((6, N, N))
    s = np.asarray(stones).reshape(N, N)
    o[0] = s == 1
    o[1] = s == 2
    o[2] = flags & 1
    o[3] = np.asarray(invd).reshape(N, N)
    o[4] = (flags >> 1) & 1
    o[5] = (flags >> 2) & 1
    return o


def record_ids(game_base, g, epoch, moves):
    """The search keys of self-play records: int32 [n, 2] rows (key game id,
    move index), the key game id being ``(game_base + g) ^ (epoch << 24)`` as
    a 32-bit word -- the id the engine derives a move's RNG streams from
    (csrc/mzgo_move.hpp ``move_key``).  ``g`` and ``moves`` broadcast."""
    g, moves = np.broadcast_arrays(np.asarray(g, np.int64).reshape(-1), np.asarray(moves, np.int64).reshape(-1))
    gid = ((int(game_base) + g) & 0xFFFFFFFF) ^ ((int(epoch) << 24) & 0xFFFFFFFF)
    return np.stack([gid.astype(np.uint32).view(np.int32), moves.astype(np.int32)], axis=1)


def latest_first(ids):
    """The order to hand positions to the queue in: a stable sort by falling
    move index.  The queue claims items in index order, and searches of
    late-game positions take several times longer than opening ones (DESIGN.md
    section 4, "Reanalysis"), so this is longest-first, as k_search_queue
    orders an epoch's moves; in the records' own order the launch ends with a
    few long searches on otherwise idle CUs."""
    return np.argsort(-np.asarray(ids).reshape(-1, 2)[:, 1].astype(np.int64), kind="stable")


class Reanalyser:
    """Fresh policy targets for main.py-format trajectories.

    ``Reanalyser(net, num_simulations, slots=None, **search options)`` owns an
    engine with ``num_games = slots`` tree slots -- the CU count of ``net``'s
    device when None, so that every CU runs a search -- created at the first
    search.  The search options are ``EngineConfig`` fields; the defaults are
    main.py's (``MainSelfPlay``'s: its MCTS variant, c_puct 2, Dirichlet(0.03)
    at 0.25, pass prior 0.05), under which a trajectory's policy target is
    counts / sum over the legal actions."""

    DEFAULTS = dict(compat="fixed", search_variant="main", c_puct=2.0, dirichlet_alpha=0.03,
                    dirichlet_epsilon=0.25, pass_epsilon=0.05)

    def __init__(self, net, num_simulations, *, slots=None, **options):
        self.net = net
        self.N = net.board_size
        self.S = num_simulations
        self.slots = slots
        self.options = {**self.DEFAULTS, **options}
        self._engine = None

    @property
    def engine(self):
        if self._engine is None:
            dev = next(self.net.parameters()).device
            if dev.type != "cuda":
                raise RuntimeError("Reanalyser searches on the GPU only: move the net with .to('cuda') first")
            slots = self.slots or torch.cuda.get_device_properties(dev).multi_processor_count
            self._engine = Engine(EngineConfig(board_size=self.N, latent_dim=self.net.latent_dim, num_games=slots,
                                               num_simulations=self.S, device=dev.index or 0, **self.options))
            self._load()
        return self._engine

    def _load(self):
        """The net's weights into the engine: on the device (a copy from one of
        the net's engines that has them, else one pack launch) when the net's
        ``device_weights`` is set, through the host otherwise."""
        if getattr(self.net, "device_weights", False):
            from .net import refresh_engine_device
            refresh_engine_device(self.net, self._engine, self.net._version())
        else:
            self._engine.set_state_dict(self.net.state_dict())

    def refresh(self, net=None):
        """Reload the weights (of ``net``, or of the net given before)."""
        if net is not None:
            if (net.board_size, net.latent_dim) != (self.N, self.net.latent_dim):
                raise ValueError("refresh: the net's board size / latent_dim differ from the reanalyser's")
            self.net = net
        if self._engine is not None:
            self._load()

    def run(self, trajectories, ids=None):
        """Search the first T = len(actions) observations of every trajectory
        and return new trajectories (shallow copies) whose ``policies`` are the
        fresh targets, with the searches' root values as ``root_values``.

        ``ids``: per trajectory an int array [T, 2] of search keys
        (``record_ids``); by default trajectory k's move t is keyed (k, t)."""
        N = self.N
        obs, lens = [], []
        for k, tr in enumerate(trajectories):
            T = len(tr["actions"])
            o = np.asarray(tr["observations"][:T], dtype=np.float64)
            if T and o.shape[1:] != (6, N, N):
                raise ValueError(f"trajectory {k}: observations are {o.shape[1:]}, the net plays {N}x{N} "
                                 f"(expected (6, {N}, {N}))")
            obs.append(o.reshape(T, 6, N, N))
            lens.append(T)
        if ids is None:
            ids = [record_ids(0, k, 0, np.arange(T)) for k, T in enumerate(lens)]
        ids = [np.asarray(i, np.int32).reshape(-1, 2) for i in ids]
        if [len(i) for i in ids] != lens:
            raise ValueError("ids must hold one (key game id, move index) row per searched observation")
        # (every move is searched with the full budget here: no row stays a fast search's)
        out = [{k: v for k, v in tr.items() if k != "fast_search"} for tr in trajectories]
        if sum(lens) == 0:
            for tr in out:
                tr["policies"], tr["root_values"] = [], []
            return out
        ids = np.concatenate(ids)
        order = latest_first(ids)
        stones, invd, flags = positions_from_planes(np.concatenate(obs)[order])
        _, v, p = self.engine.reanalyse(stones, invd, flags, ids[order])
        value, policy = np.empty(len(ids)), np.empty((len(ids), self.N * self.N + 1))
        value[order], policy[order] = v.cpu().numpy(), p.cpu().numpy()
        at = 0
        for tr, T in zip(out, lens):
            tr["policies"] = [policy[at + t].copy() for t in range(T)]
            tr["root_values"] = [float(v) for v in value[at:at + T]]
            at += T
        return out
