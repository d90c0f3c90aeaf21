"""Device replay store: finished games stay in HBM, from the self-play
records to the trainer's batch.

The reference keeps trajectories in Python lists (main.py:158-184,
``PrioritizedReplayBuffer``) and builds every training target in a Python
loop (main.py:381-522).  ``DeviceReplay`` keeps the same games in a FIFO ring
of slots on the GPU, in the self-play record format (stones i8, invd u8,
flags u8: 2 N^2 + 1 bytes per position against 48 N^2 for the f64 planes),
and serves both consumers of stored games from there:

* ``batch``     -- one launch (k_replay_batch) writes the trainer's targets for
  B (game, start, symmetry) samples (``items`` checks and uploads them once,
  ``batch_from`` and the other ``*_from`` assemblies take the device items);
  ``finish_values`` adds the bootstrap;
  ``batch_values`` -- the same with search-value targets: n-step returns
  bootstrapped from the stored root values, no bootstrap inference
  (``TrainConfig.value_target="search"``; ``value_targets_host`` is the rule);
* ``reanalyse`` -- the stored positions searched again under a ``Reanalyser``'s
  engine, the fresh policies and root values written into the store;
  ``reanalyse_sample`` -- the same for exactly the rows a drawn sample is about
  to read, from the sampler's device items (``sample`` -> ``reanalyse_sample``
  -> ``batch_from``; ``TrainConfig.reanalyse_sample``);
* ``ownership`` / ``ownership_from`` -- one more small launch on the same
  samples (k_replay_ownership): who owns each point of the game's final board,
  seen by the colour to move at every unroll step, the targets of the ownership
  head (``TrainConfig.ownership_loss_weight``; ``ownership_host`` and
  ``ownership_targets_host`` are the rules).

Ingest is ``add_games(engine)`` (device to device, one launch; what
``MainSelfPlay.play_into`` calls), the playing launch itself
(``SelfPlay.play_games_into``: continuous self-play, any number of games), or ``add(trajectory)`` for main.py-format
dicts from files and tests; ``export(i)`` gives a game back as such a dict.

Only the ledger crosses the bus: each game's length, key id and priority live
on the host (``ReplayLedger``), and sampling is main.py's --
``sample_indices`` draws exactly what ``PrioritizedReplayBuffer.sample`` draws
from the same ``np.random`` state.  One store equals
``MultiVersionReplayBuffer(num_versions=1)``.

Opt-in, the store also keeps a second, device-resident ledger -- a weight and
a generation per slot -- with a sampler on the GPU (``sample_batch``,
``update_device_priorities``, ``device_priorities``,
``set_device_priorities``; ``TrainConfig.device_sampling``): successive
sampling without replacement from a 64-ary sum tree, with a priority exponent
and importance weights, nothing on the host but the count of games.  The two
ledgers are independent: neither reads or writes the other.

Opt-in on top of the device ledger, position-level prioritized replay
(MuZero, App. G; ``enable_position_priorities``, ``sample_positions`` /
``sample_positions_batch`` / ``sample_positions_batch_values``,
``update_position_priorities``, ``position_priorities``;
``TrainConfig.position_priorities``): a weight per stored position, one draw
picking (game, start) with probability proportional to it, importance weights
over positions, and the sampled windows' weights rewritten from the step's
|value - target|.  ``sample_positions_host`` and ``position_priorities_host``
are the rules without a GPU.
"""
import ctypes

import numpy as np
import torch

from ._lib import check, lib, ptr, stream_of
from .reanalyse import FLAG_FAST, observation_planes, positions_from_planes


def symmetry_tables(board_size, symmetry):
    """The index maps the batch kernel applies for symmetry s = 0..7 on an
    N x N board (mzgo_replay_symmetry_table: the kernel's own functions run on
    the host): ``src`` int32 [N*N] -- output cell c shows input cell src[c],
    i.e. ``y.flat = x.flat[src]`` for ``y = np.rot90(x, s & 3)``, then
    ``np.flip(y, -1)`` if ``s & 4`` -- and ``dst`` int32 [N*N + 1] -- action a
    becomes dst[a]; the pass action stays."""
    cells = board_size * board_size
    src = np.empty(cells, np.int32)
    dst = np.empty(cells + 1, np.int32)
    check(lib.mzgo_replay_symmetry_table(int(board_size), int(symmetry), ptr(src), ptr(dst)))
    return src, dst


def queue_key_gids(n_games, num_games, game_base=0, epoch=0):
    """Key ids int32 [n_games] of the games one ``play_games_into(n_games)``
    call stores, in the store's order: queue game j is slot j % num_games of
    epoch ``epoch`` + j // num_games, so its id is (game_base + j % num_games)
    ^ ((epoch + j // num_games) << 24) -- ``mzgo.reanalyse.record_ids``' first
    column for that slot and epoch."""
    j = np.arange(int(n_games), dtype=np.int64)
    G = int(num_games)
    gid = ((int(game_base) + j % G) & 0xFFFFFFFF) ^ (((int(epoch) + j // G) << 24) & 0xFFFFFFFF)
    return gid.astype(np.uint32).view(np.int32)


class ReplayLedger:
    """The host's side of the store: per game its priority, length and key
    id, in logical (oldest first) order, with ``PrioritizedReplayBuffer``'s
    semantics (main.py:158-184): FIFO eviction at ``capacity``, priority 1.0
    for a new game, the same ``np.random.choice`` call."""

    def __init__(self, capacity):
        self.capacity = capacity
        self.priorities = []
        self.lengths = []
        self.key_gids = []

    def __len__(self):
        return len(self.priorities)

    def push(self, length, key_gid):
        if len(self.priorities) >= self.capacity:
            self.priorities.pop(0)
            self.lengths.pop(0)
            self.key_gids.pop(0)
        self.priorities.append(1.0)
        self.lengths.append(int(length))
        self.key_gids.append(int(key_gid))

    def sample_indices(self, batch_size):
        priorities = np.array(self.priorities)
        probs = priorities / priorities.sum()
        return np.random.choice(len(self.priorities), batch_size, replace=False, p=probs)

    def update_priorities(self, indices, new_priorities):
        for i, p in zip(indices, new_priorities):
            self.priorities[i] = p


def finish_values(val, factor, has_boot, value):
    """The value targets from ``batch``'s parts and the network's values of
    its ``boot_obs`` rows (float32, B*(K+1) of them): float32 [B, K+1],
    ``(float)(val + factor * (double)v)`` where a bootstrap position exists,
    ``(float)val`` elsewhere -- the bits of the host path's float64 sum
    (k_replay_finish)."""
    n = val.numel()
    value = value.to(val.device, torch.float32).reshape(n).contiguous()
    t_val = torch.empty(val.shape, dtype=torch.float32, device=val.device)
    check(lib.mzgo_replay_finish_values(ptr(val), ptr(factor), ptr(has_boot), ptr(value), n, ptr(t_val),
                                        stream_of(val.device)))
    return t_val


def _draw_args(seed, step, symmetries, beta):
    """A draw's (seed, step, symmetries, beta) as the library takes them."""
    return int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF, int(bool(symmetries)), float(beta)


def _sample_twin(fn, weights, length, dims, head, batch_size, draw):
    """Both sampler twins' call: ``fn(weights, length, *dims, head, B, *draw,
    items, index, weight)`` into fresh numpy buffers."""
    B = int(batch_size)
    items = np.empty((max(B, 0), 3), np.int32)
    index = np.empty(max(B, 0), np.int32)
    weight = np.empty(max(B, 0), np.float32)
    check(fn(ptr(weights), ptr(length), *dims, int(head), B, *draw, ptr(items), ptr(index), ptr(weight)))
    return dict(items=items, index=index, weight=weight)


def sample_host(prio, length, head, batch_size, *, seed, step, symmetries=False, beta=0.0):
    """The device sampler's host twin (mzgo_replay_sample_host: the kernels'
    own scan, descent and fallback functions run serially; no GPU).  ``prio``
    f64 and ``length`` i32 are per ring SLOT (``len(prio)`` = the capacity),
    ``head`` is the slot of logical game 0.  Returns a dict of numpy arrays:
    ``items`` i32 [B,3] (slot, start, symmetry), ``index`` i32 [B] and
    ``weight`` f32 [B]."""
    prio = np.ascontiguousarray(np.asarray(prio, dtype=np.float64).reshape(-1))
    length = np.ascontiguousarray(np.asarray(length, dtype=np.int32).reshape(-1))
    if len(prio) != len(length):
        raise ValueError("sample_host: prio and length have one entry per slot")
    return _sample_twin(lib.mzgo_replay_sample_host, prio, length, (len(prio),), head, batch_size,
                        _draw_args(seed, step, symmetries, beta))


def sample_positions_host(pprio, length, head, batch_size, *, seed, step, symmetries=False, beta=0.0):
    """The position sampler's host twin (mzgo_replay_sample_positions_host: the
    kernels' own scan, descent and fallback functions run serially; no GPU).
    ``pprio`` f64 [cap, M] (position weights, rows t >= length unread) and
    ``length`` i32 [cap] are per ring SLOT, ``head`` is the slot of logical
    game 0.  Returns ``sample_host``'s dict; ``items[:, 1]`` is the drawn
    position."""
    pprio = np.ascontiguousarray(np.asarray(pprio, dtype=np.float64))
    length = np.ascontiguousarray(np.asarray(length, dtype=np.int32).reshape(-1))
    if pprio.ndim != 2 or len(pprio) != len(length):
        raise ValueError("sample_positions_host: pprio is [cap, M] and length has one entry per slot")
    return _sample_twin(lib.mzgo_replay_sample_positions_host, pprio, length, pprio.shape, head, batch_size,
                        _draw_args(seed, step, symmetries, beta))


def position_priorities_host(rewards, root_values, td_steps, discount, alpha=1.0, floor=None):
    """The weights a new game's positions get under ``init="td"``
    (mzgo_replay_position_priorities_host: the fill kernel's own rule, no GPU):
    f64 [L], entry t = ``max(|root_values[t] - target_t|, floor) ** alpha`` with
    target_t the search-value target of index t (``value_targets_host``'s
    float32, widened) and ``floor`` = float32's smallest normal by default."""
    r = np.ascontiguousarray(np.asarray(rewards, dtype=np.float64).reshape(-1))
    rv = np.ascontiguousarray(np.asarray(root_values, dtype=np.float64).reshape(-1))
    if len(r) != len(rv) + 1:
        raise ValueError(f"position_priorities_host: a game of L moves has L + 1 rewards and L root values, got "
                         f"{len(r)} and {len(rv)}")
    out = np.empty(len(rv), np.float64)
    check(lib.mzgo_replay_position_priorities_host(ptr(r), ptr(rv) if len(rv) else None, len(rv), int(td_steps),
                                                   float(discount), float(alpha), 0.0 if floor is None else float(floor),
                                                   ptr(out) if len(rv) else None))
    return out


def window_items_host(length, items, unroll_steps, td_steps=None):
    """The item list of a batch's windows on the host (mzgo_replay_window_items_host:
    the builder kernel's own rule, no GPU).  ``length`` i32 per ring SLOT,
    ``items`` i32 [B,3] (slot, start, symmetry).  Sample b reads the stored
    policy rows t = start .. min(start + K, L - 1) of its slot; a triple whose
    slot is outside the store, whose game is empty or whose start is outside
    0 .. L - 1 contributes nothing.  Returns i32 [n,2] rows (slot, t) by
    falling t, equal t by batch position.  With ``td_steps`` (search-value
    targets, mzgo_replay_window_items_values_host) a sample's rows are its
    window together with its value rows t = start + td_steps ..
    min(start + K + td_steps, L - 1), each row once per sample."""
    length = np.ascontiguousarray(np.asarray(length, dtype=np.int32).reshape(-1))
    items = np.ascontiguousarray(np.asarray(items, dtype=np.int32).reshape(-1, 3))
    B, K = len(items), int(unroll_steps)
    out = np.empty((max(B, 0) * (max(K, 0) + 1) * (1 if td_steps is None else 2), 2), np.int32)
    n = ctypes.c_int32()
    if td_steps is None:
        check(lib.mzgo_replay_window_items_host(ptr(length), len(length), ptr(items), B, K, ptr(out), ctypes.byref(n)))
    else:
        check(lib.mzgo_replay_window_items_values_host(ptr(length), len(length), ptr(items), B, K, int(td_steps),
                                                       ptr(out), ctypes.byref(n)))
    return out[:n.value].copy()


def value_targets_host(rewards, root_values, start, unroll_steps, td_steps, discount):
    """The search-value targets of one sample on the host
    (mzgo_replay_value_targets_host: the batch kernel's own rule, no GPU).
    ``rewards`` f64 [L + 1] (the winner last) and ``root_values`` f64 [L] of a
    game of L moves; returns float32 [K + 1], entry k the target of trajectory
    index i = ``start`` + k with step horizon n = ``td_steps``: the discounted
    rewards r[i] .. r[i + n - 1] (stopping after r[L]) plus discount^n times
    the stored root value of position i + n where one was searched (i + n <=
    L - 1), or times r[L] at i + n = L -- the final board has no search, r[L]
    is what is left of its return -- in f64, one multiply and one add per term."""
    r = np.ascontiguousarray(np.asarray(rewards, dtype=np.float64).reshape(-1))
    rv = np.ascontiguousarray(np.asarray(root_values, dtype=np.float64).reshape(-1))
    if len(r) != len(rv) + 1:
        raise ValueError(f"value_targets_host: a game of L moves has L + 1 rewards and L root values, got {len(r)} "
                         f"and {len(rv)}")
    out = np.empty(max(int(unroll_steps), 0) + 1, np.float32)
    check(lib.mzgo_replay_value_targets_host(ptr(r), ptr(rv) if len(rv) else None, len(rv), int(start),
                                             int(unroll_steps), int(td_steps), float(discount), ptr(out)))
    return out


def ownership_host(stones, board_size):
    """Who owns each point of a board (mzgo_ownership_host: the ownership
    kernel's own fixed-point rule, no GPU).  ``stones`` [N, N] or [N*N] (1 =
    black, 2 = white, 0 = empty); returns int8 [N, N]: a stone's colour, for an
    empty point the one colour its empty region touches, 0 where the region
    touches both colours or none -- ``oracle.gogame.areas`` cell by cell."""
    N = int(board_size)
    s = np.ascontiguousarray(np.asarray(stones, dtype=np.int8).reshape(-1))
    if len(s) != N * N:
        raise ValueError(f"ownership_host: stones has {len(s)} cells, a {N}x{N} board {N * N}")
    owner = np.empty(N * N, np.int8)
    check(lib.mzgo_ownership_host(ptr(s), N, ptr(owner)))
    return owner.reshape(N, N)


def ownership_targets_host(final_stones, flags, board_size, start, unroll_steps, symmetry=0):
    """The ownership targets of one sample on the host
    (mzgo_ownership_targets_host: the kernel's own rule, no GPU).
    ``final_stones`` [N*N] is the board after the last move of a game of L
    moves (the store's row L) and ``flags`` u8 [L + 1] its positions' flag
    bytes (bit 0: white to move; bit 2 of the last: the game ended).  Returns
    ``(t_own f32 [K+1, N*N], own_mask f32 [K+1])``: row k is position
    ``start`` + k seen by its colour to move -- +1 the mover owns cell
    ``src[c]`` of ``symmetry``'s table, -1 the opponent does, 0 nobody -- with
    mask 1, or zeros with mask 0 past the final board or when the game did not
    end."""
    N = int(board_size)
    s = np.ascontiguousarray(np.asarray(final_stones, dtype=np.int8).reshape(-1))
    fl = np.ascontiguousarray(np.asarray(flags, dtype=np.uint8).reshape(-1))
    if len(s) != N * N or len(fl) < 1:
        raise ValueError(f"ownership_targets_host: final_stones has {len(s)} cells for a {N}x{N} board, flags "
                         f"{len(fl)} entries (L + 1 >= 1)")
    K1 = max(int(unroll_steps), 0) + 1
    t_own = np.empty((K1, N * N), np.float32)
    mask = np.empty(K1, np.float32)
    check(lib.mzgo_ownership_targets_host(ptr(s), ptr(fl), len(fl) - 1, N, int(start), int(symmetry),
                                          int(unroll_steps), ptr(t_own), ptr(mask)))
    return t_own, mask


class DeviceReplay:
    """``DeviceReplay(board_size, capacity, max_moves, device)``: a ring of
    ``capacity`` games of at most ``max_moves`` moves on ``device``.
    ``max_moves`` must be the move cap of the engines that feed it
    (``MainSelfPlay.max_moves``)."""

    def __init__(self, board_size, capacity, max_moves, device="cuda"):
        self.N = int(board_size)
        self.A = self.N * self.N + 1
        self.capacity = int(capacity)
        self.max_moves = int(max_moves)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceReplay lives on the GPU; use PrioritizedReplayBuffer for host trajectories")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        torch.cuda.init()
        h = ctypes.c_void_p()
        check(lib.mzgo_replay_create(self.N, self.capacity, self.max_moves, self.device.index, ctypes.byref(h)))
        self._h = h
        self.ledger = ReplayLedger(self.capacity)

    def close(self):
        if getattr(self, "_h", None):
            lib.mzgo_replay_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return len(self.ledger)

    # ---- the ledger (PrioritizedReplayBuffer's interface) ----
    @property
    def priorities(self):
        return self.ledger.priorities

    @property
    def lengths(self):
        return self.ledger.lengths

    @property
    def key_gids(self):
        return self.ledger.key_gids

    def sample_indices(self, batch_size):
        return self.ledger.sample_indices(batch_size)

    def update_priorities(self, indices, new_priorities):
        self.ledger.update_priorities(indices, new_priorities)

    def _info(self):
        size = ctypes.c_int32()
        lengths = np.zeros(self.capacity, np.int32)
        gids = np.zeros(self.capacity, np.int32)
        check(lib.mzgo_replay_info(self._h, ctypes.byref(size), None, ptr(lengths), ptr(gids)))
        return lengths[:size.value], gids[:size.value]

    def _slot_order(self):
        """What the host twins take per ring SLOT: the slots of the games held
        (logical order), the ``length`` array i32 [capacity] (empty slots 0)
        and the head."""
        size, head = ctypes.c_int32(), ctypes.c_int32()
        check(lib.mzgo_replay_info(self._h, ctypes.byref(size), ctypes.byref(head), None, None))
        slots = (head.value + np.arange(size.value)) % self.capacity
        length = np.zeros(self.capacity, np.int32)
        length[slots] = self._info()[0]
        return slots, length, head.value

    def _pushed(self, n):
        """Enter the last n games the store took into the ledger."""
        lengths, gids = self._info()
        for _ in range(max(0, n - len(lengths))):         # (more games than the capacity: evicted unseen)
            self.ledger.push(0, 0)
        for L, g in zip(lengths[-n:], gids[-n:]):
            self.ledger.push(L, g)
        assert self.ledger.lengths == [int(x) for x in lengths]

    # ---- ingest ----
    def add_games(self, engine):
        """Every finished game of ``engine``'s slots, device to device in one
        launch (mzgo_replay_add_games), as G adds in slot order; only the G
        lengths come back.  Refuses while a game is still playing."""
        if engine.counters()["playing"] != 0:
            raise RuntimeError("add_games: games are still playing on the engine")
        check(lib.mzgo_replay_add_games(self._h, engine.handle, stream_of(self.device)))
        self._pushed(engine.G)

    def add(self, trajectory, key_gid=None):
        """One main.py-format trajectory (observations T+2, actions T, policies
        T, rewards T+1; ``root_values`` T optional; ``fast_search`` T optional:
        the moves searched with the fast budget, whose policy rows every batch
        masks to zero until a reanalysis rewrites them) from the host.  ``key_gid``:
        the game's search key id for ``reanalyse`` (default: a running count
        of the games added this way)."""
        T = len(trajectory["actions"])
        if T > self.max_moves:
            raise ValueError(f"trajectory of {T} moves, the store holds at most {self.max_moves}")
        obs = np.asarray(trajectory["observations"][:T + 1], dtype=np.float64)
        if obs.shape != (T + 1, 6, self.N, self.N):
            raise ValueError(f"observations are {obs.shape[1:]} x {obs.shape[0]}, expected at least {T + 1} of "
                             f"(6, {self.N}, {self.N})")
        if len(trajectory["rewards"]) != T + 1 or len(trajectory["policies"]) != T:
            raise ValueError("a trajectory has T actions, T policies and T + 1 rewards")
        stones, invd, flags = (np.ascontiguousarray(t.numpy()) for t in positions_from_planes(obs))
        fast = trajectory.get("fast_search")
        if fast is not None:
            fast = np.asarray(fast, dtype=bool).reshape(-1)
            if fast.shape[0] != T:
                raise ValueError(f"fast_search has {fast.shape[0]} entries for {T} moves")
            flags[:T] |= np.where(fast, FLAG_FAST, 0).astype(np.uint8)   # (never the final board's row T)
        action = np.ascontiguousarray(np.asarray(trajectory["actions"], dtype=np.int32))
        policy = np.ascontiguousarray(np.asarray(trajectory["policies"], dtype=np.float64).reshape(T, self.A))
        reward = np.ascontiguousarray(np.asarray(trajectory["rewards"], dtype=np.float64))
        rv = trajectory.get("root_values")
        rv = None if rv is None else np.ascontiguousarray(np.asarray(rv, dtype=np.float64).reshape(T))
        if key_gid is None:
            key_gid = self._host_adds = getattr(self, "_host_adds", -1) + 1
        key_gid = int(np.array(int(key_gid) & 0xFFFFFFFF, np.uint32).view(np.int32))
        check(lib.mzgo_replay_add(self._h, T, ptr(stones), ptr(invd), ptr(flags), ptr(action), ptr(policy),
                                  ptr(reward), ptr(rv), key_gid, stream_of(self.device)))
        self._pushed(1)

    def export(self, i):
        """Game i (0 = oldest) as a main.py-format dict: T+2 observations, T
        actions, T policies, T+1 rewards, plus ``root_values`` and ``key_gid``
        -- and ``fast_search`` (T bools) when at least one move's row is a
        fast-budget search that no reanalysis has rewritten."""
        M, C, A, N = self.max_moves, self.N * self.N, self.A, self.N
        length, gid = ctypes.c_int32(), ctypes.c_int32()
        stones = np.empty((M + 1, C), np.int8)
        invd = np.empty((M + 1, C), np.uint8)
        flags = np.empty(M + 1, np.uint8)
        action = np.empty(M, np.int32)
        policy = np.empty((M, A), np.float64)
        reward = np.empty(M + 1, np.float64)
        rv = np.empty(M, np.float64)
        i = int(i)
        check(lib.mzgo_replay_export(self._h, i + len(self) if i < 0 else i, ctypes.byref(length), ctypes.byref(gid),
                                     ptr(stones), ptr(invd), ptr(flags), ptr(action), ptr(policy), ptr(reward),
                                     ptr(rv), stream_of(self.device)))
        T = length.value
        obs = [observation_planes(stones[t], invd[t], flags[t], N) for t in range(T + 1)]
        out = {
            "observations": obs + [obs[-1].copy()],
            "actions": [int(a) for a in action[:T]],
            "rewards": [float(r) for r in reward[:T + 1]],
            "policies": [policy[t].copy() for t in range(T)],
            "root_values": [float(v) for v in rv[:T]],
            "key_gid": gid.value,
        }
        fast = [bool(int(f) & FLAG_FAST) for f in flags[:T]]
        if any(fast):
            out["fast_search"] = fast
        return out

    # ---- the trainer's batch ----
    def items(self, indices, starts, symmetries=None):
        """The device item list of B samples given on the host
        (mzgo_replay_items): sample b is game ``indices[b]`` (0 = oldest) from
        move ``starts[b]`` under symmetry ``symmetries[b]`` (0..7; None =
        identity), checked against the store's lengths.  Returns a CUDA i32
        tensor [B,3] of (slot, start, symmetry) rows, what ``sample`` returns as
        ``items``: one check and one upload for every ``*_from`` assembly of
        the same samples."""
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int32).reshape(-1))
        st = np.ascontiguousarray(np.asarray(starts, dtype=np.int32).reshape(-1))
        sy = None if symmetries is None else np.ascontiguousarray(np.asarray(symmetries, dtype=np.int32).reshape(-1))
        if len(st) != len(idx) or (sy is not None and len(sy) != len(idx)):
            raise ValueError("indices, starts and symmetries must have one entry per sample")
        items = torch.empty(len(idx), 3, dtype=torch.int32, device=self.device)
        check(lib.mzgo_replay_items(self._h, ptr(idx), ptr(st), ptr(sy), len(idx), ptr(items), stream_of(self.device)))
        return items

    def batch(self, indices, starts, unroll_steps, discount, symmetries=None):
        """The trainer's targets for B samples in one launch (``items``, then
        ``batch_from``): sample b is game ``indices[b]`` from move ``starts[b]``
        under symmetry ``symmetries[b]`` (0..7; None = identity).  Returns a
        dict of CUDA tensors: ``obs0`` f32 [B,6,N,N], ``boot_obs`` f32
        [B,K+1,6,N,N], ``acts`` i64 [B,K], ``t_rew`` f32 [B,K], ``t_pol`` f32
        [B,K+1,A], ``val`` / ``factor`` f64 [B,K+1] and ``has_boot`` u8 [B,K+1]
        (``finish_values`` turns the last three and the network's values of
        ``boot_obs`` into ``t_val``)."""
        return self.batch_from(self.items(indices, starts, symmetries), unroll_steps, discount)

    def _values_out(self, B, K):
        N, A, dev, K1 = self.N, self.A, self.device, max(K, 0) + 1
        return dict(obs0=torch.empty(B, 6, N, N, device=dev),
                    acts=torch.empty(B, max(K, 0), dtype=torch.int64, device=dev),
                    t_rew=torch.empty(B, max(K, 0), device=dev),
                    t_pol=torch.empty(B, K1, A, device=dev),
                    t_val=torch.empty(B, K1, device=dev))

    def batch_values(self, indices, starts, unroll_steps, td_steps, discount, symmetries=None):
        """``batch`` with search-value targets (``items``, then
        ``batch_values_from``: one launch, nothing to finish): ``obs0``,
        ``acts``, ``t_rew`` and ``t_pol`` as ``batch`` gives them, and ``t_val``
        f32 [B,K+1] -- the n-step returns (n = ``td_steps`` >= 1, independent of
        K) bootstrapped from the stored root values, ``value_targets_host``'s
        bits.  No ``boot_obs``, ``val``, ``factor`` or ``has_boot``."""
        return self.batch_values_from(self.items(indices, starts, symmetries), unroll_steps, td_steps, discount)

    # ---- ownership targets ----
    def ownership(self, indices, starts, unroll_steps, symmetries=None):
        """The ownership targets of B samples in one launch (``items``, then
        ``ownership_from``; ``batch``'s indices, starts and symmetries):
        ``(t_own f32 [B, K+1, N*N], own_mask f32 [B, K+1])`` on the device.
        Row (b, k) is the final board of sample b's game seen by the colour to
        move at position start + k under the sample's symmetry: +1 the mover
        owns the point, -1 the opponent, 0 nobody, with mask 1 -- or zeros with
        mask 0 past the final board and for a game that did not end (a game cut
        off by the move cap has no winner and no ownership).
        ``ownership_targets_host`` is the rule; the batch assembly is untouched."""
        return self.ownership_from(self.items(indices, starts, symmetries), unroll_steps)

    def ownership_from(self, sample, unroll_steps):
        """``ownership`` for a drawn ``sample`` (what ``sample`` / ``sample_batch``
        returned, or its ``items`` tensor), from the device items
        (mzgo_replay_ownership_items): nothing crosses the bus, nothing
        synchronises."""
        items = self._items_of(sample)
        B, K = items.shape[0], int(unroll_steps)
        t_own, mask = self._ownership_out(B, K)
        check(lib.mzgo_replay_ownership_items(self._h, ptr(items), B, K, ptr(t_own), ptr(mask),
                                              stream_of(self.device)))
        return t_own, mask

    def _ownership_out(self, B, K):
        K1 = max(K, 0) + 1
        return (torch.empty(B, K1, self.N * self.N, device=self.device), torch.empty(B, K1, device=self.device))

    # ---- the real boards of a window (the consistency loss's targets) ----
    def window_obs(self, indices, starts, unroll_steps, symmetries=None):
        """The real boards of B sampled windows in one launch (``items``, then
        ``window_obs_from``; ``batch``'s indices, starts and symmetries):
        ``(obs f32 [K, B, 6, N, N], mask f32 [B, K])`` on the device.
        ``obs[k-1, b]`` is the observation of position start + k of sample b's
        game under the sample's symmetry, k = 1..K -- the six planes ``batch``
        writes as ``obs0`` for that position -- step-major, so that
        ``obs.view(K * B, 6, N, N)`` goes to ``mzgo.encode`` without a copy and
        lines up with the unroll's ``latents[1:]``.  ``mask[b, k-1]`` is 1 where
        start + k <= the game's length (the final board counts); past it the
        planes are zeros and the mask 0.  At K = 0: empty tensors, no launch."""
        return self.window_obs_from(self.items(indices, starts, symmetries), unroll_steps)

    def window_obs_from(self, sample, unroll_steps):
        """``window_obs`` for a drawn ``sample`` (what ``sample`` / ``sample_batch``
        returned, or its ``items`` tensor), from the device items
        (mzgo_replay_window_obs_items): nothing crosses the bus, nothing
        synchronises."""
        items = self._items_of(sample)
        B, K = items.shape[0], int(unroll_steps)
        obs, mask = self._window_obs_out(B, K)
        if K > 0:
            check(lib.mzgo_replay_window_obs_items(self._h, ptr(items), B, K, ptr(obs), ptr(mask),
                                                   stream_of(self.device)))
        return obs, mask

    def _window_obs_out(self, B, K):
        K = max(K, 0)
        return (torch.empty(K, B, 6, self.N, self.N, device=self.device), torch.empty(B, K, device=self.device))

    # ---- the device ledger and sampler ----
    # Independent of ``ledger`` above: the host ledger (``priorities``,
    # ``sample_indices``, ``update_priorities``) is main.py's np.random path and
    # never reads or writes the device weights; the methods below never touch
    # the host ledger.  A trainer uses one or the other (TrainConfig.device_sampling).
    def _batch_out(self, B, K):
        N, A, dev, K1 = self.N, self.A, self.device, max(K, 0) + 1
        return dict(obs0=torch.empty(B, 6, N, N, device=dev),
                    boot_obs=torch.empty(B, K1, 6, N, N, device=dev),
                    acts=torch.empty(B, max(K, 0), dtype=torch.int64, device=dev),
                    t_rew=torch.empty(B, max(K, 0), device=dev),
                    t_pol=torch.empty(B, K1, A, device=dev),
                    val=torch.empty(B, K1, dtype=torch.float64, device=dev),
                    factor=torch.empty(B, K1, dtype=torch.float64, device=dev),
                    has_boot=torch.empty(B, K1, dtype=torch.uint8, device=dev))

    def _sample_out(self, B):
        dev = self.device
        return dict(items=torch.empty(max(B, 0), 3, dtype=torch.int32, device=dev),
                    index=torch.empty(max(B, 0), dtype=torch.int32, device=dev),
                    gen=torch.empty(max(B, 0), dtype=torch.int32, device=dev),      # (u32 bits)
                    weight=torch.empty(max(B, 0), device=dev))

    def sample(self, batch_size, *, seed, step, symmetries=False, beta=0.0):
        """The sampler alone (mzgo_replay_sample, two launches, nothing on the
        host): ``batch_size`` distinct games drawn by successive sampling
        without replacement from the device weights.  Returns CUDA tensors
        ``items`` i32 [B,3] (slot, start, symmetry), ``index`` i32 [B]
        (logical, oldest = 0), ``gen`` i32 [B] (the slots' generations, u32
        bits) and ``weight`` f32 [B] (importance weights, all 1 at beta 0)."""
        return self._sample(False, batch_size, _draw_args(seed, step, symmetries, beta))

    # the draw, and the draw followed by either assembly, for the game sampler and (``positions``) the position sampler
    def _sample(self, positions, batch_size, draw):
        B = int(batch_size)
        s = self._sample_out(B)
        fn = lib.mzgo_replay_sample_positions if positions else lib.mzgo_replay_sample
        check(fn(self._h, B, *draw, ptr(s["items"]), ptr(s["index"]), ptr(s["gen"]), ptr(s["weight"]),
                 stream_of(self.device)))
        return s

    def _sample_batch(self, positions, batch_size, unroll_steps, discount, draw):
        s = self._sample(positions, batch_size, draw)
        return {**self.batch_from(s, unroll_steps, discount), **s}

    def _sample_batch_values(self, positions, batch_size, unroll_steps, td_steps, discount, draw):
        s = self._sample(positions, batch_size, draw)
        return {**self.batch_values_from(s, unroll_steps, td_steps, discount), **s}

    def sample_batch(self, batch_size, unroll_steps, discount, *, seed, step, symmetries=False, beta=0.0):
        """``sample`` and ``batch_from`` in one call without the host:
        ``batch``'s dict for the sampled (game, start, symmetry) triples plus
        ``sample``'s ``items``, ``index``, ``gen`` and ``weight``.  The draw depends on (seed, step) and the
        device weights only; it is ``sample_host``'s, bit for bit."""
        return self._sample_batch(False, batch_size, unroll_steps, discount, _draw_args(seed, step, symmetries, beta))

    def batch_from(self, sample, unroll_steps, discount):
        """``batch``'s dict for a drawn ``sample`` (what ``sample`` returned, or
        its ``items`` tensor): the assembly half of ``sample_batch``
        (mzgo_replay_batch_items), so that ``reanalyse_sample`` can run between
        the draw and the assembly.  ``sample`` then ``batch_from`` gives
        ``sample_batch``'s tensors bit for bit.  No synchronisation."""
        items = self._items_of(sample)
        B, K = items.shape[0], int(unroll_steps)
        out = self._batch_out(B, K)
        check(lib.mzgo_replay_batch_items(self._h, ptr(items), B, K, float(discount), ptr(out["obs0"]),
                                          ptr(out["boot_obs"]), ptr(out["acts"]), ptr(out["t_rew"]), ptr(out["t_pol"]),
                                          ptr(out["val"]), ptr(out["factor"]), ptr(out["has_boot"]),
                                          stream_of(self.device)))
        return out

    def sample_batch_values(self, batch_size, unroll_steps, td_steps, discount, *, seed, step, symmetries=False,
                            beta=0.0):
        """``sample`` and ``batch_values_from`` in one call without the host:
        ``sample_batch``'s draw, with ``batch_values``' five tensors for the
        sampled triples."""
        return self._sample_batch_values(False, batch_size, unroll_steps, td_steps, discount,
                                         _draw_args(seed, step, symmetries, beta))

    def batch_values_from(self, sample, unroll_steps, td_steps, discount):
        """``batch_values``' dict for a drawn ``sample`` (what ``sample``
        returned, or its ``items`` tensor): the assembly half of
        ``sample_batch_values`` (mzgo_replay_batch_items_values), to run after
        ``reanalyse_sample(..., td_steps=td_steps)``.  No synchronisation."""
        items = self._items_of(sample)
        B, K = items.shape[0], int(unroll_steps)
        out = self._values_out(B, K)
        check(lib.mzgo_replay_batch_items_values(self._h, ptr(items), B, K, int(td_steps), float(discount),
                                                 ptr(out["obs0"]), ptr(out["acts"]), ptr(out["t_rew"]),
                                                 ptr(out["t_pol"]), ptr(out["t_val"]), stream_of(self.device)))
        return out

    def _items_of(self, sample):
        items = sample["items"] if isinstance(sample, dict) else sample
        if not (isinstance(items, torch.Tensor) and items.is_cuda and items.dtype == torch.int32
                and items.dim() == 2 and items.shape[1] == 3):
            raise ValueError("a sample's items are a CUDA int32 tensor [B, 3] (slot, start, symmetry)")
        return items.contiguous()

    def update_device_priorities(self, sample, per=None, alpha=1.0, *, mean=None):
        """New device weights for a sampled batch (``sample``: what ``sample``
        or ``sample_batch`` returned): ``max(per[b], FLT_MIN) ** alpha`` for
        sample b from ``per`` (a CUDA f32 tensor [B]), or from ``mean`` (a CUDA
        f64 tensor of one element) the same value for all.  A slot that has
        taken a newer game since the draw keeps that game's 1.0; a loss that
        is NaN, infinite or negative leaves the weight alone and is counted
        (``skipped_updates``).  No synchronisation."""
        B = sample["items"].shape[0]
        if (per is None) == (mean is None):
            raise ValueError("update_device_priorities: give per or mean")
        if per is not None:
            per = per.detach().to(self.device, torch.float32).reshape(-1).contiguous()
            if per.numel() != B:
                raise ValueError(f"update_device_priorities: {per.numel()} losses for {B} samples")
        else:
            mean = mean.detach().to(self.device, torch.float64).reshape(-1).contiguous()
            if mean.numel() != 1:
                raise ValueError("update_device_priorities: mean is one value")
        check(lib.mzgo_replay_update_priorities(self._h, ptr(sample["items"]), ptr(sample["gen"]), ptr(per), ptr(mean),
                                                B, float(alpha), stream_of(self.device)))

    def device_priorities(self):
        """The device weights of the games held, f64 CUDA tensor in logical
        order (oldest first)."""
        out = torch.empty(len(self), dtype=torch.float64, device=self.device)
        check(lib.mzgo_replay_priorities(self._h, ptr(out), None, stream_of(self.device)))
        return out

    def device_generations(self):
        """The slots' generation counts of the games held (int64 CUDA tensor,
        logical order): + 1 each time a game is written into the slot."""
        out = torch.empty(len(self), dtype=torch.int32, device=self.device)
        check(lib.mzgo_replay_priorities(self._h, None, ptr(out), stream_of(self.device)))
        return out.long() & 0xFFFFFFFF

    def set_device_priorities(self, values):
        """Set the device weights of the games held (logical order; finite
        values > 0 only)."""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1))
        check(lib.mzgo_replay_set_priorities(self._h, ptr(v), len(v), stream_of(self.device)))

    def skipped_updates(self):
        """How many priority updates were refused so far (synchronises)."""
        n = ctypes.c_int64()
        check(lib.mzgo_replay_skipped_updates(self._h, ctypes.byref(n), stream_of(self.device)))
        return n.value

    def sample_host(self, batch_size, *, seed, step, symmetries=False, beta=0.0):
        """The sampler's host twin on this store's present weights (copied
        back) and lengths: numpy ``items``, ``index``, ``weight``."""
        slots, length, head = self._slot_order()
        prio = np.zeros(self.capacity)
        prio[slots] = self.device_priorities().cpu().numpy()
        return sample_host(prio, length, head, batch_size, seed=seed, step=step, symmetries=symmetries, beta=beta)

    # ---- position-level priorities (opt-in on top of the device ledger) ----
    def enable_position_priorities(self, td_steps, discount, alpha=1.0, floor=None, init="td"):
        """Keep a sampling weight per stored position (MuZero's prioritized
        replay, App. G; mzgo_replay_enable_positions): f64 [capacity,
        max_moves] on the device, allocated here.  A position's weight is
        ``max(err, floor) ** alpha`` (``floor``: float32's smallest normal by
        default; raise it so that no position starves).  With ``init="td"`` a
        new game's positions start from err = |root value - n-step search-value
        target| (n = ``td_steps``, under ``discount``:
        ``position_priorities_host`` is the rule), with ``init="uniform"`` from
        1.0; the games already held get the same.  A second call with the same
        parameters is a no-op, with others an error."""
        if init not in ("td", "uniform"):
            raise ValueError(f"init must be 'td' or 'uniform', not {init!r}")
        check(lib.mzgo_replay_enable_positions(self._h, int(td_steps), float(discount), float(alpha),
                                               0.0 if floor is None else float(floor), int(init == "uniform"),
                                               stream_of(self.device)))

    def sample_positions(self, batch_size, *, seed, step, symmetries=False, beta=0.0):
        """``sample`` over positions (mzgo_replay_sample_positions, two
        launches, nothing on the host): ``batch_size`` distinct games, game s
        from position t with probability w[s, t] / total on the first draw --
        one uniform picks both.  ``sample``'s tensors; ``items[:, 1]`` is the
        drawn position and ``weight`` the importance weights over positions,
        (n_positions w / total) ** -beta over the batch's largest."""
        return self._sample(True, batch_size, _draw_args(seed, step, symmetries, beta))

    def sample_positions_batch(self, batch_size, unroll_steps, discount, *, seed, step, symmetries=False, beta=0.0):
        """``sample_batch`` with the position sampler's draw."""
        return self._sample_batch(True, batch_size, unroll_steps, discount, _draw_args(seed, step, symmetries, beta))

    def sample_positions_batch_values(self, batch_size, unroll_steps, td_steps, discount, *, seed, step,
                                      symmetries=False, beta=0.0):
        """``sample_batch_values`` with the position sampler's draw."""
        return self._sample_batch_values(True, batch_size, unroll_steps, td_steps, discount,
                                         _draw_args(seed, step, symmetries, beta))

    def update_position_priorities(self, sample, value, t_val):
        """New position weights for a sampled batch's windows
        (mzgo_replay_update_position_priorities): position start_b + k of
        sample b's game gets ``max(|value[b, k] - t_val[b, k]|, floor) **
        alpha`` from ``value`` and ``t_val``, CUDA f32 [B, K + 1] -- the raw
        value head outputs and the raw value targets (``use_value_transform``
        shapes the loss, not the priority).  Rows past the game's end and
        slots that have taken a newer game since the draw are left alone; so
        is an error that is NaN or infinite, which is counted
        (``skipped_updates``).  No synchronisation."""
        B = sample["items"].shape[0]
        value = value.detach().to(self.device, torch.float32).contiguous()
        t_val = t_val.detach().to(self.device, torch.float32).contiguous()
        if value.dim() != 2 or value.shape[0] != B or value.shape[1] < 2 or t_val.shape != value.shape:
            raise ValueError(f"update_position_priorities: value and t_val are [B, K + 1] with B = {B}, got "
                             f"{tuple(value.shape)} and {tuple(t_val.shape)}")
        check(lib.mzgo_replay_update_position_priorities(self._h, ptr(sample["items"]), ptr(sample["gen"]), ptr(value),
                                                         ptr(t_val), B, value.shape[1] - 1, stream_of(self.device)))

    def position_priorities(self):
        """The position weights of the games held: f64 CUDA tensor
        [len(self), max_moves] in logical order (oldest first); entries t >= a
        game's length are unspecified."""
        out = torch.empty(len(self), self.max_moves, dtype=torch.float64, device=self.device)
        check(lib.mzgo_replay_position_priorities(self._h, ptr(out), stream_of(self.device)))
        return out

    def set_position_priorities(self, values):
        """Set the position weights of the games held ([len(self), max_moves],
        logical order; a test hook): finite entries >= 0, and every game with
        moves keeps at least one entry > 0 among its positions."""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float64))
        if v.ndim != 2 or v.shape[1] != self.max_moves:
            raise ValueError(f"set_position_priorities: values are [games, max_moves = {self.max_moves}], got {v.shape}")
        check(lib.mzgo_replay_set_position_priorities(self._h, ptr(v), len(v), stream_of(self.device)))

    def sample_positions_host(self, batch_size, *, seed, step, symmetries=False, beta=0.0):
        """The position sampler's host twin on this store's present position
        weights (copied back) and lengths: numpy ``items``, ``index``,
        ``weight``."""
        slots, length, head = self._slot_order()
        pprio = np.zeros((self.capacity, self.max_moves))
        pprio[slots] = self.position_priorities().cpu().numpy()
        return sample_positions_host(pprio, length, head, batch_size, seed=seed, step=step, symmetries=symmetries,
                                     beta=beta)

    # ---- reanalysis in place ----
    def reanalyse(self, reanalyser, games=None):
        """Search the stored positions of ``games`` (logical indices; all by
        default) under ``reanalyser``'s engine and weights, position t of a
        game keyed (key_gid, t), latest moves first; the fresh policy rows and
        root values replace the stored ones (mzgo_replay_reanalyse).  No
        position or policy visits the host."""
        if reanalyser.N != self.N:
            raise ValueError(f"the reanalyser plays {reanalyser.N}x{reanalyser.N}, the store holds {self.N}x{self.N}")
        g = None if games is None else np.ascontiguousarray(np.asarray(games, dtype=np.int32).reshape(-1))
        check(lib.mzgo_replay_reanalyse(self._h, reanalyser.engine.handle, ptr(g), 0 if g is None else len(g),
                                        stream_of(self.device)))

    def reanalyse_sample(self, reanalyser, sample, unroll_steps, td_steps=None):
        """MuZero Reanalyse for a drawn ``sample`` (what ``sample`` returned, or
        its ``items`` tensor), without the host: the stored policy rows the
        batch is about to read -- sample b's rows start .. min(start + K, L - 1)
        -- are searched under ``reanalyser``'s engine and weights, keyed as
        ``reanalyse`` keys them, latest moves first, by one persistent queue
        launch that reads each position from the store and writes the fresh
        policy row and root value into it (mzgo_replay_reanalyse_sample).
        Rows outside the windows stay as they are.  With ``td_steps``
        (search-value targets, mzgo_replay_reanalyse_sample_values) the rows
        searched are those ``batch_values_from`` reads: the windows together
        with each sample's value rows start + td_steps .. min(start + K +
        td_steps, L - 1), a row once per sample.  Returns the number of
        positions searched as a CUDA int32 tensor of one element; nothing is
        copied back and nothing synchronises."""
        if reanalyser.N != self.N:
            raise ValueError(f"the reanalyser plays {reanalyser.N}x{reanalyser.N}, the store holds {self.N}x{self.N}")
        items = self._items_of(sample)
        n = torch.empty(1, dtype=torch.int32, device=self.device)
        if td_steps is None:
            check(lib.mzgo_replay_reanalyse_sample(self._h, reanalyser.engine.handle, ptr(items), items.shape[0],
                                                   int(unroll_steps), ptr(n), stream_of(self.device)))
        else:
            check(lib.mzgo_replay_reanalyse_sample_values(self._h, reanalyser.engine.handle, ptr(items),
                                                          items.shape[0], int(unroll_steps), int(td_steps), ptr(n),
                                                          stream_of(self.device)))
        return n

    def window_items_host(self, items, unroll_steps, td_steps=None):
        """``window_items_host`` on this store's lengths (the host mirror's,
        in slot order): numpy i32 [n,2] rows (slot, t).  ``items``: [B,3]
        (slot, start, symmetry), a tensor or an array."""
        length = self._slot_order()[1]
        if isinstance(items, dict):
            items = items["items"]
        if isinstance(items, torch.Tensor):
            items = items.cpu().numpy()
        return window_items_host(length, items, unroll_steps, td_steps)
