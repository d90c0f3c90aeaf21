"""Trainer ingestion: main.py's MuZero training step
over trajectories produced by the device self-play.

The reference trains in main.py (``MuZeroAgent.train``, main.py:381-501;
``compute_target_value``, :503-522) on trajectory dicts built by its own
self-play loop (main.py:636-713): ``observations`` T+2 (the initial
observation, one per move, the terminal one again), ``actions`` T,
``policies`` T (child-visit distributions) and ``rewards`` T+1 (the env
rewards, -0.5 added to the last one when the game hit the move cap, then the
winner).  This module produces exactly that format from the engine's records
(``trajectory_from_record``, ``MainSelfPlay`` -- main.py's MCTS and move rule
on the device, every game of a batch at once) and trains on it:

* ``mode="reference"`` -- main.py's step, quirks included: ``zero_grad`` once
  per batch but ``backward`` + ``clip_grad_norm_`` + ``optimizer.step`` per
  trajectory, so gradients accumulate across the batch;
  bootstrap values with the weights of that moment; every priority set to the
  batch's mean loss; ``StepLR`` stepped once per batch.  Pinned by a step
  recorded from the reference (``tests/golden/train_*``).
* ``mode="batched"`` -- the same losses for all B trajectories in one unroll
  (B x 10 recurrent steps, each one launch for all B) and ONE optimizer step
  on their summed gradient; the bootstrap values of every (trajectory, unroll
  step) pair come from one batched ``initial_inference`` on the HIP engine.
  With ``hip_forward=True`` the unroll's forward runs on the HIP kernels
  (``initial_inference_hip`` / ``recurrent_inference_hip``: the engine's
  k_initial_inference / k_recurrent_inference for the 3x3 convs, autograd
  Functions whose backward is the HIP kernels of csrc/mzgo_train.hip for every
  3x3 conv -- the dynamics conv from its saved input and output, the
  representation's three after recomputing its two hidden activations on the
  same kernels); the 1x1 heads stay torch ops on the engine's latents.  The
  default is torch's ops (MIOpen), measured 8 % faster at main.py's sizes.
  ``train`` also takes a ``mzgo.DeviceReplay`` here: the same targets
  (``host_targets`` and ``device_targets`` agree bit for bit) assembled on the
  device from games that never left it, optionally under a random board
  symmetry per sample (``TrainConfig.symmetries``); both feed ``_unroll_step``.
  ``TrainConfig.fused_loss`` (default off) moves the loss arithmetic of the
  K + 1 steps -- some thirty-five small torch ops each, forward and again
  backward -- onto one HIP launch (``mzgo.unroll_loss``, csrc/mzgo_loss.hip):
  the heads' outputs are stacked once, the kernel returns the per-sample
  losses, the f64 totals and the gradients with respect to every head output,
  and autograd continues from those into the heads.  With
  ``TrainConfig.sample_priorities`` (default off) a sampled game's new
  priority is its own loss (floored at float32's smallest normal) instead of
  main.py's batch mean, so the store tells sampled games apart; in batched
  mode the per-sample losses ride in the step's one synchronising copy.
  ``TrainConfig.device_sampling`` (default off; batched mode on a
  ``DeviceReplay`` only) moves the sampling and the priorities onto the
  store's device ledger: ``sample_batch`` draws the games, starts and
  symmetries and assembles the targets without the host, the priority update
  is a launch, and only the totals come back -- on demand (``read_stats``)
  with ``deferred_stats``.  ``importance_beta`` weights the loss by the
  sampler's importance weights, ``priority_alpha`` is the priority exponent.
  ``TrainConfig.device_weights`` (default off) sets ``MuZeroNet.device_weights``:
  after an optimizer step the engines take the new weights from the
  parameters in device memory (one pack launch, ``Engine.set_parameters_device``;
  a copy for the net's further engines) instead of 22 host copies and the
  host packers -- the same packed weights bit for bit.  A ``deferred_stats``
  step synchronises nowhere only with it.
  ``TrainConfig.fused_unroll`` (default off) takes the heads' outputs of all
  K + 1 steps from ``mzgo.unroll`` (csrc/mzgo_unroll.hip): the representation,
  the K dynamics steps and every head are ONE autograd node whose forward is
  one HIP call (K + 5 launches enqueued from C++) and whose backward is another
  (K + 17) -- the 3x3 convs on the kernels ``hip_forward`` uses for its
  backward, the heads and their backward on kernels that cover all K + 1
  latents in one launch each -- instead of some forty torch ops per unroll
  step.  The loss, the importance weights, the priorities and the device tail
  are unchanged: ``fused_loss`` reads the stacked outputs as they come, the
  torch loss ops read their slices.
  ``TrainConfig.unroll_precision="bf16"`` (default ``"fp32"``; ``fused_unroll``
  in batched mode, ``latent_dim`` a multiple of 32) is mixed precision for the
  dynamics conv, where nine tenths of the unroll's arithmetic are: its forward,
  its input gradient and its weight gradient run on bf16 MFMA
  (csrc/mzgo_conv_bf16.hip) with both operands rounded to bfloat16, nearest
  even, and float32 accumulation.  The master weights, the stored latents, all
  22 gradients, the representation, the heads and the optimizer stay float32,
  and the step stays deterministic.
  ``TrainConfig.reanalyse_sample`` (default off; ``device_sampling`` and a
  ``Reanalyser`` on the trainer's net) is MuZero Reanalyse inside the step:
  between the draw and the target assembly one queue launch searches exactly
  the stored positions whose policy rows the batch reads and writes the fresh
  rows into the store (``DeviceReplay.reanalyse_sample``), every
  ``reanalyse_every``-th step.

  ``TrainConfig.device_optimizer`` (default off; the net on the GPU) replaces
  the step's tail -- ``clip_grad_norm_``, ``Adam.step`` and ``StepLR.step``, some
  two dozen small torch launches over the 22 tensors -- by ``mzgo.DeviceAdam``:
  one stream-ordered call of three launches (csrc/mzgo_optim.hip) that also
  refuses a step whose gradient norm is not finite, on the device, and counts
  it (``skipped_steps``) -- with ``device_sampling`` + ``deferred_stats`` +
  ``device_weights`` no gradient visits the host, and ``clip_grad_norm_`` would
  turn one such entry into NaN in every parameter and, at the next pack, in
  every engine.  ``p.grad`` keeps the unclipped gradient.

  ``TrainConfig.value_target="search"`` (default ``"network"``; batched mode)
  takes every value target from the root values the searches left with the
  game -- ``trajectory["root_values"]`` on the host, ``Store::root_value`` in a
  ``DeviceReplay`` -- instead of a network evaluation: the n-step return of
  index i is the discounted rewards r[i] .. r[i + n - 1] plus discount^n times
  the root value of position i + n, with n = ``td_steps`` (0 = ``unroll_steps``)
  independent of the unroll length.  Where i + n is the final board, which no
  search saw, the bootstrap is the winner entry r[L] (network targets evaluate
  that board).  On a ``DeviceReplay`` the batch assembly writes ``t_val``
  itself (``batch_values``, csrc/mzgo_replay.hip k_replay_batch<true>): no
  bootstrap observations, no ``initial_inference``, no ``finish_values``; with
  ``reanalyse_sample`` the searched rows include those the value targets read.

  ``TrainConfig.position_priorities`` (default off; ``device_sampling``) is
  MuZero's own prioritized replay (paper, App. G) in place of the per-game
  weights: the store keeps a weight per stored position, the sampler draws
  (game, start) with probability proportional to it
  (``DeviceReplay.sample_positions*``; importance weights over positions), and
  after the loss the sampled windows' positions get ``max(|value - target|,
  priority_floor) ** priority_alpha`` from the step's raw value outputs and
  raw value targets (``update_position_priorities``; ``use_value_transform``
  shapes the loss, not the priority) in place of the per-game update.  A new
  game's positions start from |root value - n-step search-value target|, n =
  ``td_steps`` (``unroll_steps`` under network targets).

  ``TrainConfig.ownership_loss_weight`` (default 0 = off; batched mode with
  ``fused_unroll`` and ``fused_loss``, the net on the GPU, a ``DeviceReplay``)
  trains KataGo's ownership auxiliary target on the unroll's latents: a 1x1
  conv of its own (``mzgo.OwnershipHead``, ``trainer.ownership_head``; the
  net keeps its 22 tensors) predicts for every point who owns it on the game's
  final board, seen by the colour to move at each unroll step.  The store gives
  the targets for the step's items (``DeviceReplay.ownership`` /
  ``ownership_from``, one small launch), ``mzgo.unroll(..., return_latents=True)``
  the latents, ``mzgo.ownership_loss`` the per-sample losses, which are added to
  the unroll loss's under the same importance weights; the head's two
  parameters join the optimizer and the clip norm.  Priorities,
  ``training_loss`` and the three totals keep their meaning (without
  ownership); ``last["ownership_loss"]`` reports the ownership total.

  ``TrainConfig.consistency_loss_weight`` (default 0 = off; the ownership
  option's requirements, and ``unroll_steps`` >= 1) trains EfficientZero's
  temporal consistency loss on the same latents: ``s_k`` is pulled towards
  the representation's latent of the real board at start + k, through a head
  of two 1x1 convs of its own (``mzgo.ConsistencyHead``,
  ``trainer.consistency_head``, ``consistency_proj_dim`` wide; four parameters
  next to the net's 22) and with no gradient on the target side.  The store
  gives the windows' real boards for the step's items
  (``DeviceReplay.window_obs`` / ``window_obs_from``, one small launch),
  ``mzgo.encode`` their latents under the current weights (three launches),
  ``mzgo.consistency_loss`` the per-sample losses, added to ``per`` under the
  same importance weights.  It runs together with the ownership option: both
  gradients arrive on the one ``latents`` output.  ``last["consistency_loss"]``
  reports its total; the other totals keep their meaning.

``initial_inference_torch`` / ``recurrent_inference_torch`` restate
main.py:72-144 with torch ops on the module's own parameters (reference
mode, and the CPU).  Replay buffers restate main.py:158-244.
"""
import ctypes
import random
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from .net import MuZeroNet
from .reanalyse import FLAG_FAST, observation_planes
from .selfplay import SelfPlay


# ---------------------------------------------------------------------------
# configuration (main.py:27-53, the trainer's part)
# ---------------------------------------------------------------------------
@dataclass
class TrainConfig:
    learning_rate: float = 1e-4
    unroll_steps: int = 10
    discount: float = 0.99
    value_loss_weight: float = 1.0
    policy_loss_weight: float = 1.0
    reward_loss_weight: float = 1.0
    use_value_transform: bool = True
    lr_step_size: int = 1000          # StepLR(step_size=1000, gamma=0.9), main.py:379
    lr_gamma: float = 0.9
    max_grad_norm: float = 1.0        # main.py:481
    symmetries: bool = False          # DeviceReplay batches: a random board symmetry per sample (not in main.py)
    fused_loss: bool = False          # batched mode: the unroll's loss and head gradients on mzgo_unroll_loss
    sample_priorities: bool = False   # a sampled game's priority = its own loss (main.py: the batch mean)
    device_sampling: bool = False     # DeviceReplay: sample and update priorities on the device (its own ledger)
    importance_beta: float = 0.0      # device_sampling: importance-weight exponent (0 = unweighted loss)
    priority_alpha: float = 1.0       # device_sampling: a new priority is loss ** alpha
    deferred_stats: bool = False      # device_sampling: train() returns a device scalar; read_stats() fills last
    device_weights: bool = False      # the net's engines take new weights on the device (MuZeroNet.device_weights)
    fused_unroll: bool = False        # batched mode: the whole unroll, heads included, on mzgo.unroll (one autograd node)
    reanalyse_sample: bool = False    # device_sampling: search the sampled windows' positions before the targets
    reanalyse_every: int = 1          # reanalyse_sample: on the steps with sample_step % reanalyse_every == 0
    device_optimizer: bool = False    # batched mode: clip + Adam + StepLR as one HIP call (mzgo.DeviceAdam)
    value_target: str = "network"     # "network": main.py's bootstrap; "search": the stored root values (batched mode)
    td_steps: int = 0                 # value_target="search": the n-step horizon; 0 = unroll_steps
    unroll_precision: str = "fp32"    # fused_unroll: "bf16" runs the dynamics conv's products on bf16 MFMA
    position_priorities: bool = False  # device_sampling: sample positions by |value - target| (MuZero, App. G)
    priority_floor: float = 0.0       # position_priorities: the smallest value error a weight is formed from; 0 = FLT_MIN
    ownership_loss_weight: float = 0.0  # > 0: the ownership head's loss on the fused unroll's latents (DeviceReplay)
    consistency_loss_weight: float = 0.0  # > 0: the latent consistency loss on the fused unroll's latents (DeviceReplay)
    consistency_proj_dim: int = 32    # consistency_loss_weight: the head's projection width (16, 32, 48 or 64)


def reward_value_transform(x, epsilon=0.001):
    """h(x) = sign(x) (sqrt(|x| + 1) - 1) + eps x (main.py:66-69)."""
    return torch.sign(x) * (torch.sqrt(torch.abs(x) + 1) - 1) + epsilon * x


# ---------------------------------------------------------------------------
# differentiable forward (main.py:72-144), on the MuZeroNet's parameters
# ---------------------------------------------------------------------------
def _prediction(net, latent):
    p = net.prediction
    value = p.value_fc(p.value_conv(latent).mean(dim=[2, 3]))
    policy_map = p.policy_conv(latent)
    b = policy_map.size(0)
    logits = torch.cat([policy_map.view(b, -1), p.pass_logit.expand(b, 1)], dim=1)
    return value, logits


def initial_inference_torch(net, observation):
    r = net.representation
    x = F.relu(r.conv1(observation))
    x = F.relu(r.conv2(x))
    latent = F.relu(r.conv3(x))
    value, logits = _prediction(net, latent)
    return latent, value, logits


def recurrent_inference_torch(net, latent, action):
    d = net.dynamics
    b = latent.shape[0]
    emb = d.action_embedding(action).view(b, latent.shape[1], 1, 1).expand_as(latent)
    x = F.relu(d.conv(latent + emb))
    reward = d.fc_reward_output(F.relu(d.fc_reward_hidden(d.reward_conv(x).mean(dim=[2, 3]))))
    value, logits = _prediction(net, x)
    return x, reward, value, logits


# ---------------------------------------------------------------------------
# the same networks with the forward on the HIP engine (SURVEY.md §8(f) 1:
# "forward only through HIP, backward via torch")
# ---------------------------------------------------------------------------
def conv3x3_forward_hip(x, weight, bias):
    """relu(conv3x3(x) + bias), padding 1, on the HIP fp32-MFMA kernel
    (mzgo_conv3x3_relu_forward): the representation's hidden activations
    recomputed for its backward (main.py:72-84)."""
    from ._lib import check, lib, ptr, stream_of
    B, Cin, N, _ = x.shape
    Cout = weight.shape[0]
    dev = x.device
    f = [t.detach().to(dev, torch.float32).contiguous() for t in (x, weight, bias)]
    y = torch.empty(B, Cout, N, N, device=dev)
    check(lib.mzgo_conv3x3_relu_forward(ptr(f[0]), None, None, ptr(f[1]), ptr(f[2]), B, Cin, Cout, N, ptr(y),
                                        stream_of(dev)))
    return y


def conv3x3_backward_hip(g, out, x, weight, action=None, emb=None, need_input_grad=True):
    """Backward of out = relu(conv3x3(x') + b), x' = x (+ emb[action] broadcast),
    on the HIP kernels (mzgo_conv3x3_backward: fp32 MFMA implicit GEMMs,
    deterministic; replaces torch.nn.grad.conv2d_input / conv2d_weight): with
    gp = g * [out > 0], returns (d x or None, d weight, d bias)."""
    from ._lib import check, lib, ptr, stream_of
    B, Cin, N, _ = x.shape
    Cout = weight.shape[0]
    dev = x.device
    f = [t.detach().to(dev, torch.float32).contiguous() for t in (g, out, x, weight)]
    e = emb.detach().to(dev, torch.float32).contiguous() if emb is not None else None
    act = action.to(dev, torch.int64).contiguous() if action is not None else None
    ws = ctypes.c_int64()
    check(lib.mzgo_conv3x3_backward_workspace(B, Cin, Cout, ctypes.byref(ws)))
    work = torch.empty(ws.value, dtype=torch.uint8, device=dev)
    gx = torch.empty_like(f[2]) if need_input_grad else None
    gw = torch.empty_like(f[3])
    gb = torch.empty(Cout, device=dev)
    check(lib.mzgo_conv3x3_backward(ptr(f[0]), ptr(f[1]), ptr(f[2]), ptr(act), ptr(e), ptr(f[3]), B, Cin, Cout, N,
                                    ptr(gx), ptr(gw), ptr(gb), ptr(work), ws.value, stream_of(dev)))
    return gx, gw, gb


def dyn_conv_backward_hip(g, nxt, latent, action, emb, weight):
    """The dynamics conv's backward on the HIP kernels (mzgo_dyn_conv_backward,
    csrc/mzgo_train.hip): with gp = g * [nxt > 0], returns (d latent, d weight,
    d bias) of nxt = relu(conv3x3(latent + emb[action]) + bias), main.py:97-103."""
    from ._lib import check, lib, ptr, stream_of
    B, C, N, _ = latent.shape
    dev = latent.device
    f = [t.detach().to(dev, torch.float32).contiguous() for t in (g, nxt, latent, emb, weight)]
    act = action.to(dev, torch.int64).contiguous()
    ws = ctypes.c_int64()
    check(lib.mzgo_dyn_conv_backward_workspace(B, C, ctypes.byref(ws)))
    work = torch.empty(ws.value, dtype=torch.uint8, device=dev)
    gx = torch.empty_like(f[2])
    gw = torch.empty_like(f[4])
    gb = torch.empty(C, device=dev)
    check(lib.mzgo_dyn_conv_backward(ptr(f[0]), ptr(f[1]), ptr(f[2]), ptr(act), ptr(f[3]), ptr(f[4]), B, C, N,
                                     ptr(gx), ptr(gw), ptr(gb), ptr(work), ws.value, stream_of(dev)))
    return gx, gw, gb


class _HipDynamicsConv(torch.autograd.Function):
    """x' = relu(conv3x3(latent + emb[a]) + b) (main.py:97-103) with the
    forward on the engine's k_recurrent_inference and the backward on the
    HIP backward kernels from the saved input and output (ReLU mask = x' > 0;
    dyn_conv_backward_hip); the embedding's gradient = the input gradient
    summed over the board, added into row a."""

    @staticmethod
    def forward(ctx, latent, action, weight, bias, emb, net):
        nxt, _, _, _ = net.engine().recurrent_inference(latent.detach(), action)
        ctx.save_for_backward(latent, action, weight, emb, nxt)
        return nxt

    @staticmethod
    def backward(ctx, g):
        latent, action, weight, emb, nxt = ctx.saved_tensors
        gx, gw, gb = dyn_conv_backward_hip(g, nxt, latent, action, emb, weight)
        gemb = torch.zeros_like(emb).index_add_(0, action, gx.sum(dim=(2, 3)))
        return gx, None, gw, gb, gemb, None


class _HipRepresentation(torch.autograd.Function):
    """The representation (main.py:72-84) with the forward on the engine's
    k_initial_inference and the backward on the HIP kernels: the two hidden
    activations recomputed (mzgo_conv3x3_relu_forward; the engine keeps them
    on chip), then each conv's input / weight / bias gradients from the saved
    input and output (mzgo_conv3x3_backward), conv3 -> conv2 -> conv1."""

    @staticmethod
    def forward(ctx, obs, w1, b1, w2, b2, w3, b3, net):
        lat, _, _ = net.engine().initial_inference(obs.detach())
        ctx.save_for_backward(obs, w1, b1, w2, b2, w3, b3, lat)
        return lat

    @staticmethod
    def backward(ctx, g):
        obs, w1, b1, w2, b2, w3, b3, lat = ctx.saved_tensors
        x1 = conv3x3_forward_hip(obs, w1, b1)
        x2 = conv3x3_forward_hip(x1, w2, b2)
        g2, gw3, gb3 = conv3x3_backward_hip(g, lat, x2, w3)
        g1, gw2, gb2 = conv3x3_backward_hip(g2, x2, x1, w2)
        _, gw1, gb1 = conv3x3_backward_hip(g1, x1, obs, w1, need_input_grad=False)
        return None, gw1, gb1, gw2, gb2, gw3, gb3, None


def initial_inference_hip(net, observation):
    r = net.representation
    latent = _HipRepresentation.apply(observation.contiguous(), r.conv1.weight, r.conv1.bias, r.conv2.weight,
                                      r.conv2.bias, r.conv3.weight, r.conv3.bias, net)
    value, logits = _prediction(net, latent)
    return latent, value, logits


def recurrent_inference_hip(net, latent, action):
    d = net.dynamics
    x = _HipDynamicsConv.apply(latent.contiguous(), action.contiguous(), d.conv.weight, d.conv.bias,
                               d.action_embedding.weight, net)
    reward = d.fc_reward_output(F.relu(d.fc_reward_hidden(d.reward_conv(x).mean(dim=[2, 3]))))
    value, logits = _prediction(net, x)
    return x, reward, value, logits


# ---------------------------------------------------------------------------
# replay buffers (main.py:158-244)
# ---------------------------------------------------------------------------
class PrioritizedReplayBuffer:
    def __init__(self, capacity):
        self.capacity = capacity
        self.buffer = []
        self.priorities = []

    def add(self, trajectory):
        if len(self.buffer) >= self.capacity:
            self.buffer.pop(0)
            self.priorities.pop(0)
        self.buffer.append(trajectory)
        self.priorities.append(1.0)

    def sample(self, batch_size):
        priorities = np.array(self.priorities)
        probs = priorities / priorities.sum()
        indices = np.random.choice(len(self.buffer), batch_size, replace=False, p=probs)
        return [self.buffer[i] for i in indices], indices

    def update_priorities(self, indices, new_priorities):
        for i, p in zip(indices, new_priorities):
            self.priorities[i] = p


class MultiVersionReplayBuffer:
    """Buffers of the last ``num_versions`` model versions, sampled jointly."""

    def __init__(self, capacity, num_versions=1, prioritized=True):
        from collections import deque
        self.capacity = capacity
        self.prioritized = prioritized
        self.buffers = deque(maxlen=num_versions)
        self.add_version()

    def add_version(self):
        from collections import deque
        self.buffers.append(PrioritizedReplayBuffer(self.capacity) if self.prioritized
                            else deque(maxlen=self.capacity))

    def add(self, trajectory):
        if self.prioritized:
            self.buffers[-1].add(trajectory)
        else:
            self.buffers[-1].append(trajectory)

    def sample(self, batch_size):
        if not self.prioritized:
            combined = [t for buf in self.buffers for t in buf]
            if len(combined) < batch_size:
                return [], []
            return random.sample(combined, batch_size), None
        combined, combined_p, owner = [], [], []
        for b, buf in enumerate(self.buffers):
            combined.extend(buf.buffer)
            combined_p.extend(buf.priorities)
            owner.extend((b, i) for i in range(len(buf.buffer)))
        if len(combined) < batch_size:
            return [], []
        probs = np.array(combined_p) / sum(combined_p)
        indices = np.random.choice(len(combined), batch_size, replace=False, p=probs)
        return [combined[i] for i in indices], [owner[i] for i in indices]

    def update_priorities(self, mapping, new_priorities):
        if not self.prioritized or mapping is None:
            return
        for (b, i), p in zip(mapping, new_priorities):
            if b < len(self.buffers):
                self.buffers[b].priorities[i] = p


# ---------------------------------------------------------------------------
# trajectories in main.py's format
# ---------------------------------------------------------------------------
_planes = observation_planes             # (the name tests import)


def trajectory_from_record(rec, final_obs, board_size, max_moves):
    """main.py:636-713's trajectory from an engine record (``Engine.record``)
    and the board after the game's last move (``final_obs``, f64 [6,N,N]):
    observations T+2, actions T, policies T, rewards T+1."""
    N = board_size
    L = int(rec["length"])
    acts = [int(a) for a in rec["action"][:L]]
    obs = [_planes(rec["stones"][t], rec["invd"][t], int(rec["flags"][t]), N) for t in range(L)]
    final_obs = np.asarray(final_obs, dtype=np.float64)
    done = bool(final_obs[5].max() > 0)
    rewards = [float(r) for r in rec["reward"][:L]]
    if not done and L >= max_moves and rewards:
        rewards[-1] += -0.5                      # main.py:699-702 (move cap)
    winner = float(rec["final_reward"]) if done else 0.0   # env.winner(): 0 unless ended
    out = {
        "observations": obs + [final_obs, final_obs],
        "actions": acts,
        "rewards": rewards + [winner],
        "policies": [np.array(p, dtype=np.float64) for p in rec["policy"][:L]],
    }
    # playout cap randomization: the moves searched with the fast budget (flags
    # bit 3), whose policies are no targets -- only when the game has one
    fast = [bool(int(rec["flags"][t]) & FLAG_FAST) for t in range(L)]
    if any(fast):
        out["fast_search"] = fast
    return out


class MainSelfPlay:
    """main.py's self-play loop (main.py:636-713) for G games at once: its MCTS
    (``search_variant="main"``: c_puct 2, Dirichlet(0.03) at 0.25, pass prior
    0.05), its move rule (argmax of child visits, main.py:660-673) and its
    move cap int(1.5 N^2) (main.py:51).  ``play()`` returns main.py
    trajectories."""

    def __init__(self, net, num_games, num_simulations, *, seed=1234, game_base=0, dynamics="factored",
                 fast_simulations=0, full_search_prob=1.0):
        N = net.board_size
        self.max_moves = int(N * N * 1.5)
        self.N = N
        self.sp = SelfPlay(net, num_games, num_simulations, seed=seed, compat="fixed", max_moves=self.max_moves,
                           game_base=game_base, c_puct=2.0, dirichlet_alpha=0.03, dirichlet_epsilon=0.25,
                           pass_epsilon=0.05, search_variant="main", dynamics=dynamics,
                           fast_simulations=fast_simulations, full_search_prob=full_search_prob)

    def refresh(self):
        """The net's current weights into the self-play engine (``SelfPlay.refresh``)."""
        return self.sp.refresh()

    def play(self):
        sp = self.sp
        sp.reset()
        for _ in range(self.max_moves):
            sp.move()
        eng = sp.engine
        if eng.counters()["playing"] != 0:
            raise RuntimeError("games still playing after max_moves moves")
        finals = eng.board_planes().cpu().numpy()
        out = [trajectory_from_record(eng.record(g), finals[g], self.N, self.max_moves) for g in range(sp.G)]
        sp.epoch += 1
        return out

    def play_into(self, replay):
        """``play()`` with the games left on the device: the G trajectories go
        into ``replay`` (a ``DeviceReplay`` with this engine's board size and
        move cap) in one device-to-device launch, in slot order; only their
        lengths come back.  ``replay.export(i)`` is what ``play()`` returns."""
        sp = self.sp
        sp.reset()
        for _ in range(self.max_moves):
            sp.move()
        replay.add_games(sp.engine)          # (refuses while a game is still playing)
        sp.epoch += 1

    def play_games_into(self, replay, n_games):
        """``n_games`` games -- any number up to the store's capacity, not the
        engine's G -- into ``replay`` from one launch (``SelfPlay.play_games_into``):
        the games ``ceil(n_games / G)`` calls of ``play_into`` store (of the
        last, its first ``n_games % G`` when that is not 0), without a launch
        per move or a tail per G games."""
        self.sp.play_games_into(replay, n_games)


# ---------------------------------------------------------------------------
# the training step (main.py:381-522)
# ---------------------------------------------------------------------------
class MuZeroTrainer:
    """main.py's ``MuZeroAgent`` training half: Adam + StepLR on ``net``'s
    parameters, ``train(replay_buffer, batch_size)`` as main.py:381-501.

    ``start_index(trajectory_length)`` draws a trajectory's start (main.py:395
    ``random.randint(0, T - 1)``; tests pass a fixed sequence).

    For inspection and tests, a ``device_sampling`` step leaves two device
    tensors behind without synchronising: ``last_searched_device`` (i32 [1],
    the positions ``reanalyse_sample`` searched on the last searched step) and
    ``last_t_val_device`` (f32 [B, K+1], the value targets the last step
    trained on, under either ``value_target``; held until the next step)."""

    def __init__(self, net: MuZeroNet, config: TrainConfig = None, mode="reference", start_index=None,
                 hip_forward=None, sample_seed=0, reanalyser=None, ownership_head=None, consistency_head=None):
        if mode not in ("reference", "batched"):
            raise ValueError(f"mode must be 'reference' or 'batched', not {mode!r}")
        self.net = net
        # batched mode: the unroll's forward and 3x3-conv backward on the HIP
        # kernels (hip_forward=True) or on torch's ops (MIOpen convs, the
        # default): measured at main.py's 6x6 / C=128 / batch 128 x unroll 10,
        # the network part takes 10.49 ms on the HIP kernels and 9.71 ms on
        # MIOpen, the whole step 22.1 vs 21.0 ms (scripts/trainer_timing.py,
        # profiles/r5_trainer_step.json), so the faster one is the default
        self.hip_forward = False if hip_forward is None else hip_forward
        self.config = config or TrainConfig()
        if self.config.fused_loss and mode != "batched":
            raise ValueError("fused_loss needs mode='batched': mode='reference' is main.py's per-trajectory step, "
                             "whose loss is built and backpropagated one trajectory at a time")
        c = self.config
        if c.device_sampling and mode != "batched":
            raise ValueError("device_sampling needs mode='batched' and a DeviceReplay: mode='reference' is main.py's "
                             "per-trajectory step over host trajectories")
        if not c.device_sampling and (c.deferred_stats or c.importance_beta != 0.0 or c.priority_alpha != 1.0):
            raise ValueError("deferred_stats, importance_beta and priority_alpha belong to device_sampling "
                             "(TrainConfig.device_sampling=True)")
        if c.importance_beta < 0 or not c.priority_alpha > 0:
            raise ValueError("importance_beta must be >= 0 and priority_alpha > 0")
        if c.position_priorities and not c.device_sampling:
            raise ValueError("position_priorities needs device_sampling (TrainConfig.device_sampling=True) in "
                             "mode='batched': the position weights live in the DeviceReplay's device ledger")
        if not c.position_priorities and c.priority_floor != 0.0:
            raise ValueError("priority_floor belongs to position_priorities (TrainConfig.position_priorities=True)")
        if not (0.0 <= c.priority_floor < float("inf")):
            raise ValueError(f"priority_floor must be finite and >= 0 (0 = float32's smallest normal), got "
                             f"{c.priority_floor}")
        if not (0.0 <= c.ownership_loss_weight < float("inf")):
            raise ValueError(f"ownership_loss_weight must be finite and >= 0 (0 = off), got {c.ownership_loss_weight}")
        if c.ownership_loss_weight > 0:
            if mode != "batched":
                raise ValueError("ownership_loss_weight needs mode='batched' with fused_unroll and fused_loss: "
                                 "mode='reference' is main.py's per-trajectory step, which has no ownership head")
            if not c.fused_unroll:
                raise ValueError("ownership_loss_weight needs fused_unroll=True: the ownership head reads the latents "
                                 "mzgo.unroll returns (return_latents=True)")
            if not c.fused_loss:
                raise ValueError("ownership_loss_weight needs fused_loss=True: the ownership loss joins the per-sample "
                                 "losses of mzgo.unroll_loss")
            if next(net.parameters()).device.type != "cuda":
                raise ValueError("ownership_loss_weight needs the net on the GPU (net.to('cuda')): "
                                 "mzgo.ownership_loss has no eager fall-back")
            from .ownership import OwnershipHead
            if ownership_head is None:
                ownership_head = OwnershipHead(net.latent_dim).to(next(net.parameters()).device)
            if not isinstance(ownership_head, OwnershipHead) or ownership_head.latent_dim != net.latent_dim:
                raise ValueError(f"ownership_head must be an OwnershipHead({net.latent_dim}) (the net's latent_dim)")
            if ownership_head.conv.weight.device != next(net.parameters()).device:
                raise ValueError("ownership_head must be on the net's device")
        elif ownership_head is not None:
            raise ValueError("ownership_head belongs to ownership_loss_weight > 0 (TrainConfig.ownership_loss_weight)")
        # the ownership head (None: off): a module of its own -- the net keeps the reference's 22 tensors, and the
        # engines, the weight packers and the search never see the head; its two parameters join the optimizer's
        self.ownership_head = ownership_head
        if not (0.0 <= c.consistency_loss_weight < float("inf")):
            raise ValueError(f"consistency_loss_weight must be finite and >= 0 (0 = off), got "
                             f"{c.consistency_loss_weight}")
        if c.consistency_loss_weight > 0:
            if mode != "batched":
                raise ValueError("consistency_loss_weight needs mode='batched' with fused_unroll and fused_loss: "
                                 "mode='reference' is main.py's per-trajectory step, which has no consistency head")
            if not c.fused_unroll:
                raise ValueError("consistency_loss_weight needs fused_unroll=True: the consistency head reads the "
                                 "latents mzgo.unroll returns (return_latents=True)")
            if not c.fused_loss:
                raise ValueError("consistency_loss_weight needs fused_loss=True: the consistency loss joins the "
                                 "per-sample losses of mzgo.unroll_loss")
            if int(c.unroll_steps) < 1:
                raise ValueError(f"consistency_loss_weight needs unroll_steps >= 1 (the loss is on the latents of "
                                 f"steps 1..K), got {c.unroll_steps}")
            from .consistency import MAX_LATENT_DIM, ConsistencyHead
            if net.latent_dim > MAX_LATENT_DIM:
                raise ValueError(f"consistency_loss_weight needs latent_dim <= {MAX_LATENT_DIM} (the kernels stage "
                                 f"the projection's weights in LDS), got {net.latent_dim}")
            if consistency_head is not None and (not isinstance(consistency_head, ConsistencyHead)
                                                 or consistency_head.latent_dim != net.latent_dim):
                raise ValueError(f"consistency_head must be a ConsistencyHead({net.latent_dim}, proj_dim) (the net's "
                                 "latent_dim)")
            if next(net.parameters()).device.type != "cuda":
                raise ValueError("consistency_loss_weight needs the net on the GPU (net.to('cuda')): "
                                 "mzgo.consistency_loss has no eager fall-back")
            if consistency_head is None:       # (a proj_dim outside 16, 32, 48, 64 is the head's ValueError)
                consistency_head = ConsistencyHead(net.latent_dim, c.consistency_proj_dim).to(
                    next(net.parameters()).device)
            if consistency_head.proj.weight.device != next(net.parameters()).device:
                raise ValueError("consistency_head must be on the net's device")
        elif consistency_head is not None or c.consistency_proj_dim != 32:
            raise ValueError("consistency_head and consistency_proj_dim belong to consistency_loss_weight > 0 "
                             "(TrainConfig.consistency_loss_weight)")
        # the consistency head (None: off): a module of its own like the ownership head; its four parameters join
        # the optimizer's
        self.consistency_head = consistency_head
        if c.unroll_precision not in ("fp32", "bf16"):
            raise ValueError(f"unroll_precision must be 'fp32' or 'bf16', not {c.unroll_precision!r}")
        if c.unroll_precision == "bf16":
            if mode != "batched":
                raise ValueError("unroll_precision='bf16' needs mode='batched' and fused_unroll=True: mode='reference' "
                                 "is main.py's per-trajectory float32 step")
            if not c.fused_unroll:
                raise ValueError("unroll_precision='bf16' needs fused_unroll=True: the bf16 kernels are mzgo.unroll's "
                                 "(the per-layer paths are float32 only)")
            if isinstance(net, MuZeroNet) and net.latent_dim % 32:
                raise ValueError(f"unroll_precision='bf16' needs latent_dim to be a multiple of 32, got "
                                 f"{net.latent_dim}")
        if c.fused_unroll:
            if not isinstance(net, MuZeroNet):
                raise ValueError(f"fused_unroll runs the reference network (MuZeroNet) only, not {type(net).__name__}: "
                                 "mzgo.unroll has no kernels for another architecture")
            if mode != "batched":
                raise ValueError("fused_unroll needs mode='batched': mode='reference' is main.py's per-trajectory "
                                 "step, which unrolls one trajectory at a time")
            if self.hip_forward:
                raise ValueError("fused_unroll and hip_forward=True are two different HIP paths for the unroll "
                                 "(one autograd node for all of it / one Function per conv layer): choose one")
            if net.latent_dim < 16 or net.latent_dim % 16:
                raise ValueError(f"fused_unroll needs latent_dim to be a multiple of 16, got {net.latent_dim}")
            if next(net.parameters()).device.type != "cuda":
                raise ValueError("fused_unroll needs the net on the GPU (net.to('cuda')): mzgo.unroll has no eager "
                                 "fall-back")
        if c.device_weights:
            if next(net.parameters()).device.type != "cuda":
                raise ValueError("device_weights needs the net on the GPU (net.to('cuda')): the engines' weights are "
                                 "packed from the parameters in device memory")
            net.device_weights = True
        if c.reanalyse_sample:
            if not c.device_sampling:
                raise ValueError("reanalyse_sample needs device_sampling (TrainConfig.device_sampling=True): the "
                                 "windows are searched from the sampler's device items")
            if reanalyser is None or getattr(reanalyser, "net", None) is not net:
                raise ValueError("reanalyse_sample needs a Reanalyser on the trainer's net "
                                 "(MuZeroTrainer(net, ..., reanalyser=Reanalyser(net, num_simulations)))")
            if int(c.reanalyse_every) < 1:
                raise ValueError(f"reanalyse_every must be >= 1, got {c.reanalyse_every}")
        elif reanalyser is not None or c.reanalyse_every != 1:
            raise ValueError("reanalyser and reanalyse_every belong to reanalyse_sample "
                             "(TrainConfig.reanalyse_sample=True)")
        if c.device_optimizer:
            if mode != "batched":
                raise ValueError("device_optimizer needs mode='batched': mode='reference' is main.py's per-trajectory "
                                 "step, which clips and steps the optimizer once per trajectory")
            if next(net.parameters()).device.type != "cuda":
                raise ValueError("device_optimizer needs the net on the GPU (net.to('cuda')): mzgo.DeviceAdam has no "
                                 "eager fall-back")
        if c.value_target not in ("network", "search"):
            raise ValueError(f"value_target must be 'network' or 'search', not {c.value_target!r}")
        if int(c.td_steps) < 0:
            raise ValueError(f"td_steps must be >= 0 (0 = unroll_steps), got {c.td_steps}")
        if c.value_target == "search":
            if mode != "batched":
                raise ValueError("value_target='search' needs mode='batched': mode='reference' is main.py's own "
                                 "step, whose value targets bootstrap from the network")
        elif c.td_steps != 0:
            raise ValueError("td_steps belongs to value_target='search' (TrainConfig.value_target): network targets "
                             "bootstrap unroll_steps moves on, as main.py does")
        # value_target="search": the n of the n-step return (None: network targets)
        self.td_steps = (int(c.td_steps) or int(c.unroll_steps)) if c.value_target == "search" else None
        self.reanalyser = reanalyser
        self.mode = mode
        self.sample_seed = int(sample_seed)   # device_sampling: the sampler's seed; its step is sample_step
        self.sample_step = 0                  # steps taken with device_sampling
        self._pending = None                  # device_sampling: the last step's totals, still on the device
        self.last_per_sample_device = None    # device_sampling + sample_priorities: the per-sample losses (CUDA)
        self.last_searched_device = None      # reanalyse_sample: the positions the last searched step searched (CUDA i32 [1])
        self.last_t_val_device = None         # device_sampling: the value targets the last step trained on (CUDA f32 [B, K+1])
        self.action_size = net.board_size ** 2 + 1
        if c.device_optimizer:
            from .optim import DeviceAdam
            # clip_grad_norm_, Adam and StepLR in one: ``scheduler`` has nothing left to step
            self.optimizer = DeviceAdam(self._parameters(), lr=c.learning_rate, max_grad_norm=c.max_grad_norm,
                                        lr_step_size=c.lr_step_size, lr_gamma=c.lr_gamma)
            self.scheduler = None
        else:
            self.optimizer = torch.optim.Adam(self._parameters(), lr=self.config.learning_rate)
            self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=self.config.lr_step_size,
                                                             gamma=self.config.lr_gamma)
        self.start_index = start_index or (lambda T: random.randint(0, T - 1))
        self.symmetry_index = lambda: random.randrange(8)      # TrainConfig.symmetries
        self.last = {}
        self.last_per_sample = None      # TrainConfig.sample_priorities: the last step's per-sample losses (numpy)

    @property
    def device(self):
        return next(self.net.parameters()).device

    def _parameters(self):
        """What the optimizer steps and one clip norm covers: the net's 22 tensors, then the ownership head's two
        and the consistency head's four."""
        params = list(self.net.parameters())
        if self.ownership_head is not None:
            params += list(self.ownership_head.parameters())
        if self.consistency_head is not None:
            params += list(self.consistency_head.parameters())
        return params

    # -- targets ------------------------------------------------------------
    def _discounted(self, trajectory, index):
        """The reward part of compute_target_value (main.py:503-515) and the
        bootstrap position (or None)."""
        c = self.config
        target, factor = 0.0, 1.0
        rewards = trajectory["rewards"]
        T = len(rewards)
        for k in range(c.unroll_steps):
            j = index + k
            if j >= T:
                break
            target += factor * rewards[j]
            factor *= c.discount
        boot = index + c.unroll_steps if index + c.unroll_steps < T else None
        return target, factor, boot

    def _search_value(self, trajectory, index):
        """The search-value target of ``index`` (value_target="search"): the
        rewards of ``td_steps`` moves, then the stored root value of the
        position reached -- or, where that is the final board, which no search
        saw, the winner entry r[L] -- in float64, mzgo_replay.hpp's
        search_value_target operation by operation."""
        rewards, nu = trajectory["rewards"], trajectory["root_values"]
        L, n = len(trajectory["actions"]), self.td_steps
        target, factor = 0.0, 1.0
        for j in range(index, index + n):
            if j > L:
                break
            target += factor * float(rewards[j])
            factor *= self.config.discount
        if index + n <= L - 1:
            target += factor * float(nu[index + n])
        elif index + n == L:
            target += factor * float(rewards[L])
        return target

    def compute_target_value(self, trajectory, index, unroll_steps=None):
        """main.py:503-522 (bootstrap value from the current weights)."""
        target, factor, boot = self._discounted(trajectory, index)
        if boot is not None:
            obs = torch.as_tensor(np.asarray(trajectory["observations"][boot]), dtype=torch.float32,
                                  device=self.device).unsqueeze(0)
            with torch.no_grad():
                _, value, _ = initial_inference_torch(self.net, obs)
            target += factor * value.item()
        return target

    def _policy_target(self, trajectory, i):
        pol = trajectory["policies"]
        if i >= len(pol):
            return np.ones(self.action_size) / self.action_size
        # a move searched with the fast budget (playout cap randomization) is no
        # policy target: the all-zero row the device assembly writes, on which
        # the loss and its gradient are exactly 0
        fast = trajectory.get("fast_search")
        if fast is not None and fast[i]:
            return np.zeros(self.action_size)
        return pol[i]

    def _value_loss(self, value, target):
        if self.config.use_value_transform:
            return F.mse_loss(reward_value_transform(value), reward_value_transform(target), reduction="none")
        return F.mse_loss(value, target, reduction="none")

    # -- main.py's step -------------------------------------------------------
    def train(self, replay_buffer, batch_size):
        from .replay import DeviceReplay
        if isinstance(replay_buffer, DeviceReplay):
            return self._train_device(replay_buffer, batch_size)
        if self.config.device_sampling:
            raise ValueError("device_sampling needs a DeviceReplay: a host buffer has no device ledger to sample")
        if self.ownership_head is not None:
            raise ValueError("ownership_loss_weight needs a DeviceReplay: the ownership targets come from the final "
                             "boards the store keeps (host trajectories are out of scope)")
        if self.consistency_head is not None:
            raise ValueError("consistency_loss_weight needs a DeviceReplay: the targets are the real boards the store "
                             "keeps for the window (host trajectories are out of scope)")
        batch, indices = replay_buffer.sample(batch_size)
        if not batch or len(batch) < batch_size:
            return None
        avg = self._train_reference(batch) if self.mode == "reference" else self._train_batched(batch)
        if indices is not None:
            replay_buffer.update_priorities(indices, self._priorities(avg, len(indices)))
        self._scheduler_step()
        return avg

    def _scheduler_step(self):
        """StepLR once per batch (main.py:500); ``device_optimizer``'s step has done it."""
        if self.scheduler is not None:
            self.scheduler.step()

    def _optimizer_step(self):
        """The step's tail after ``backward()``: ``clip_grad_norm_`` and Adam's
        step, or with ``device_optimizer`` the one call that is both (and
        StepLR's).  Returns the learning rate the step used."""
        if self.config.device_optimizer:
            lr = self.optimizer.lr
            self.optimizer.step()
            return lr
        torch.nn.utils.clip_grad_norm_(self._parameters(), max_norm=self.config.max_grad_norm)
        self.optimizer.step()
        return self.optimizer.param_groups[0]["lr"]

    def skipped_steps(self):
        """``device_optimizer``: the optimizer steps refused so far because the
        gradient norm was not finite (synchronises)."""
        if not self.config.device_optimizer:
            raise ValueError("skipped_steps belongs to device_optimizer (TrainConfig.device_optimizer=True): "
                             "torch's Adam refuses nothing")
        return self.optimizer.skipped()

    def _priorities(self, avg, n):
        """The sampled games' new priorities: the batch's mean loss for every
        one (main.py:498-499), or with ``sample_priorities`` each game's own
        loss, kept positive (``np.random.choice`` takes no weight <= 0)."""
        if not self.config.sample_priorities:
            return [avg] * n
        tiny = float(np.finfo(np.float32).tiny)
        return [max(float(p), tiny) for p in self.last_per_sample]

    def _train_reference(self, batch):
        c, dev, net = self.config, self.device, self.net
        A = self.action_size
        loss_total = tot_v = tot_p = tot_r = 0.0
        per = []
        self.optimizer.zero_grad()                       # once per batch (main.py:391)
        for trajectory in batch:
            T = len(trajectory["actions"])
            start = self.start_index(T)
            obs = torch.as_tensor(np.asarray(trajectory["observations"][start]), dtype=torch.float32,
                                  device=dev).unsqueeze(0)
            latent, value, logits = initial_inference_torch(net, obs)
            tv = torch.tensor(self.compute_target_value(trajectory, start), dtype=torch.float32, device=dev)
            tp = torch.tensor(self._policy_target(trajectory, start), dtype=torch.float32, device=dev)
            v_loss = self._value_loss(value.squeeze(), tv)
            p_loss = F.kl_div(F.log_softmax(logits, dim=1), tp, reduction="batchmean")
            step_loss = c.value_loss_weight * v_loss + c.policy_loss_weight * p_loss
            tot_v += c.value_loss_weight * v_loss.item()
            tot_p += c.policy_loss_weight * p_loss.item()
            for k in range(1, c.unroll_steps + 1):
                j = start + k - 1
                a = trajectory["actions"][j] if j < T else A - 1          # pass past the end
                latent, reward, value, logits = recurrent_inference_torch(
                    net, latent, torch.tensor([a], dtype=torch.long, device=dev))
                tr = trajectory["rewards"][j] if j < len(trajectory["rewards"]) else 0.0
                tr = torch.tensor(tr, dtype=torch.float32, device=dev)
                tv = torch.tensor(self.compute_target_value(trajectory, start + k), dtype=torch.float32, device=dev)
                tp = torch.tensor(self._policy_target(trajectory, start + k), dtype=torch.float32, device=dev)
                r_loss = F.mse_loss(reward.squeeze(), tr)
                v_loss = self._value_loss(value.squeeze(), tv)
                p_loss = F.kl_div(F.log_softmax(logits, dim=1), tp, reduction="batchmean")
                step_loss = step_loss + (c.reward_loss_weight * r_loss + c.value_loss_weight * v_loss
                                         + c.policy_loss_weight * p_loss)
                tot_r += c.reward_loss_weight * r_loss.item()
                tot_v += c.value_loss_weight * v_loss.item()
                tot_p += c.policy_loss_weight * p_loss.item()
            step_loss.backward()
            torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=c.max_grad_norm)
            self.optimizer.step()
            per.append(step_loss.item())
            loss_total += per[-1]
        n = len(batch)
        self.last_per_sample = np.asarray(per, dtype=np.float32) if c.sample_priorities else None
        self.last = dict(training_loss=loss_total / n, value_loss=tot_v / n, policy_loss=tot_p / n,
                         reward_loss=tot_r / n, lr=self.optimizer.param_groups[0]["lr"])
        return loss_total / n

    def _train_device(self, replay, batch_size):
        """The batched step on a ``DeviceReplay``: indices drawn on the host
        (main.py's np.random sequence), targets assembled on the device."""
        if self.mode != "batched":
            raise ValueError("a DeviceReplay trains in mode='batched' only: mode='reference' is main.py's "
                             "per-trajectory step over host trajectories (use PrioritizedReplayBuffer)")
        if len(replay) < batch_size:
            return None
        if self.config.device_sampling:
            return self._train_device_sampled(replay, batch_size)
        indices = replay.sample_indices(batch_size)
        starts = [self.start_index(replay.lengths[i]) for i in indices]
        syms = [self.symmetry_index() for _ in indices] if self.config.symmetries else None
        # one check and one upload of the samples for every assembly of the step
        items, K = replay.items(indices, starts, syms), self.config.unroll_steps
        own = replay.ownership_from(items, K) if self.ownership_head is not None else None
        cons = replay.window_obs_from(items, K) if self.consistency_head is not None else None
        avg = self._unroll_step(*self._targets_from(replay, items), device_totals=True, ownership=own,
                                consistency=cons)
        replay.update_priorities(indices, self._priorities(avg, len(indices)))
        self._scheduler_step()
        return avg

    def _train_device_sampled(self, replay, batch_size):
        """``_train_device`` with the store's device ledger: the sample, the
        targets, the step and the priority update are queued on the stream
        without the host seeing an index or a loss; the one copy of the totals
        is the step's only synchronisation of its own (none with
        ``deferred_stats``).  The bootstrap values' ``initial_inference`` still
        reloads the engine's weights through the host after every optimizer
        step, with one blocking copy per tensor, unless ``device_weights`` is
        set: only then is a ``deferred_stats`` step free of synchronisation.

        Every step is draw -> assemble (``sample`` or ``sample_positions``, then
        ``_targets_from``); with ``reanalyse_sample``, ``reanalyser.refresh()``
        and ``reanalyse_sample`` run between the two (on the steps with
        ``sample_step % reanalyse_every == 0``):
        the policy rows the batch is about to read are searched under the
        current weights, in the store, before the targets are assembled.  The
        refresh goes through the host (one blocking copy per tensor) without
        ``device_weights`` and is a device copy with it; the searches and the
        assembly never synchronise.

        With ``value_target="search"`` the assembly writes ``t_val`` itself from
        the stored root values (``batch_values_from``; with
        ``reanalyse_sample``: after ``reanalyse_sample(td_steps=...)``, which also
        searches the rows the value targets read):
        no bootstrap rows, no ``initial_inference``, no ``finish_values``, and
        so no weight reload on the step's own account."""
        c, td = self.config, self.td_steps
        draw = dict(seed=self.sample_seed, step=self.sample_step, symmetries=c.symmetries, beta=c.importance_beta)
        sample = replay.sample
        if c.position_priorities:
            # (a no-op after the first step; the store refuses other parameters than it was enabled with)
            replay.enable_position_priorities(td or c.unroll_steps, c.discount, alpha=c.priority_alpha,
                                              floor=c.priority_floor or None)
            sample = replay.sample_positions
        s = sample(batch_size, **draw)
        if c.reanalyse_sample and self.sample_step % c.reanalyse_every == 0:
            self.reanalyser.refresh()
            self.last_searched_device = replay.reanalyse_sample(self.reanalyser, s, c.unroll_steps, td_steps=td)
        self.sample_step += 1
        obs0, acts, t_val, t_rew, t_pol = self._targets_from(replay, s)
        self.last_t_val_device = t_val
        # the ownership targets of the same items: one more small launch, nothing on the host
        own = replay.ownership_from(s, c.unroll_steps) if self.ownership_head is not None else None
        # the real boards of the same items' windows (the consistency loss's targets): one more small launch
        cons = replay.window_obs_from(s, c.unroll_steps) if self.consistency_head is not None else None
        avg = self._unroll_step(obs0, acts, t_val, t_rew, t_pol, device_totals=True, device_sample=(replay, s),
                                ownership=own, consistency=cons)
        self._scheduler_step()
        return avg

    def _finish_device(self, device_sample, per, totals, B, lr, value=None, t_val=None, own_total=None,
                       cons_total=None):
        """The tail of a device-sampled step: the priorities from ``per`` (f32
        [B], unweighted) or the batch mean -- with ``position_priorities`` the
        sampled windows' position weights from ``value`` and ``t_val`` (f32
        [B, K+1]: the raw value outputs and targets) instead -- and the totals
        (f64 [4], unweighted; ``own_total`` and ``cons_total`` f64 [1]: the ownership and the consistency
        loss's, apart) left on the device for ``read_stats``."""
        replay, sample = device_sample
        c = self.config
        if c.position_priorities:
            replay.update_position_priorities(sample, value, t_val)
        elif c.sample_priorities:
            replay.update_device_priorities(sample, per, c.priority_alpha)
        else:
            replay.update_device_priorities(sample, alpha=c.priority_alpha, mean=totals[:1] / B)
        self.last_per_sample = None
        self.last_per_sample_device = per if c.sample_priorities else None
        self._pending = (totals, B, lr, own_total, cons_total)
        if c.deferred_stats:
            self.last = {}
            return totals[0] / B
        return self.read_stats()["training_loss"]

    def read_stats(self):
        """``last`` of the latest step; with ``deferred_stats`` this is where the
        totals are copied from the device (one synchronising copy)."""
        if self._pending is not None:
            totals, B, lr, own_total, cons_total = self._pending
            self._pending = None
            aux = [t for t in (own_total, cons_total) if t is not None]
            if aux:                                     # (still one copy)
                totals = torch.cat([totals, *aux])
            total, tot_v, tot_p, tot_r, *aux = totals.tolist()
            self.last = dict(training_loss=total / B, value_loss=tot_v / B, policy_loss=tot_p / B,
                             reward_loss=tot_r / B, lr=lr)
            if own_total is not None:
                self.last["ownership_loss"] = aux.pop(0) / B
            if cons_total is not None:
                self.last["consistency_loss"] = aux.pop(0) / B
        return self.last

    def device_targets(self, replay, indices, starts, symmetries=None):
        """``host_targets`` from a ``DeviceReplay``: one batch-assembly launch,
        one ``initial_inference`` over all B (K+1) bootstrap rows (a workgroup
        per row, so a row's value does not depend on its neighbours), one
        finishing launch.  Nothing comes back to the host."""
        return self._targets_from(replay, replay.items(indices, starts, symmetries))

    def _targets_from(self, replay, sample):
        """(obs0, acts, t_val, t_rew, t_pol) for a sample's device items: the
        assembly and, for network value targets, the bootstrap inference and
        the finishing launch."""
        from .replay import finish_values
        c, N = self.config, self.net.board_size
        if self.td_steps is not None:       # value_target="search": one launch, no inference, nothing to finish
            bt = replay.batch_values_from(sample, c.unroll_steps, self.td_steps, c.discount)
            return bt["obs0"], bt["acts"], bt["t_val"], bt["t_rew"], bt["t_pol"]
        bt = replay.batch_from(sample, c.unroll_steps, c.discount)
        with torch.no_grad():
            _, v, _ = self.net.initial_inference(bt["boot_obs"].view(-1, 6, N, N))
        t_val = finish_values(bt["val"], bt["factor"], bt["has_boot"], v)
        return bt["obs0"], bt["acts"], t_val, bt["t_rew"], bt["t_pol"]

    def host_targets(self, batch, starts):
        """``batch_targets`` as the float32 / int64 tensors the unroll reads,
        on the trainer's device: (obs0, acts, t_val, t_rew, t_pol)."""
        dev = self.device
        obs0, acts, t_val, t_rew, t_pol = self.batch_targets(batch, starts)
        f32 = lambda x: torch.as_tensor(x, dtype=torch.float32, device=dev)
        t_val, t_rew, t_pol = f32(t_val), f32(t_rew), f32(t_pol)
        return f32(obs0), torch.as_tensor(acts, device=dev), t_val, t_rew, t_pol

    def _train_batched(self, batch):
        starts = [self.start_index(len(t["actions"])) for t in batch]
        return self._unroll_step(*self.host_targets(batch, starts))

    def batch_targets(self, batch, starts):
        """The host target builder: for trajectories ``batch`` from moves
        ``starts``, numpy arrays (obs0 f64 [B,6,N,N], acts i64 [B,K], t_val
        f64 [B,K+1], t_rew f64 [B,K], t_pol f64 [B,K+1,A]) -- rewards,
        policies, actions and every value target, whose bootstrap values come
        from one batched ``initial_inference`` under the current weights."""
        c, dev, net = self.config, self.device, self.net
        A, K, B = self.action_size, c.unroll_steps, len(batch)
        # targets: rewards, policies and the discounted part of every value
        # target; all bootstrap positions in one inference
        t_val = np.zeros((B, K + 1))
        t_rew = np.zeros((B, K))
        t_pol = np.zeros((B, K + 1, A))
        acts = np.full((B, K), A - 1, dtype=np.int64)
        boot_obs, boot_at = [], []
        search = self.td_steps is not None
        for b, (tr, s) in enumerate(zip(batch, starts)):
            T = len(tr["actions"])
            if search and (tr.get("root_values") is None or len(tr["root_values"]) != T):
                raise ValueError(f"value_target='search' reads trajectory['root_values'] (one per move, as Reanalyser "
                                 f"and DeviceReplay.export give them); trajectory {b} has "
                                 f"{'none' if tr.get('root_values') is None else len(tr['root_values'])} for {T} moves")
            for k in range(K + 1):
                if search:
                    t_val[b, k] = self._search_value(tr, s + k)
                else:
                    val, factor, boot = self._discounted(tr, s + k)
                    t_val[b, k] = val
                    if boot is not None:
                        boot_obs.append(np.asarray(tr["observations"][boot]))
                        boot_at.append((b, k, factor))
                t_pol[b, k] = self._policy_target(tr, s + k)
            for k in range(K):
                j = s + k
                if j < T:
                    acts[b, k] = tr["actions"][j]
                t_rew[b, k] = tr["rewards"][j] if j < len(tr["rewards"]) else 0.0
        if boot_obs:
            obs = torch.as_tensor(np.stack(boot_obs), dtype=torch.float32, device=dev)
            with torch.no_grad():
                if dev.type == "cuda":
                    _, v, _ = net.initial_inference(obs)      # HIP engine, one launch
                else:
                    _, v, _ = initial_inference_torch(net, obs)
            v = v.squeeze(1).double().cpu().numpy()
            for (b, k, factor), vb in zip(boot_at, v):
                t_val[b, k] += factor * float(np.float32(vb))
        obs0 = np.stack([np.asarray(tr["observations"][s]) for tr, s in zip(batch, starts)])
        return obs0, acts, t_val, t_rew, t_pol

    def _unroll_step(self, obs0, acts, t_val, t_rew, t_pol, device_totals=False, device_sample=None, ownership=None,
                     consistency=None):
        """One optimizer step on the summed losses of B samples unrolled K
        steps, from targets on the device (obs0 f32 [B,6,N,N], acts i64 [B,K],
        t_val f32 [B,K+1], t_rew f32 [B,K], t_pol f32 [B,K+1,A]); returns the
        mean loss.  The per-term totals of ``self.last`` are read back term by
        term (the host path), or with ``device_totals`` summed on the device in
        float64 -- the same sums -- and read with the loss in one copy, the
        step's only synchronisation.  ``TrainConfig.fused_loss`` takes the
        loss, the totals and the heads' gradients from ``mzgo.unroll_loss``
        instead (``_unroll_step_fused``); ``sample_priorities`` keeps the
        per-sample losses in ``last_per_sample`` (in that same copy).  With
        ``device_sample`` = (the store, what its ``sample`` returned) the
        losses and totals stay on the device (``_finish_device``) and the loss
        is weighted by the sample's importance weights when
        ``importance_beta`` > 0."""
        c, net = self.config, self.net
        B, K = acts.shape
        if c.fused_loss:
            return self._unroll_step_fused(obs0, acts, t_val, t_rew, t_pol, device_sample, ownership, consistency)
        tot = (lambda x: x.detach().sum().double()) if device_totals else (lambda x: x.sum().item())
        self.optimizer.zero_grad()
        steps = self._head_outputs(obs0, acts)
        _, value, logits = next(steps)
        kl = lambda lg, tp: F.kl_div(F.log_softmax(lg, dim=1), tp, reduction="none").sum(dim=1)
        v_l = c.value_loss_weight * self._value_loss(value, t_val[:, 0])
        p_l = c.policy_loss_weight * kl(logits, t_pol[:, 0])
        per = v_l + p_l
        tot_v, tot_p, tot_r = tot(v_l), tot(p_l), 0.0
        values = [value.detach()] if c.position_priorities else None     # the raw value outputs of the K + 1 steps
        for k in range(1, K + 1):
            reward, value, logits = next(steps)
            if values is not None:
                values.append(value.detach())
            r_l = c.reward_loss_weight * F.mse_loss(reward, t_rew[:, k - 1], reduction="none")
            v_l = c.value_loss_weight * self._value_loss(value, t_val[:, k])
            p_l = c.policy_loss_weight * kl(logits, t_pol[:, k])
            per = per + r_l + v_l + p_l
            tot_r += tot(r_l)
            tot_v += tot(v_l)
            tot_p += tot(p_l)
        loss = per.sum() if not self._weighted(device_sample) else (per * device_sample[1]["weight"]).sum()
        loss.backward()
        lr = self._optimizer_step()
        self.last_per_sample = None
        if device_sample is not None:
            d = per.detach()
            totals = torch.stack([d.sum().double(), tot_v, tot_p, tot_r])
            value = torch.stack(values, dim=1) if values is not None else None
            return self._finish_device(device_sample, d, totals, B, lr, value, t_val)
        if device_totals and c.sample_priorities:
            back = torch.cat([torch.stack([loss.detach().double(), tot_v, tot_p, tot_r]),
                              per.detach().double()]).tolist()
            total, tot_v, tot_p, tot_r = back[:4]
            self.last_per_sample = np.asarray(back[4:], dtype=np.float32)
        elif device_totals:
            total, tot_v, tot_p, tot_r = torch.stack([loss.detach().double(), tot_v, tot_p, tot_r]).tolist()
        else:
            total = loss.item()
            if c.sample_priorities:
                self.last_per_sample = per.detach().cpu().numpy()
        self.last = dict(training_loss=total / B, value_loss=tot_v / B, policy_loss=tot_p / B,
                         reward_loss=tot_r / B, lr=lr)
        return total / B

    def _head_outputs(self, obs0, acts):
        """(reward [B] (None at k = 0), value [B], logits [B, A]) of the unroll's
        steps k = 0..K, one at a time: from the per-step graph (torch's ops, or
        ``hip_forward``'s Functions), or with ``fused_unroll`` as slices of
        ``mzgo.unroll``'s stacked outputs (the whole unroll runs before the
        first is yielded)."""
        net = self.net
        K = acts.shape[1]
        if self.config.fused_unroll:
            from .unroll import unroll
            logits, value, reward = unroll(net, obs0, acts, self.config.unroll_precision)
            for k in range(K + 1):
                yield (reward[k - 1] if k else None), value[k], logits[k]
            return
        fwd0, fwd = ((initial_inference_hip, recurrent_inference_hip) if self.hip_forward
                     else (initial_inference_torch, recurrent_inference_torch))
        latent, value, logits = fwd0(net, obs0)
        yield None, value.squeeze(1), logits
        for k in range(1, K + 1):
            latent, reward, value, logits = fwd(net, latent, acts[:, k - 1])
            yield reward.squeeze(1), value.squeeze(1), logits

    def _weighted(self, device_sample):
        """Whether the step's loss is the importance-weighted sum (the
        priorities and the reported totals stay unweighted)."""
        return device_sample is not None and self.config.importance_beta > 0

    def _unroll_step_fused(self, obs0, acts, t_val, t_rew, t_pol, device_sample=None, ownership=None,
                           consistency=None):
        """``_unroll_step`` with the loss on the HIP kernel: the K + 1 steps'
        head outputs are collected and stacked once (``fused_unroll``:
        they come stacked from ``mzgo.unroll``), ``mzgo.unroll_loss`` gives
        ``per`` and the f64 totals in one call, and autograd enters the network
        through its saved head gradients.  One copy brings the totals (and,
        with ``sample_priorities``, the per-sample losses) back.

        With ``ownership`` = (t_own, own_mask) (``ownership_loss_weight`` > 0;
        ``fused_unroll``) the unroll also returns its latents, the ownership
        head's per-sample losses (``mzgo.ownership_loss``) are added to ``per``
        under the same importance weights, and the gradient that reaches the
        latents goes back into the unroll's backward.  The priorities,
        ``training_loss`` and the three totals stay those of ``per`` without
        ownership; the ownership total is ``last["ownership_loss"]``.

        With ``consistency`` = (obs, mask) (``consistency_loss_weight`` > 0:
        the real boards of the windows' steps 1..K, ``DeviceReplay.window_obs``)
        ``mzgo.encode`` gives the boards' latents under the current weights,
        and ``mzgo.consistency_loss`` on the unroll's latents joins ``per`` in
        the same way; its total is ``last["consistency_loss"]``.  Both
        auxiliary losses hang on the one ``latents`` output: autograd adds
        their gradients before the unroll's backward."""
        from .loss import unroll_loss
        c, net = self.config, self.net
        B, K = acts.shape
        self.optimizer.zero_grad()
        per_own = own_total = per_cons = cons_total = None
        if ownership is not None or consistency is not None:
            from .unroll import unroll
            if consistency is not None:
                from .consistency import consistency_loss
                from .unroll import encode
                obs_k, cons_mask = consistency
                N = net.board_size
                targets = encode(net, obs_k.view(K * B, 6, N, N)).view(K, B, net.latent_dim, N, N)
            lgs, vals, rews, latents = unroll(net, obs0, acts, c.unroll_precision, return_latents=True)
            if ownership is not None:
                from .ownership import ownership_loss
                per_own, own_total = ownership_loss(latents, self.ownership_head, *ownership,
                                                    weight=c.ownership_loss_weight)
            if consistency is not None:
                per_cons, cons_total = consistency_loss(latents, targets, cons_mask, self.consistency_head,
                                                        weight=c.consistency_loss_weight)
        elif c.fused_unroll:
            from .unroll import unroll
            lgs, vals, rews = unroll(net, obs0, acts, c.unroll_precision)   # stacked as they come
        else:
            lgs, vals, rews = [], [], []
            for reward, value, logits in self._head_outputs(obs0, acts):
                lgs.append(logits)
                vals.append(value)
                if reward is not None:
                    rews.append(reward)
            lgs, vals, rews = torch.stack(lgs), torch.stack(vals), torch.stack(rews) if rews else None
        per, totals = unroll_loss(lgs, vals, rews, t_pol, t_val, t_rew, value_loss_weight=c.value_loss_weight,
                                  policy_loss_weight=c.policy_loss_weight, reward_loss_weight=c.reward_loss_weight,
                                  value_transform=c.use_value_transform)
        trained = per if per_own is None else per + per_own
        if per_cons is not None:
            trained = trained + per_cons
        loss = trained.sum() if not self._weighted(device_sample) else (trained * device_sample[1]["weight"]).sum()
        loss.backward()
        lr = self._optimizer_step()
        self.last_per_sample = None
        if device_sample is not None:
            value = vals.detach().t().contiguous() if c.position_priorities else None    # [K+1, B] -> [B, K+1]
            return self._finish_device(device_sample, per.detach(), totals, B, lr, value, t_val, own_total, cons_total)
        aux = [t for t in (own_total, cons_total) if t is not None]
        if aux:                                         # (still one copy; the per-sample losses follow the totals)
            totals = torch.cat([totals, *aux])
        n = totals.numel()
        if c.sample_priorities:
            back = torch.cat([totals, per.detach().double()]).tolist()
            self.last_per_sample = np.asarray(back[n:], dtype=np.float32)
        else:
            back = totals.tolist()
        total, tot_v, tot_p, tot_r = back[:4]
        self.last = dict(training_loss=total / B, value_loss=tot_v / B, policy_loss=tot_p / B,
                         reward_loss=tot_r / B, lr=lr)
        if own_total is not None:
            self.last["ownership_loss"] = back[4] / B
        if cons_total is not None:
            self.last["consistency_loss"] = back[n - 1] / B
        return total / B
