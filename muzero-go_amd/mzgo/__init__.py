"""mzgo -- MI355X-native MuZero-Go self-play engine (host side).

Drop-in counterparts of the reference's hot path (Sir-Teo/MuZero-Go
self_play.py), all executed by libmzgo.so's HIP kernels:

* ``MuZeroNet``   -- same parameters/state_dict keys; initial/recurrent inference on MFMA
* ``ResMuZeroNet`` -- BASELINE config 5's residual-tower network (bf16 MFMA tower engine)
* ``MCTS``, ``MuZeroAgent`` -- device search (select / expand / backup kernels)
* ``MainMCTS`` -- main.py's MCTS variant (trainer self-play / arena) on the same kernels
* ``GoEnv``       -- GymGo rules as bit-exact integer kernels
* ``SelfPlay``    -- G concurrent games per GPU, one fused kernel step per move; opt-in playout cap
  randomization (``fast_simulations``, ``full_search_prob``; ``playout_budget_host`` is the rule)
* ``SelfPlayEvaluator`` -- main.py's arena (two networks, all games at once)
* ``GameHistory``, ``save_batches`` -- the reference's record / pickle format
* ``Reanalyser``, ``Engine.reanalyse`` -- stored positions searched again under the
  current weights, from one device work queue (fresh policy targets for a trainer)
* ``DeviceReplay`` -- finished games kept in HBM: the trainer's batches (with board
  symmetries) and reanalysis in place, without the games visiting the host -- whole games
  (``reanalyse``) or exactly the rows a drawn sample reads (``reanalyse_sample``,
  ``TrainConfig.reanalyse_sample``; ``window_items_host`` states the rule on the host);
  opt-in search-value targets from the stored root values (``batch_values``,
  ``TrainConfig.value_target="search"``, ``td_steps``; ``value_targets_host`` is the rule);
  opt-in position-level prioritized replay (``enable_position_priorities``, ``sample_positions``,
  ``update_position_priorities``, ``TrainConfig.position_priorities``; ``sample_positions_host``
  and ``position_priorities_host`` are the rules)
* ``unroll_loss`` -- the trainer's value / policy / reward losses of a whole unroll, their
  per-sample sums and the heads' gradients from one kernel (``TrainConfig.fused_loss``)
* ``unroll`` -- the trainer's whole K-step unroll (representation, dynamics chain, the heads of
  every latent) as one autograd node: one HIP forward call, one backward call
  (``TrainConfig.fused_unroll``); ``precision="bf16"`` (``TrainConfig.unroll_precision``) runs the
  dynamics conv's three matrix products on bf16 MFMA with float32 accumulation and float32 master
  weights, and ``bf16_round_host`` is the kernels' rounding on host arrays
* ``OwnershipHead``, ``ownership_loss`` -- the ownership auxiliary target (KataGo's, on the
  unrolled latents): ``unroll(..., return_latents=True)`` hands out the K + 1 latents and takes a
  gradient on them, the head and its loss are two HIP launches each way, and the targets come
  from the store's final boards (``DeviceReplay.ownership``;
  ``TrainConfig.ownership_loss_weight``); ``ownership_host``, ``ownership_targets_host`` and
  ``ownership_loss_host`` are the rules on host arrays
* ``ConsistencyHead``, ``consistency_loss``, ``encode`` -- the latent consistency loss
  (EfficientZero's, in SimSiam's form): the unrolled latents ``s_1..s_K`` are pulled towards the
  representation's latents (``encode``: the representation alone, no gradient) of the real boards
  the store holds for the window (``DeviceReplay.window_obs``), through a head of two 1x1 convs
  on f32 MFMA kernels, two launches each way (``TrainConfig.consistency_loss_weight``);
  ``consistency_loss_host`` is the rule on host arrays
* ``DeviceAdam`` -- the optimizer tail (gradient-norm clip, Adam / AdamW, StepLR) of any float32
  module in one stream-ordered HIP call that refuses and counts a non-finite gradient
  (``TrainConfig.device_optimizer``); ``adam_step_host`` is its host twin on numpy arrays
* ``pack_weights_host`` -- an engine's packed weight blob from a state_dict on the host: the rule
  both weight paths (``Engine.set_state_dict``, ``Engine.set_parameters_device``) run
* ``mzgo.play`` -- play.py's interactive human-vs-agent loop (``python -m mzgo.play weights.pth``)
"""
from ._lib import MzgoError
from .arena import SelfPlayEvaluator
from .engine import Engine, EngineConfig, pack_weights_host, playout_budget_host
from .consistency import ConsistencyHead, consistency_loss, consistency_loss_host
from .env import GoEnv
from .loss import unroll_loss, unroll_loss_host
from .net import MuZeroNet
from .optim import DeviceAdam, adam_step_host, optim_chunk
from .ownership import OwnershipHead, ownership_loss, ownership_loss_host
from .reanalyse import Reanalyser, positions_from_planes, record_ids
from .replay import (DeviceReplay, ownership_host, ownership_targets_host, position_priorities_host, queue_key_gids,
                     sample_positions_host, value_targets_host, window_items_host)
from .resnet import ResMuZeroNet
from .search import MCTS, MainMCTS, MuZeroAgent
from .selfplay import GameHistory, SelfPlay, history_from_device, save_batches
from .unroll import bf16_round_host, encode, unroll, unroll_heads_host
from .weights import deterministic_res_state_dict, deterministic_state_dict

__all__ = ["Engine", "EngineConfig", "GoEnv", "MuZeroNet", "MCTS", "MainMCTS", "MuZeroAgent", "SelfPlay",
           "GameHistory", "history_from_device", "save_batches", "deterministic_state_dict", "SelfPlayEvaluator",
           "ResMuZeroNet", "deterministic_res_state_dict", "MzgoError", "Reanalyser",
           "positions_from_planes", "record_ids", "DeviceReplay", "queue_key_gids", "unroll_loss",
           "unroll_loss_host", "unroll", "unroll_heads_host", "bf16_round_host", "window_items_host", "value_targets_host",
           "sample_positions_host", "position_priorities_host", "DeviceAdam", "adam_step_host", "optim_chunk",
           "playout_budget_host", "OwnershipHead", "ownership_loss", "ownership_loss_host", "ownership_host",
           "ownership_targets_host", "pack_weights_host", "ConsistencyHead", "consistency_loss",
           "consistency_loss_host", "encode"]
