"""Record tests/golden/weight_blobs.json: for each of the six kernel sets and
two state dicts (``oracle.weights.deterministic_state_dict(C, A, 3)`` and
``oracle.weights.scaled_state_dict(C, A, 7)``) the float count and the SHA-256
of the bytes that ``Engine.export_weights()`` returns after
``Engine.set_state_dict`` (1 game x 1 simulation, ``compat="fixed"``).  The
device path (``set_parameters_device``) must give the same bytes, or nothing is
written.  tests/test_weights_pack.py and tests/test_gpu_weights_device.py hold
every later packer to these hashes.

Usage (GPU box): python scripts/record_weight_blobs.py [out.json]
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "muzero-go_amd")]

import torch  # noqa: E402

KERNEL_SETS = [(5, 96), (6, 64), (6, 96), (6, 128), (9, 96), (19, 96)]


def state_dicts(C, A):
    from oracle.weights import deterministic_state_dict, scaled_state_dict
    return {"deterministic_3": deterministic_state_dict(C, A, 3), "scaled_7": scaled_state_dict(C, A, 7)}


def main():
    from mzgo.engine import Engine, EngineConfig
    out = os.path.join(ROOT, "tests", "golden", "weight_blobs.json") if len(sys.argv) < 2 else sys.argv[1]
    cases = []
    for N, C in KERNEL_SETS:
        mk = lambda: Engine(EngineConfig(board_size=N, latent_dim=C, num_games=1, num_simulations=1, compat="fixed"))
        host, dev = mk(), mk()
        for name, sd in state_dicts(C, N * N + 1).items():
            sd = {k: torch.from_numpy(v) for k, v in sd.items()}
            host.set_state_dict(sd)
            dev.set_parameters_device({k: v.cuda() for k, v in sd.items()})
            blob = host.export_weights()
            digest = hashlib.sha256(blob.tobytes()).hexdigest()
            assert hashlib.sha256(dev.export_weights().tobytes()).hexdigest() == digest, (N, C, name)
            cases.append({"board_size": N, "latent_dim": C, "state_dict": name, "n_floats": int(blob.size),
                          "sha256": digest})
            print(cases[-1], flush=True)
        host.close()
        dev.close()
    with open(out, "w") as f:
        json.dump({"cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
