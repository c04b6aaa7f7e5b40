#!/usr/bin/env python3
"""Copy the reference's own input files that the CPU tests read into tests/golden/, so that the suite needs no reference checkout:

    python tools/gen_golden_ref_inputs.py <reference checkout>

  ispd18_sample.input.{lef,def,guide}.gz   simulator/testcases/ispd18_sample/  (tests/test_lefdef.py)
  ispd18_test1.input.{lef,def,guide}.gz    ispd/ispd18_test1/                  (tests/test_lefdef.py)
  ref_dqn_routing_state.npz                the shipped DQN checkpoint's state dict (tests/test_agents.py)
  ref_ppo_routing_random_state.npz         the shipped PPO checkpoint's state dict (tests/test_agents.py)

Data only: design inputs gzipped byte for byte, checkpoint tensors as named arrays in the checkpoint's key order."""
import gzip
import os
import shutil
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
DESIGNS = (("simulator/testcases/ispd18_sample", "ispd18_sample.input"), ("ispd/ispd18_test1", "ispd18_test1.input"))
CHECKPOINTS = (("baseline/DQN/results/2023-05-10--11-06-26/DQN_routing.pth", "ref_dqn_routing_state.npz"),
               ("baseline/PPO/results/2023-04-27--05-00-38/PPO_routing_random.pth", "ref_ppo_routing_random_state.npz"))


def main(ref):
    for sub, stem in DESIGNS:
        for ext in ("lef", "def", "guide"):
            src = os.path.join(ref, sub, f"{stem}.{ext}")
            # mtime 0 and no file name in the header: the same input gives the same bytes
            with open(src, "rb") as fi, open(os.path.join(OUT, f"{stem}.{ext}.gz"), "wb") as raw, \
                    gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=raw, mtime=0) as fo:
                shutil.copyfileobj(fi, fo)
    import torch
    for src, name in CHECKPOINTS:
        sd = torch.load(os.path.join(ref, src), map_location="cpu")
        np.savez_compressed(os.path.join(OUT, name), **{k: v.numpy() for k, v in sd.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
