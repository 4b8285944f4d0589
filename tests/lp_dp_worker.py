"""Worker of tests/test_gpu_lp.py::test_lp_two_ranks_equal_one_rank_global_batch: one rank of a data-parallel LP run
(WORLD_SIZE / RANK / LOCAL_RANK set by the test).  Every rank takes its shard of the same global batches, runs `steps`
optimisation steps and rank 0 saves the layer."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rpo_amd.dist import GradSync  # noqa: E402


def main(out_path: str, global_batch: int, steps: int):
    from test_gpu_lp import lp_workload, DP_OPTIM, DP_SEEDS          # noqa: E402 (tests/ is this script's directory)
    from rpo_amd.lp import LP
    sync = GradSync()
    first, count = sync.shard(global_batch)
    dev = torch.device(f"cuda:{sync.local_rank}")
    torch.cuda.set_device(dev)
    cfg, sd, toks = lp_workload(2)
    tr = LP(sd, toks, DP_OPTIM(), dev, torch.float32, batch_size=count, num_batches=10 ** 9, sync=sync, max_batch=count,
            cfg=cfg)
    from rpo_amd import synth
    for s in range(steps):
        img = synth.images(cfg, global_batch, seed=DP_SEEDS[s][0])[first:first + count]
        lab = synth.labels(cfg, global_batch, seed=DP_SEEDS[s][1])[first:first + count]
        tr.forward_backward({"img": torch.from_numpy(img), "label": torch.from_numpy(lab)})
    if sync.rank == 0:
        np.savez(out_path, params=tr.engine.lp_params.cpu().numpy(), world=sync.world_size)
    sync.barrier()
    sync.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
