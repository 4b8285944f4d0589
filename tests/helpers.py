"""Shared builders for tests: synthetic workload -> oracle objects."""
import functools
import os

import numpy as np
import torch

from oracle.rpo_oracle import OracleRPO
from rpo_amd import synth
from rpo_amd.config import vit_b16

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Model-level bounds of the storage modes against the reference / the oracle (tests/test_gpu_model.py,
# tests/test_gpu_batch_sizes.py)
TOL_F32 = 1e-3
BF16_LOGIT_ATOL = 0.12         # logits are O(1..8) at scale 100; measured <= 0.06 (printed by the test)
BF16_GRAD_REL = 0.05           # relative to max |grad|; measured 2.0-2.3 %
F16_LOGIT_ATOL = 1e-2          # native IEEE-half storage mode (TRAINER.RPO.PREC = fp16 / amp): 8x finer than bf16
F16_GRAD_REL = 6e-3

# tag -> (depth, K, B, logit_scale)   (must match tools/make_golden.py)
CASES = {
    "d1_k4_b2": (1, 4, 2, np.log(100.0)),
    "d2_k8_b3": (2, 8, 3, np.log(100.0)),
    "d2_k24_b2_init": (2, 24, 2, np.log(1 / 0.07)),
    "d2_k16_b2": (2, 16, 2, np.log(100.0)),
    "d2_k48_b2": (2, 48, 2, np.log(100.0)),
    "d12_k24_b4": (12, 24, 4, np.log(100.0)),
}


def load_golden(tag):
    return dict(np.load(os.path.join(GOLDEN, f"ref_{tag}.npz")))


@functools.lru_cache(maxsize=2)
def workload(tag):
    depth, K, B, ls = CASES[tag]
    cfg = vit_b16(layers_v=depth, layers_t=depth, K=K)
    toks = synth.oxford_pets_base_tokens()
    sd = synth.clip_state_dict(cfg, seed=0, logit_scale=float(ls))
    tp, ip = synth.prompts(cfg, sd, seed=7)
    image = synth.images(cfg, B)
    label = synth.labels(cfg, B)
    return cfg, sd, toks, tp, ip, image, label


def oracle_for(tag):
    cfg, sd, toks, tp, ip, image, label = workload(tag)
    m = OracleRPO(sd, toks, cfg.K, cfg.patch)
    m.set_prompts(tp, ip)
    return m, image, label


# fp32 unit roundoff: the kernels accumulate in fp32 whatever the storage mode
U32 = 2.0 ** -24


def assert_within(got, ref, bound, what, floor=0.0):
    """Scale-aware check: every element of ``got`` is finite and within ``bound + floor`` of ``ref``, where ``bound``
    (same shape, or broadcastable: per row) is a tolerance times the magnitude of the same computation taken over
    absolute values -- so an outlier channel does not widen the budget of the rest of the tensor, which a bound on
    max|err| / max|ref| over the whole tensor would.  Returns the worst err / (bound + floor)."""
    got = got.detach().to(torch.float64).cpu()
    ref = ref.detach().to(torch.float64).cpu()
    lim = torch.broadcast_to(torch.as_tensor(bound, dtype=torch.float64).cpu(), ref.shape) + floor
    bad = ~torch.isfinite(got)
    assert not bad.any(), f"{what}: {int(bad.sum())} NaN / Inf, first at {tuple(bad.nonzero()[0].tolist())}"
    assert torch.isfinite(ref).all() and torch.isfinite(lim).all(), f"{what}: non-finite reference"
    err = (got - ref).abs()
    ratio = err / lim.clamp_min(1e-300)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        i = tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0].tolist())
        raise AssertionError(f"{what}: err {err[i]:.3e} > bound {lim[i]:.3e} at {i} (got {got[i]:.6e}, ref {ref[i]:.6e}; "
                             f"{int((ratio > 1).sum())} of {ratio.numel()} elements over, worst ratio {worst:.2f})")
    return worst
