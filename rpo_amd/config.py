"""Static description of one RPO train-step workload.

The reference hard-codes the ViT-B/16 numbers inside ``trainers/rpo.py``
(``d_v = 768`` at :52, ``14 * 14`` patches at :154, 8 text heads at :142,
embed dim 512 at :185, context length 77 at :141).  Here they are fields so the
same kernels serve ViT-L/14 (BASELINE.json configs[3]) as well.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

# Oxford-Pets base split: first ceil(37/2)=19 class names in label order
# (datasets/oxford_pets.py:55-72 lower-cases "<breed>_<n>.jpg" -> breed;
#  :161-167 keeps the first half).  RPO keeps the underscores
# (trainers/rpo.py:133 replaces only the template's "_").
OXFORD_PETS_BASE_CLASSES = (
    "abyssinian", "american_bulldog", "american_pit_bull_terrier", "basset_hound",
    "beagle", "bengal", "birman", "bombay", "boxer", "british_shorthair",
    "chihuahua", "egyptian_mau", "english_cocker_spaniel", "english_setter",
    "german_shorthaired", "great_pyrenees", "havanese", "japanese_chin", "keeshond",
)
PROMPT_TEMPLATE = "a photo of a _."

SOT_TOKEN = 49406
EOT_TOKEN = 49407
HEAD_DIM = 64


@dataclass(frozen=True)
class RPOConfig:
    """Dimensions of the two towers plus the few-shot step parameters."""

    name: str = "ViT-B/16"
    # image tower
    image_size: int = 224
    patch: int = 16
    d_v: int = 768
    layers_v: int = 12
    # text tower
    d_t: int = 512
    layers_t: int = 12
    context: int = 77
    vocab: int = 49408
    # joint space
    embed: int = 512
    # RPO
    K: int = 24
    n_cls: int = 19
    # image tower kind: "vit", or "rn" for CLIP's ModifiedResNet (clip/model.py:94-152).  For "rn", d_v is the ResNet
    # feature width (rn_width * 32, the attention pool's embed dim), patch = 32 (the tower's total stride: grid is the
    # attention pool's grid, n_frozen its H*W + 1 tokens, heads_v its heads) and layers_v = 0
    vision: str = "vit"
    rn_layers: tuple = ()
    rn_width: int = 0

    @property
    def is_rn(self) -> bool:
        return self.vision == "rn"

    @property
    def heads_v(self) -> int:
        return self.d_v // HEAD_DIM

    @property
    def heads_t(self) -> int:
        return self.d_t // HEAD_DIM

    @property
    def grid(self) -> int:
        return self.image_size // self.patch

    @property
    def n_patches(self) -> int:
        return self.grid * self.grid

    @property
    def n_frozen(self) -> int:
        """CLS + patches: the tokens every query may read (trainers/rpo.py:154)."""
        return 1 + self.n_patches

    @property
    def seq_v(self) -> int:
        return self.n_frozen + self.K

    @property
    def patch_dim(self) -> int:
        return 3 * self.patch * self.patch

    def with_(self, **kw) -> "RPOConfig":
        return replace(self, **kw)


def vit_b16(**kw) -> RPOConfig:
    return RPOConfig(**kw)


def vit_l14(**kw) -> RPOConfig:
    """ViT-L/14: d=1024, 24 layers, 16 heads, patch 14 (257 frozen tokens);
    text width 768 / 12 heads, embed 768.  The reference cannot run it
    (SURVEY.md finding 7); only the oracle restatement pins it."""
    base = dict(name="ViT-L/14", patch=14, d_v=1024, layers_v=24, d_t=768,
                layers_t=12, embed=768)
    base.update(kw)
    return RPOConfig(**base)


def vit_b32(**kw) -> RPOConfig:
    """ViT-B/32 (clip/clip.py:34; configs/trainers/CoOp/vit_b32.yaml): ViT-B/16's widths on a 7 x 7 grid -- 50 frozen
    tokens, patch rows of 3 * 32 * 32 = 3072."""
    base = dict(name="ViT-B/32", patch=32)
    base.update(kw)
    return RPOConfig(**base)


def vit_l14_336(**kw) -> RPOConfig:
    """ViT-L/14@336px (clip/clip.py:38): ViT-L/14's widths on a 24 x 24 grid -- 577 frozen tokens, which the image
    tower's attention walks in chunks (ATTN_LDS_TOKENS)."""
    return vit_l14(**{**dict(name="ViT-L/14@336px", image_size=336), **kw})


# Frozen tokens of an image whose K / V the attention kernels hold in LDS at once (include/rpo_amd.h).  Above it
# rpo_attn_readonly_fwd / _fwd_rows / _bwd walk the keys in chunks (up to ATTN_MAX_TOKENS); rpo_attn_prompt_fwd (the
# shared-frozen-rows evaluation, FrozenImageKV) and rpo_attn_readonly_bwd_proj (the fused d out-proj) do not.
ATTN_LDS_TOKENS = 288
ATTN_MAX_TOKENS = 1025


def refuse_long_grid(cfg: RPOConfig, what: str) -> None:
    """The paths built on rpo_attn_prompt_fwd stop at its 288-token limit: refused where they are set up, not mid-pass."""
    if not cfg.is_rn and cfg.n_frozen > ATTN_LDS_TOKENS:
        raise NotImplementedError(f"{what}: {cfg.name} has {cfg.n_frozen} frozen tokens per image, above the "
                                  f"{ATTN_LDS_TOKENS}-token limit of rpo_attn_prompt_fwd (the prompt-row pass on shared or "
                                  "cached frozen K / V); evaluate through the whole image pass instead")


def rn_clip(layers=(3, 4, 6, 3), width: int = 64, embed: int = 1024, image_size: int = 224, **kw) -> RPOConfig:
    """CLIP ResNet (clip/model.py:94-152, built by :412-419): RN50 = (3, 4, 6, 3) / width 64 / embed 1024, RN101 =
    (3, 4, 23, 3) / 64 / 512; text tower as ViT-B/16's (512 wide, 12 layers) unless given."""
    name = RN_NAMES.get((tuple(layers), width), f"RN{tuple(layers)}x{width}")
    base = dict(name=name, vision="rn", rn_layers=tuple(int(l) for l in layers), rn_width=width, d_v=width * 32, patch=32,
                layers_v=0, image_size=image_size, embed=embed)
    base.update(kw)
    return RPOConfig(**base)


# (blocks per stage, stem width) -> name (clip/clip.py:30-34 lists these five ResNets)
RN_NAMES = {((3, 4, 6, 3), 64): "RN50", ((3, 4, 23, 3), 64): "RN101", ((4, 6, 10, 6), 80): "RN50x4",
            ((6, 8, 18, 8), 96): "RN50x16", ((3, 15, 36, 10), 128): "RN50x64"}


def rn_plan(cfg: RPOConfig):
    """The convolutions of the ResNet tower in execution order (clip/model.py:99-152): one dict per Bottleneck with its
    input size / channels, planes, stride and whether it has a downsample branch."""
    w, H = cfg.rn_width, cfg.image_size // 4
    inpl, blocks = w, []
    for s, n in enumerate(cfg.rn_layers):
        planes = w * (1 << s)
        for i in range(n):
            stride = 2 if (s > 0 and i == 0) else 1
            blocks.append(dict(name=f"layer{s + 1}.{i}", H=H, cin=inpl, planes=planes, stride=stride,
                               down=stride > 1 or inpl != planes * 4))
            inpl = planes * 4
            H //= stride
    return blocks


def flops_rn_image(cfg: RPOConfig) -> float:
    """Algorithmic forward FLOPs per image of the ResNet tower (2 per MAC): the three stem convolutions, every Bottleneck's
    three convolutions and downsample, and the attention pool (K / V of all H*W + 1 tokens, q of token 0, its scores and
    weighted sum, c_proj).  Pools, BatchNorm (folded) and ReLU are not counted."""
    w, R = cfg.rn_width, cfg.image_size
    h1 = R // 2
    f = 2.0 * h1 * h1 * 27 * (w // 2) + 2.0 * h1 * h1 * 9 * (w // 2) * (w // 2) + 2.0 * h1 * h1 * 9 * (w // 2) * w
    for b in rn_plan(cfg):
        H, Ho, cin, p = b["H"], b["H"] // b["stride"], b["cin"], b["planes"]
        f += 2.0 * H * H * cin * p + 2.0 * H * H * 9 * p * p + 2.0 * Ho * Ho * p * 4 * p
        if b["down"]:
            f += 2.0 * Ho * Ho * cin * 4 * p
    C, T = cfg.d_v, cfg.n_frozen
    f += 2.0 * T * C * 2 * C + 2.0 * C * C + 2.0 * 2 * T * C + 2.0 * C * cfg.embed
    return f


# ---------------------------------------------------------------------------
# Algorithmic FLOPs: mask-aware minimal work, 2 FLOP per
# MAC.  Used by bench.py for roofline.achieved; cannot be inflated by wasted
# compute because it counts only what the read-only structure requires.
# ---------------------------------------------------------------------------

def flops_image(cfg: RPOConfig) -> tuple[float, float]:
    """(forward, backward) FLOPs per image for the image tower."""
    L, d, N, K, S, e = cfg.layers_v, cfg.d_v, cfg.n_frozen, cfg.K, cfg.seq_v, cfg.embed
    fwd = L * (20 * S * d * d + 4 * N * d * d + 4 * S * N * d) \
        + 2 * (N - 1) * d * cfg.patch_dim + 2 * K * d * e
    bwd = L * (20 * K * d * d + 4 * K * N * d) + 2 * K * d * e
    return float(fwd), float(bwd)


def flops_text(cfg: RPOConfig, len_prompts) -> float:
    """FLOPs per step for the K prompt rows of every class (fwd + bwd);
    the frozen rows' K/V are cached once per run and excluded."""
    L, d, K, e = cfg.layers_t, cfg.d_t, cfg.K, cfg.embed
    tot = 0.0
    for lc in len_prompts:
        tot += L * (20 * K * d * d + 4 * K * int(lc) * d)
    tot += len(len_prompts) * 2 * K * d * e
    return 2.0 * tot


def flops_step(cfg: RPOConfig, batch: int, len_prompts) -> float:
    f, b = flops_image(cfg)
    return batch * (f + b) + flops_text(cfg, len_prompts) + batch * 2.0 * cfg.K * cfg.embed * cfg.n_cls


def flops_coop_step(cfg: RPOConfig, batch: int, lens, replicas: int = 1) -> float:
    """Algorithmic FLOPs of one CoOp (replicas = 1) / CoCoOp (replicas = batch) train step, trainers/coop.py:258-281 /
    trainers/cocoop.py:255-275: the plain image tower forward for `batch` images (all N tokens through all blocks; no
    backward -- nothing trainable sits in front of it), and the DENSE text tower forward + backward-to-input for the
    tokens [0, len_c) of every class (causal attention counted as the lower triangle; backward: the dX GEMMs of the four
    linears -- weights frozen -- and 2x the attention's forward), once per replica; projections and head on top."""
    Lv, dv, N, e = cfg.layers_v, cfg.d_v, cfg.n_frozen, cfg.embed
    Lt, dt = cfg.layers_t, cfg.d_t
    img = Lv * (24.0 * N * dv * dv + 4.0 * N * N * dv) + 2.0 * (N - 1) * dv * cfg.patch_dim + 2.0 * dv * e
    T = float(sum(int(l) for l in lens))
    tri = float(sum(int(l) * (int(l) + 1) // 2 for l in lens))
    text = Lt * (48.0 * T * dt * dt + 3.0 * 4.0 * tri * dt) + 2.0 * 2.0 * len(lens) * dt * e
    return batch * img + replicas * text + 4.0 * batch * len(lens) * e


def flops_last_block_dead(cfg: RPOConfig) -> float:
    """FLOPs per image that flops_image (the SURVEY 8d contract figure) counts but the engine does not execute: in the
    LAST image block only the K prompt rows are consumed (ln_post, trainers/rpo.py:210), so the N frozen rows skip
    their q-projection, attention, out-proj and MLP (they still provide K / V)."""
    d, N = cfg.d_v, cfg.n_frozen
    return float(20 * N * d * d + 4 * N * N * d)


def act_dtype_for_prec(prec: str):
    """`TRAINER.RPO.PREC` (configs/trainers/RPO/main_K24.yaml:35, trainers/rpo.py:247-249,278,298-304) -> the
    activation / weight storage dtype of the HIP engine.

    "fp32": exact-f32 MFMA path (the parity mode).  "fp16" (the reference's GPU default: fp16 weights and
    activations, plain SGD, no loss scaling) -> native IEEE half storage: f16 weights / activations on
    v_mfma_f32_32x32x16_f16 with fp32 accumulation.  Unlike the reference's fp16 mode the residual stream, LayerNorm,
    softmax, logits, the prompts, the prompt GRADIENTS and the optimiser state stay fp32, and there is no loss
    scaling.  What IS stored in fp16 in the backward are the A operands of the dX GEMMs (the back-propagated row
    gradients dx / du / dq and the two feature gradients the head writes): entries below 6e-5 go subnormal and below
    6e-8 flush, exactly as in the reference's own fp16 run (plain SGD, no GradScaler: main_K24.yaml:35,
    trainers/rpo.py:278 builds the scaler for "amp" only).  With the synthetic weights the row gradients are
    1e-4 .. 1e-1 and the goldens bound the effect (gradients within 0.6 % of their largest entry); a user whose
    gradients are much smaller should pick torch.bfloat16 (fp32 exponent range) -- no loss scale is applied for them.
    "amp" (fp32 master weights + autocast + GradScaler) maps onto the same storage mode: autocast's fp16 GEMMs with
    fp32 accumulate are what the f16 mode computes and its fp32 master copy of the only trainable state is what the
    engine keeps anyway; of GradScaler only the skipping of a step whose gradient holds Inf / NaN is reproduced --
    `RPO(..., amp=True)` (rpo_sgd_step_guarded) -- its scaling of small gradients is NOT.  bf16 remains available as
    `torch.bfloat16` (same MFMA rate, fp32 exponent range, 8 x the rounding error)."""
    import torch
    table = {"fp32": torch.float32, "fp16": torch.float16, "amp": torch.float16}
    if prec not in table:
        raise ValueError(f"TRAINER.RPO.PREC must be one of {sorted(table)} (trainers/rpo.py:247), got {prec!r}")
    return table[prec]
