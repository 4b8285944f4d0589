"""The CLIP ResNet image tower on the GPU (rpo_amd/csrc/conv.hip, rpo_amd/engine_rn.py).

Op level: every kernel against float64 torch on the CPU, each element bounded by the mode's tolerance times the same sum
over absolute values (helpers.assert_within).  Model level: plain CLIP and CoOp against the reference's own outputs
(tests/golden/ref_rn_*.npz, tools/make_golden_rn.py)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import BF16_GRAD_REL, BF16_LOGIT_ATOL, F16_GRAD_REL, F16_LOGIT_ATOL, TOL_F32, assert_within  # noqa: E402
from rpo_amd import ops, synth  # noqa: E402
from rpo_amd.config import rn_clip  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
# per-element tolerance on sum |a| |w|: operands are rounded to the act dtype before the float64 reference, so this covers
# the fp32 accumulation and the one rounding of the output
TOL = {"f32": 2e-6, "bf16": 8e-3, "f16": 1e-3}
CFGS = {"mini": lambda: rn_clip((1, 1, 1, 1), 64, 1024, layers_t=2), "rn50": lambda: rn_clip(),
        "rn101": lambda: rn_clip((3, 4, 23, 3), 64, 512)}


@functools.lru_cache(maxsize=None)
def _sd(tag):
    return synth.rn_clip_state_dict(CFGS[tag](), seed=0, check=False)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _conv_case(B, H, cin, cout, k, mode, resid, relu, seed=0, tile_config=0):
    dt = DT[mode]
    x = _rand((B, H, H, cin), seed).to(dt)
    w = _rand((cout, k, k, cin), seed + 1, (2.0 / (cin * k * k)) ** 0.5).to(dt)
    bias = _rand((cout,), seed + 2, 0.1).float()
    r = _rand((B, H, H, cout), seed + 3).to(dt) if resid else None
    y = torch.full((B, H, H, cout), float("nan"), dtype=dt, device="cuda")
    ops.conv2d_nhwc(x.cuda(), w.cuda(), bias.cuda(), y, None if r is None else r.cuda(), relu, tile_config)
    x64, w64 = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2)
    ref = F.conv2d(x64, w64, padding=k // 2) + bias.double()[None, :, None, None]
    mag = F.conv2d(x64.abs(), w64.abs(), padding=k // 2) + bias.double().abs()[None, :, None, None]
    if r is not None:
        ref, mag = ref + r.double().permute(0, 3, 1, 2), mag + r.double().abs().permute(0, 3, 1, 2)
    if relu:
        ref = ref.clamp_min(0)
    return y, ref.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)


def _rn50_conv_shapes():
    """Every distinct (H, Cin, Cout, k) the RN50 forward launches at 224 px, from the tower's own plan (config.rn_plan):
    stem convs 2 / 3, each Bottleneck's conv1 / conv2 at the block's input size, conv3 and the downsample after the pool."""
    from rpo_amd.config import rn_plan
    cfg = rn_clip()
    w, out = cfg.rn_width, {(112, 32, 32, 3), (112, 32, 64, 3)}
    for b in rn_plan(cfg):
        H, Ho, p = b["H"], b["H"] // b["stride"], b["planes"]
        out |= {(H, b["cin"], p, 1), (H, p, p, 3), (Ho, p, 4 * p, 1)}
        if b["down"]:
            out.add((Ho, b["cin"], 4 * p, 1))
    return sorted(out, key=lambda s: (-s[0], s[1], s[2], s[3]))


SHAPES = _rn50_conv_shapes()


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("H,cin,cout,k", SHAPES)
def test_conv_shapes_against_float64(H, cin, cout, k, mode):
    for resid, relu in ((False, True), (True, True), (False, False)):
        y, ref, mag = _conv_case(2, H, cin, cout, k, mode, resid, relu)
        assert_within(y, ref, TOL[mode] * mag, f"conv {H}x{H} {cin}->{cout} k{k} {mode} resid={resid} relu={relu}")


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("H,cin,cout,k", [(56, 64, 64, 3), (28, 512, 128, 1), (7, 512, 2048, 1)])
def test_conv_batch100_and_tiles_bit_identical(H, cin, cout, k, mode):
    y, ref, mag = _conv_case(100, H, cin, cout, k, mode, True, True, seed=5)
    assert_within(y, ref, TOL[mode] * mag, f"conv B=100 {H} {cin}->{cout} k{k} {mode}")
    for tc in (1, 2, 3):
        y2, _, _ = _conv_case(100, H, cin, cout, k, mode, True, True, seed=5, tile_config=tc)
        assert torch.equal(y2.view(torch.int16 if mode != "f32" else torch.int32), y.view(torch.int16 if mode != "f32" else torch.int32)), tc


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_stem_pool_and_refusals(mode):
    dt = DT[mode]
    img = _rand((2, 3, 224, 224), 7).float()
    w = _rand((32, 3, 3, 3), 8, 0.2).to(dt)
    bias = _rand((32,), 9, 0.1).float()
    y = torch.empty(2, 112, 112, 32, dtype=dt, device="cuda")
    ops.conv_stem(img.cuda(), w.cuda(), bias.cuda(), y)
    w64 = w.double().permute(0, 3, 1, 2)
    ref = (F.conv2d(img.double(), w64, stride=2, padding=1) + bias.double()[None, :, None, None]).clamp_min(0)
    mag = F.conv2d(img.double().abs(), w64.abs(), stride=2, padding=1) + bias.double().abs()[None, :, None, None]
    assert_within(y, ref.permute(0, 2, 3, 1), TOL[mode] * mag.permute(0, 2, 3, 1), f"stem {mode}")
    for k in (2, 4):
        x = _rand((2, 28, 28, 64), 10).to(dt)
        p = torch.empty(2, 28 // k, 28 // k, 64, dtype=dt, device="cuda")
        ops.avgpool_nhwc(x.cuda(), p, k)
        ref = F.avg_pool2d(x.double().permute(0, 3, 1, 2), k).permute(0, 2, 3, 1)
        assert_within(p, ref, TOL[mode] * F.avg_pool2d(x.double().abs().permute(0, 3, 1, 2), k).permute(0, 2, 3, 1) + 1e-30,
                      f"pool {k} {mode}")
    # refusals: nothing launched, the output untouched
    from rpo_amd import _lib
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    x = torch.zeros(1, 8, 8, 48, dtype=dt, device="cuda")
    out = torch.full((1, 8, 8, 64), 3.0, dtype=dt, device="cuda")
    wb = torch.zeros(64, 3, 3, 48, dtype=dt, device="cuda")
    b = torch.zeros(64, device="cuda")
    code = ops.dtype_code(dt)
    cases = [(48, 64, 3), (64, 64, 5), (64, 48, 1)] if mode != "f32" else [(24, 64, 3), (64, 64, 5), (64, 48, 1)]
    for cin, cout, k in cases:
        assert lib.rpo_conv2d_nhwc(x.data_ptr(), wb.data_ptr(), b.data_ptr(), None, out.data_ptr(), code, 1, 8, 8, cin, cout,
                                   k, 1, 0, s) == -2
    assert lib.rpo_conv2d_nhwc(x.data_ptr() + 2, wb.data_ptr(), b.data_ptr(), None, out.data_ptr(), code, 1, 8, 8, 64, 64,
                               1, 1, 0, s) == -4
    assert lib.rpo_avgpool_nhwc(x.data_ptr(), out.data_ptr(), code, 1, 7, 7, 64, 2, s) == -2
    assert lib.rpo_conv_stem(img.cuda().data_ptr(), wb.data_ptr(), b.data_ptr(), out.data_ptr(), code, 1, 223, 224, 32, 1, s) == -2
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


def _attnpool_ref(x, pos, wq, bq, wkv, bkv, heads):
    B, H, W, C = x.shape
    xs = x.reshape(B, H * W, C)
    tok = torch.cat([xs.mean(1, keepdim=True), xs], 1) + pos[None]
    kv = tok @ wkv.T + bkv
    q = (tok[:, 0] @ wq.T + bq) * (C // heads) ** -0.5
    k, v = kv[..., :C].reshape(B, -1, heads, 64), kv[..., C:].reshape(B, -1, heads, 64)
    s = torch.einsum("bhd,bthd->bht", q.reshape(B, heads, 64), k).softmax(-1)
    return torch.einsum("bht,bthd->bhd", s, v).reshape(B, C)


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("grid,C", [(7, 2048), (9, 2048), (7, 512)])
def test_attention_pool_against_float64(grid, C, mode):
    dt, B, heads = DT[mode], 3, C // 64
    x = _rand((B, grid, grid, C), 20).to(dt)
    pos = _rand((grid * grid + 1, C), 21, C ** -0.5).float()
    wq, wkv = _rand((C, C), 22, C ** -0.5).to(dt), _rand((2 * C, C), 23, C ** -0.5).to(dt)
    bq, bkv = _rand((C,), 24, 0.02).float(), _rand((2 * C,), 25, 0.02).float()
    T = grid * grid + 1
    tok = torch.empty(B, T, C, dtype=dt, device="cuda")
    kv = torch.empty(B * T, 2 * C, dtype=dt, device="cuda")
    q = torch.empty(B, C, device="cuda")
    out = torch.empty(B, C, dtype=dt, device="cuda")
    ops.attnpool_tokens(x.cuda(), pos.cuda(), tok)
    ops.gemm_nt(tok.view(B * T, C), wkv.cuda(), kv, ops.EPI_BIAS, bias=bkv.cuda())
    ops.gemm_nt(tok[:, 0, :], wq.cuda(), q, ops.EPI_BIAS, bias=bq.cuda())
    ops.attnpool_attn(q, kv.view(B, T, 2 * C), out, heads, 64 ** -0.5)
    ref = _attnpool_ref(x.double(), pos.double(), wq.double(), bq.double(), wkv.double(), bkv.double(), heads)
    # the value rows are O(1): bound by the tolerance times the largest |v| path, sum_j p_j |v_j| <= max |v|
    vmax = (x.double().abs().amax() + pos.double().abs().amax()) * wkv.double().abs().sum(1).amax() + bkv.abs().amax()
    tol = {"f32": 1e-5, "bf16": 2e-2, "f16": 4e-3}[mode]
    assert_within(out, ref, tol * vmax * torch.ones_like(ref), f"attnpool {grid}x{grid} C{C} {mode}")
    out2 = out.clone()
    ops.attnpool_attn(q, kv.view(B, T, 2 * C), out, heads, 64 ** -0.5)
    assert torch.equal(out, out2)


# ---- model level ------------------------------------------------------------------------------------------------------

# (logits bound, image-feature relative bound) per backbone and mode: about twice the measured figures (test docstring)
PLAIN_TOL = {"mini": {"f32": (1e-4, 1e-5), "f16": (8e-3, 1.5e-3), "bf16": (0.11, 0.013)},
             "rn50": {"f32": (1e-4, 1e-5), "f16": (1e-2, 1.2e-3), "bf16": (0.08, 0.01)},
             "rn101": {"f32": (2e-4, 2e-5), "f16": (0.14, 0.016), "bf16": (0.36, 0.085)}}


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("tag,B", [("mini", 3), ("rn50", 4), ("rn101", 2)])
def test_zeroshot_rn_matches_reference(tag, B, mode):
    """ZeroshotCLIP.model_inference on an RN state dict (unchanged keys) against the reference's CLIP.forward.  Bounds
    are about twice the measured errors (logits; image features relative to their largest entry):
      reduced RN  f32 1.2e-5 / 1.4e-6   f16 3.5e-3 / 6.4e-4   bf16 0.053 / 6.1e-3
      RN50        f32 1.3e-5 / 1.8e-6   f16 4.2e-3 / 5.7e-4   bf16 0.039 / 4.9e-3
      RN101       f32 8.9e-5 / 7.0e-6   f16 0.071 / 7.7e-3    bf16 0.18 / 0.042
    RN101 is looser than twice the ViT plain-CLIP bounds (1e-2 f16 / 0.12 bf16): its 23 layer-3 blocks grow the synthetic
    activations to RMS ~13 (RN50: ~2) and every block stores its output in the act dtype, so the rounding of the residual
    stream is 6x larger in absolute terms.  f32 stays within the 1e-3 parity bar."""
    from rpo_amd.zeroshot import ZeroshotCLIP
    gold = dict(np.load(os.path.join(GOLD, f"ref_rn_plainclip_{tag}_b{B}.npz")))
    cfg, sd = CFGS[tag](), _sd(tag)
    m = ZeroshotCLIP(sd, device="cuda:0", act_dtype=DT[mode], max_batch=4)
    assert m.cfg == cfg.with_(K=1)
    image = torch.from_numpy(synth.images(cfg, B))
    logits = m.model_inference(image).cpu().numpy()
    feats = m.engine.img_cls_f[:B].cpu().numpy()
    le = np.abs(logits - gold["logits"]).max()
    fe = np.abs(feats - gold["image_features"]).max() / np.abs(gold["image_features"]).max()
    print(f"[rn {tag} {mode}] logits err {le:.3e} image-feature rel {fe:.3e}")
    lt, ft = PLAIN_TOL[tag][mode]
    assert le <= lt and fe <= ft
    assert np.array_equal(m.model_inference(image).cpu().numpy(), logits)


@pytest.mark.parametrize("n_ctx", [4, 16])
@pytest.mark.parametrize("mode", ["f32", "f16", "bf16"])
def test_coop_rn_matches_reference_trainer(n_ctx, mode):
    """CoOp training on a ResNet (trainers/coop.py:258-281): logits, cross-entropy and d loss / d ctx against the
    reference's coop.CustomCLIP + F.cross_entropy + backward on the reduced RN (tests/golden/ref_rn_coop_*.npz), at the
    CoOp tolerances of test_gpu_model.py; embed 1024 runs the dense text backward's projection at that width."""
    from rpo_amd.coop import CoOpCustomCLIP
    gold = dict(np.load(os.path.join(GOLD, f"ref_rn_coop_mini_b3_ctx{n_ctx}.npz")))
    cfg, sd = CFGS["mini"](), _sd("mini")
    m = CoOpCustomCLIP(sd, gold["tokenized_prompts"], n_ctx, "cuda:0", DT[mode], max_batch=4, ctx=gold["ctx"])
    image = torch.from_numpy(synth.images(cfg, 3)).cuda()
    label = torch.from_numpy(gold["label"]).cuda()
    eng = m.engine
    logits = eng.coop_forward_backward(image, label).cpu().numpy()
    loss, g = eng.loss.item(), eng.coop_grad.cpu().numpy()
    le, ll = np.abs(logits - gold["logits"]).max(), abs(loss - float(gold["loss"]))
    gr = float(np.abs(g - gold["ctx_grad"]).max() / np.abs(gold["ctx_grad"]).max())
    print(f"[rn coop ctx{n_ctx} {mode}] logits err {le:.3e} loss err {ll:.3e} ctx_grad rel {gr:.3e}")
    lt, gt = {"f32": (TOL_F32, TOL_F32), "f16": (F16_LOGIT_ATOL, F16_GRAD_REL), "bf16": (BF16_LOGIT_ATOL, BF16_GRAD_REL)}[mode]
    assert le <= lt and ll <= lt and gr <= gt
    eng.coop_forward_backward(image, label)
    assert np.array_equal(eng.coop_grad.cpu().numpy(), g)


def test_rn_tower_batch_sizes_and_graph():
    """One engine, B in {1, 3, 32, 100}, every tower buffer NaN-filled before each call: EVERY image's features (the last
    partial row tiles included) equal its single-image run within 1 % of that image's largest feature (bf16; the conv
    kernels are row-independent, so a gap would be a tail bug, not rounding); a graph-captured forward replays to the
    same bits as the eager one."""
    from rpo_amd.zeroshot import ZeroshotCLIP
    cfg, sd = CFGS["rn50"](), _sd("rn50")
    m = ZeroshotCLIP(sd, device="cuda:0", act_dtype=torch.bfloat16, max_batch=100)
    eng = m.engine
    imgs = torch.from_numpy(synth.images(cfg, 100, seed=77)).cuda()

    def run(x):
        for t in eng.rn_buf + [eng.rn_pool, eng.rn_tok, eng.rn_kv, eng.rn_q, eng.rn_att, eng.img_cls_f]:
            t.fill_(float("nan"))
        eng.rn_forward(x)
        return eng.img_cls_f[:x.shape[0]].clone()
    single = torch.cat([run(imgs[i:i + 1].contiguous()) for i in range(100)])
    for B in (1, 3, 32, 100):
        f = run(imgs[:B].contiguous())
        assert torch.isfinite(f).all()
        err = (f - single[:B]).abs().amax(1) / single[:B].abs().amax(1)
        print(f"[rn batch {B}] worst per-image rel {float(err.max()):.3e}")
        assert bool((err <= 0.01).all()), (B, int(err.argmax()), float(err.max()))
    eager = run(imgs)
    g = torch.cuda.CUDAGraph()
    x = imgs.clone()
    with torch.cuda.graph(g):
        eng.rn_forward(x)
    eng.img_cls_f.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(eng.img_cls_f[:100], eager)


def test_rpo_lp_cocoop_refuse_rn():
    from rpo_amd.coop import CoCoOpCustomCLIP
    from rpo_amd.custom_clip import CustomCLIP
    from rpo_amd.lp import LPCustomCLIP
    from rpo_amd.trainer import RPO
    cfg, sd = CFGS["mini"](), _sd("mini")
    toks = synth.oxford_pets_base_tokens()
    with pytest.raises(NotImplementedError, match="ResNet"):
        CustomCLIP(cfg, sd, toks, "cuda:0", torch.float32, max_batch=2)
    with pytest.raises(NotImplementedError, match="ResNet"):
        RPO(cfg, sd, toks)
    with pytest.raises(NotImplementedError, match="ResNet"):
        LPCustomCLIP(sd, toks, "cuda:0")
    with pytest.raises(NotImplementedError, match="ResNet"):
        CoCoOpCustomCLIP(sd, toks, 4, "cuda:0")


# ---- CoOp on RN50 at configs/trainers/CoOp/rn50.yaml's batch 32, n_ctx 16 ----------------------------------------------

@functools.lru_cache(maxsize=None)
def _coop_gold():
    return dict(np.load(os.path.join(GOLD, "ref_rn_coop_rn50_b32_ctx16.npz")))


def _coop_batch(step, B=32):
    cfg = CFGS["rn50"]()
    return {"img": torch.from_numpy(synth.images(cfg, B, seed=70 + step)),
            "label": torch.from_numpy(synth.labels(cfg, B, seed=80 + step))}


@pytest.mark.parametrize("mode", ["f32", "f16", "bf16"])
def test_coop_rn50_b32_matches_reference_trainer(mode):
    """CoOp's default backbone (RN50, batch 32, n_ctx 16): logits, cross-entropy and d loss / d ctx of the HIP path
    against the reference's coop.CustomCLIP + F.cross_entropy + backward (tests/golden/ref_rn_coop_rn50_b32_ctx16.npz), at
    the CoOp tolerances of test_gpu_model.py."""
    from rpo_amd.coop import CoOpCustomCLIP
    gold = _coop_gold()
    m = CoOpCustomCLIP(_sd("rn50"), gold["tokenized_prompts"], 16, "cuda:0", DT[mode], max_batch=32, ctx=gold["ctx"])
    bt = _coop_batch(0)
    assert np.array_equal(bt["label"].numpy(), gold["label"])
    eng = m.engine
    logits = eng.coop_forward_backward(bt["img"].cuda(), bt["label"].cuda()).cpu().numpy()
    loss, g = eng.loss.item(), eng.coop_grad.cpu().numpy()
    le, ll = np.abs(logits - gold["logits"]).max(), abs(loss - float(gold["loss"]))
    gr = float(np.abs(g - gold["ctx_grad"]).max() / np.abs(gold["ctx_grad"]).max())
    print(f"[rn50 coop b32 {mode}] logits err {le:.3e} loss err {ll:.3e} ctx_grad rel {gr:.3e}")
    lt, gt = {"f32": (TOL_F32, TOL_F32), "f16": (F16_LOGIT_ATOL, F16_GRAD_REL), "bf16": (BF16_LOGIT_ATOL, BF16_GRAD_REL)}[mode]
    assert le <= lt and ll <= lt and gr <= gt


def _coop_trainer(mode, **kw):
    from rpo_amd.coop import CoOp
    from rpo_amd.trainer import OptimConfig
    gold = _coop_gold()
    oc = kw.pop("oc", None) or OptimConfig(lr=float(gold["lr"]), momentum=float(gold["momentum"]),
                                           weight_decay=float(gold["weight_decay"]), warmup_epoch=0,
                                           lr_scheduler="constant")
    return CoOp(_sd("rn50"), gold["tokenized_prompts"], 16, oc, "cuda:0", DT[mode], batch_size=32,
                ctx=gold["ctx"], **kw)


def test_coop_rn50_sgd_trajectory():
    """Three steps of the CoOp trainer (fp32) against the reference's three torch.optim.SGD steps (LR 0.002, momentum 0.9,
    weight decay 5e-4) on the same batches: the context after every step and the losses."""
    gold = _coop_gold()
    tr = _coop_trainer("f32", num_batches=10 ** 9)
    for step in range(3):
        out = tr.forward_backward(_coop_batch(step))
        ctx = tr.model.prompt_learner.ctx.detach().cpu().numpy()
        err = float(np.abs(ctx - gold["traj_ctx"][step]).max())
        print(f"[rn50 coop sgd] step {step + 1}: loss {out['loss']:.6f} (ref {gold['traj_loss'][step]:.6f}) ctx err {err:.2e}")
        assert abs(out["loss"] - float(gold["traj_loss"][step])) <= TOL_F32 and err <= 1e-6


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_coop_rn50_graph_step_matches_eager_across_lr_recapture(mode):
    """use_graph=True (the whole step, RN50 tower on the main stream beside the text tower on the side stream, replayed
    from one graph, recaptured when the LR changes at each epoch of a cosine schedule) leaves the same context bits as
    the eager step (both with amp=True: the guarded SGD step; no batch here has a non-finite gradient)."""
    from rpo_amd.trainer import OptimConfig
    oc = OptimConfig(lr=0.002, max_epoch=4, lr_scheduler="cosine", warmup_epoch=0)
    ea = _coop_trainer(mode, oc=oc, num_batches=2, amp=True)
    gr = _coop_trainer(mode, oc=oc, num_batches=2, use_graph=True, amp=True)
    lrs = []
    for step in range(6):
        bt = _coop_batch(step % 3)
        lrs.append(gr.lr)
        la, lg = ea.forward_backward(bt)["loss"], gr.forward_backward(bt)["loss"]
        assert la == lg, (step, la, lg)
        assert torch.equal(ea.engine.coop_params, gr.engine.coop_params), step
    assert len(set(lrs)) >= 3 and gr.skipped_steps == 0


def test_coop_rn50_checkpoint_round_trip(tmp_path):
    """save_model -> a fresh trainer's resume_model restores context and momentum: its next step equals the original
    trainer's next step bit for bit."""
    tr = _coop_trainer("bf16", num_batches=10 ** 9)
    tr.forward_backward(_coop_batch(0))
    tr.save_model(str(tmp_path), is_best=True)
    tr2 = _coop_trainer("bf16", num_batches=10 ** 9)
    tr2.resume_model(str(tmp_path))
    assert torch.equal(tr2.engine.coop_params, tr.engine.coop_params)
    tr.forward_backward(_coop_batch(1))
    tr2.forward_backward(_coop_batch(1))
    assert torch.equal(tr2.engine.coop_params, tr.engine.coop_params), "resume != continue"
