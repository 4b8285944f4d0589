"""CPU-side checks: the C-ABI library loads and exports every symbol the header declares,
the ctypes signatures cover them, LR schedule / config helpers, and the product package never
imports the oracle."""
import ast
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    src = open(os.path.join(ROOT, "include", "rpo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rpo_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from rpo_amd import _lib
    from rpo_amd.build import build_library
    build_library()
    names = _header_functions()
    assert len(names) >= 18
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"librpo_hip.so does not export {n}"
        assert n in _lib.SIGNATURES, f"no ctypes signature for {n}"
    assert sorted(_lib.SIGNATURES) == names
    assert _lib.load().rpo_version() == 8
    assert b"shape" in _lib.load().rpo_error_string(-2)


def test_dynamic_symbol_table_is_the_header_and_nothing_else():
    """-fvisibility=hidden + csrc/exports.map: `nm -D` of the product library lists exactly the functions include/rpo_amd.h
    declares -- no C++-mangled helpers, no kernel handles / host stubs, no toolchain bookkeeping symbols."""
    import subprocess
    from rpo_amd import _lib
    from rpo_amd.build import build_library
    build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert exported == _header_functions(), sorted(set(exported) ^ set(_header_functions()))


def test_integration_md_snippets_use_the_structs_real_field_names():
    """INTEGRATION.md's Level-2 snippet builds a GemmArgs by keyword: every keyword must be a field of the struct (a wrong
    name raises TypeError in ctypes -- round 5 shipped `a_dtype` / `c_dtype`)."""
    from rpo_amd._lib import GemmArgs
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    calls = re.findall(r"GemmArgs\((.*?)\)\n", text, flags=re.S)
    assert calls, "the GemmArgs(...) snippet is gone from INTEGRATION.md"
    fields = {f[0] for f in GemmArgs._fields_}
    for body in calls:
        kws = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*=(?!=)", body)
        assert kws and set(kws) <= fields, sorted(set(kws) - fields)
        GemmArgs(**{k: 0 for k in kws})             # constructs


def test_experiments_live_only_in_the_experimental_library():
    """include/rpo_amd_experimental.h: every entry point it declares is exported by the -DRPO_EXPERIMENTAL build and by
    that build alone -- the product library and the product header carry none of it."""
    from rpo_amd import _lib
    from rpo_amd.build import LIB_EXP, build_library
    build_library()
    build_library(experimental=True)
    src = open(os.path.join(ROOT, "include", "rpo_amd_experimental.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    exp = sorted(set(re.findall(r"\b(rpo_[a-z0-9_]+)\s*\(", src)))
    assert exp and sorted(_lib.EXPERIMENTAL_SIGNATURES) == exp
    assert not set(exp) & set(_header_functions())
    product, experimental = ctypes.CDLL(_lib.LIB_PATH), ctypes.CDLL(LIB_EXP)
    for n in exp:
        assert not hasattr(product, n), f"librpo_hip.so exports the experiment {n}"
        assert hasattr(experimental, n), f"librpo_hip_exp.so does not export {n}"
    for n in _header_functions():
        assert hasattr(experimental, n)


def test_gemm_args_struct_matches_header_field_order():
    from rpo_amd._lib import GemmArgs
    src = open(os.path.join(ROOT, "include", "rpo_amd.h")).read()
    body = src[src.index("typedef struct rpo_gemm_args {"):src.index("} rpo_gemm_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            fields.append(part.strip().split()[-1].lstrip("*"))
    assert fields == [f[0] for f in GemmArgs._fields_]


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from rpo_amd import synth
    from rpo_amd.config import vit_b16
    from rpo_amd.custom_clip import CustomCLIP
    cfg = vit_b16(layers_v=1, layers_t=1, K=4)
    toks = synth.oxford_pets_base_tokens()
    sd = synth.clip_state_dict(cfg, token_rows=np.unique(toks).tolist() + [49407])
    with pytest.raises(RuntimeError, match="no CPU path"):
        CustomCLIP(cfg, sd, toks, "cuda:0")


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "rpo_amd")
    for fn in os.listdir(pkg):
        if not fn.endswith(".py"):
            continue
        tree = ast.parse(open(os.path.join(pkg, fn)).read())
        for node in ast.walk(tree):
            mods = []
            if isinstance(node, ast.Import):
                mods = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                mods = [node.module or ""]
            assert not any(m.split(".")[0] == "oracle" for m in mods), f"{fn} imports the oracle"


class _ConstantWarmup(torch.optim.lr_scheduler.LRScheduler):
    """Dassl's ConstantWarmupScheduler, re-created from its published semantics (Dassl.pytorch is not vendored:
    dassl/optim/lr_scheduler.py `_BaseWarmupScheduler.step` forwards to the successor only once
    last_epoch >= warmup_epoch, else does a plain scheduler step returning the constant LR)."""

    def __init__(self, optimizer, successor, warmup_epoch, cons_lr):
        self.successor, self.warmup_epoch, self.cons_lr = successor, warmup_epoch, cons_lr
        super().__init__(optimizer)

    def get_lr(self):
        if self.last_epoch >= self.warmup_epoch:
            return self.successor.get_last_lr()
        return [self.cons_lr for _ in self.base_lrs]

    def step(self, epoch=None):
        if self.last_epoch >= self.warmup_epoch:
            self.successor.step(epoch)
            self._last_lr = self.successor.get_last_lr()
        else:
            super().step(epoch)


@pytest.mark.parametrize("warmup,max_epoch,lr", [(1, 15, 0.01), (0, 15, 0.01), (3, 10, 0.002)])
def test_lr_schedule_matches_torch_driven_dassl_recreation(warmup, max_epoch, lr):
    """The product's closed form (and the oracle's) against torch's CosineAnnealingLR stepped by the re-created
    Dassl warm-up wrapper, the way `TrainerX.update_lr` steps it once per epoch (trainers/rpo.py:313-314)."""
    import warnings
    from oracle.rpo_oracle import cosine_lr_with_constant_warmup
    from rpo_amd.trainer import OptimConfig, lr_at_epoch
    oc = OptimConfig(lr=lr, max_epoch=max_epoch, warmup_epoch=warmup)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=lr)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        succ = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=max_epoch)
        sched = _ConstantWarmup(opt, succ, warmup, 1e-5) if warmup > 0 else succ
        for ep in range(max_epoch):
            want = opt.param_groups[0]["lr"]
            assert math.isclose(lr_at_epoch(oc, ep), want, rel_tol=1e-9, abs_tol=1e-15), (ep, lr_at_epoch(oc, ep), want)
            assert math.isclose(cosine_lr_with_constant_warmup(lr, ep, max_epoch, warmup, 1e-5), want,
                                rel_tol=1e-9, abs_tol=1e-15)
            opt.step()
            sched.step()


def test_lr_schedule_yaml_values():
    from rpo_amd.trainer import OptimConfig, lr_at_epoch
    oc = OptimConfig()                                      # main_K24.yaml:15-22
    assert lr_at_epoch(oc, 0) == 1e-5
    assert lr_at_epoch(oc, 1) == 0.01                       # the cosine starts when the warm-up ends
    assert math.isclose(lr_at_epoch(oc, 14), 0.5 * 0.01 * (1 + math.cos(math.pi * 13 / 15)))   # 4.32e-4


def test_checkpoint_writer_satisfies_the_reference_reader_contract(tmp_path):
    """trainers/rpo.py:325-357 opens <dir>/prompt_learner/model-best.pth.tar (or model.pth.tar-<epoch>), reads
    checkpoint["state_dict"] / ["epoch"], drops token_prefix / token_suffix and load_state_dict(strict=False)s the
    rest into PromptLearner (parameters text_prompt [K, d_t], img_prompt [K, 768])."""
    from rpo_amd.optim import rows_from_state_dict
    from rpo_amd.trainer import OptimConfig, checkpoint_dict, write_checkpoint
    K, dt, dv = 4, 512, 768
    state = {"text_prompt": torch.randn(K, dt), "img_prompt": torch.randn(K, dv)}
    mom = torch.randn(K * dt + K * dv)
    ck = checkpoint_dict(state, 7, mom, OptimConfig(), 0.005, 12, K * dt, val_result=55.5)
    fn = write_checkpoint(str(tmp_path), ck, 7, is_best=True)
    d = os.path.join(str(tmp_path), "prompt_learner")
    assert sorted(os.listdir(d)) == ["checkpoint", "model-best.pth.tar", "model.pth.tar-7"]
    assert open(os.path.join(d, "checkpoint")).read().strip() == "model.pth.tar-7" and fn.endswith("model.pth.tar-7")
    for name in ("model-best.pth.tar", "model.pth.tar-7"):
        got = torch.load(os.path.join(d, name), map_location="cpu", weights_only=True)
        assert got["epoch"] == 7 and got["val_result"] == 55.5
        assert set(got["state_dict"]) == {"text_prompt", "img_prompt"}

        class PL(torch.nn.Module):                          # the reader's target module, shape-wise
            def __init__(self):
                super().__init__()
                self.text_prompt = torch.nn.Parameter(torch.zeros(K, dt))
                self.img_prompt = torch.nn.Parameter(torch.zeros(K, dv))
        pl = PL()
        missing = pl.load_state_dict(got["state_dict"], strict=False)
        assert not missing.missing_keys and not missing.unexpected_keys
        assert torch.equal(pl.text_prompt.data, state["text_prompt"])
        opt = torch.optim.SGD(pl.parameters(), lr=0.1, momentum=0.9)
        opt.load_state_dict(got["optimizer"])
        assert opt.param_groups[0]["lr"] == 0.005 and opt.param_groups[0]["weight_decay"] == 5e-4
        rows, _ = rows_from_state_dict(OptimConfig(), got["optimizer"], [(K, dt), (K, dv)])
        assert len(rows) == 1 and torch.equal(rows[0], mom)
    assert rows_from_state_dict(OptimConfig(), {"state": {}, "param_groups": []}, [(5,)]) is None


def test_committed_reference_checkpoint_fixture_layout():
    """tests/golden/ckpt_d1_k4 (written by tools/make_golden.py from the reference's own modules) is in the layout a
    real Dassl run leaves: its `scheduler` entry is the warm-up scheduler's state dict, which HOLDS the successor
    CosineAnnealingLR object and through it the optimiser -- so torch's weights-only load refuses it, and the product's
    restricted loader reads it (without arbitrary unpickling) and finds the keys the reader touches."""
    import pickle
    from rpo_amd.trainer import load_checkpoint_file
    d = os.path.join(ROOT, "tests", "golden", "ckpt_d1_k4", "prompt_learner")
    for name in ("model-best.pth.tar", "model.pth.tar-2"):
        with pytest.raises(pickle.UnpicklingError):
            torch.load(os.path.join(d, name), map_location="cpu", weights_only=True)
        ck = load_checkpoint_file(os.path.join(d, name))
        assert ck["epoch"] == 2 and {"text_prompt", "img_prompt", "token_prefix", "token_suffix"} == set(ck["state_dict"])
        succ = ck["scheduler"]["successor"]
        # the scheduler / optimiser objects come back as inert data holders (nothing needs them alive)
        assert type(succ).__name__ == "_Inert" and succ.T_max == 15 and type(succ.optimizer).__name__ == "_Inert"
        assert ck["scheduler"]["warmup_epoch"] == 1 and ck["scheduler"]["cons_lr"] == 1e-5
        assert set(ck["optimizer"]["state"]) == {0, 1}
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_ckpt_d1_k4.npz")))
    assert np.array_equal(ck["state_dict"]["text_prompt"].numpy(), g["text_prompt"])


def test_checkpoint_loader_refuses_arbitrary_callables(tmp_path, monkeypatch):
    """The restricted loader resolves an allow-list of names only: a pickle that reduces to os.system (or anything else
    outside tensors / containers / torch's optimiser + scheduler classes) is refused; dassl.* classes (un-vendored)
    become inert stand-ins; RPO_TRUST_CHECKPOINT=1 is the explicit opt-in to a full unpickle."""
    import pickle
    import sys
    import types
    from rpo_amd.trainer import load_checkpoint_file

    marker = tmp_path / "pwned"

    class Evil:
        def __reduce__(self):
            return (os.system, (f"touch {marker}",))

    f = str(tmp_path / "evil.pth")
    torch.save({"state_dict": {}, "epoch": 1, "x": Evil()}, f)
    monkeypatch.delenv("RPO_TRUST_CHECKPOINT", raising=False)
    with pytest.raises(pickle.UnpicklingError, match="not allowed"):
        load_checkpoint_file(f)
    assert not marker.exists()
    # a class from the un-vendored trainer engine inside the scheduler entry: inert stand-in, rest of the file intact
    mod = types.ModuleType("dassl.optim.lr_scheduler")

    class ConstantWarmupScheduler:
        def __init__(self):
            self.warmup_epoch = 1
    ConstantWarmupScheduler.__module__ = "dassl.optim.lr_scheduler"
    ConstantWarmupScheduler.__qualname__ = "ConstantWarmupScheduler"
    mod.ConstantWarmupScheduler = ConstantWarmupScheduler
    for name in ("dassl", "dassl.optim"):
        monkeypatch.setitem(sys.modules, name, types.ModuleType(name))
    monkeypatch.setitem(sys.modules, "dassl.optim.lr_scheduler", mod)
    f2 = str(tmp_path / "dassl.pth")
    torch.save({"state_dict": {"text_prompt": torch.ones(2, 3)}, "epoch": 4, "scheduler": ConstantWarmupScheduler()}, f2)
    for name in ("dassl", "dassl.optim", "dassl.optim.lr_scheduler"):
        monkeypatch.delitem(sys.modules, name)
    ck = load_checkpoint_file(f2)
    assert ck["epoch"] == 4 and torch.equal(ck["state_dict"]["text_prompt"], torch.ones(2, 3))
    assert type(ck["scheduler"]).__name__ == "_Inert" and ck["scheduler"].warmup_epoch == 1


def _torch_zip_with_pickle(path, payload: bytes):
    """A torch-zip checkpoint whose data.pkl is `payload` (hand-written pickle opcodes)."""
    import io
    import zipfile
    buf = io.BytesIO()
    torch.save({"epoch": 1}, buf)
    src = zipfile.ZipFile(io.BytesIO(buf.getvalue()))
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as dst:
        for item in src.infolist():
            data = src.read(item.filename)
            dst.writestr(item.filename, payload if item.filename.endswith("data.pkl") else data)


def test_checkpoint_loader_refuses_dotted_names_and_reexported_callables(tmp_path, monkeypatch):
    """Advisor finding (round 3): pickle protocol 4 resolves a dotted name by a getattr chain, so
    GLOBAL('torch.optim.lr_scheduler', 'types.FunctionType') reached types.FunctionType through a module the old prefix
    rule allowed, and the un-dotted `partial` (functools.partial, re-exported there) passed too.  Now: dotted names are
    refused; everything under torch.optim resolves to the inert stand-in, whose call does nothing."""
    import pickle
    from rpo_amd.trainer import _Inert, _RestrictedUnpickler, load_checkpoint_file
    import io
    monkeypatch.delenv("RPO_TRUST_CHECKPOINT", raising=False)
    marker = tmp_path / "pwned"
    u = _RestrictedUnpickler(io.BytesIO(b""))
    for mod, name in (("torch.optim.lr_scheduler", "types.FunctionType"), ("torch.optim.lr_scheduler", "types.CodeType"),
                      ("torch", "optim.lr_scheduler.types.FunctionType"), ("collections", "OrderedDict.fromkeys"),
                      ("builtins", "dict.fromkeys"), ("os", "system"), ("builtins", "eval"), ("builtins", "getattr")):
        with pytest.raises(pickle.UnpicklingError):
            u.find_class(mod, name)
    assert u.find_class("torch.optim.lr_scheduler", "partial") is _Inert
    assert u.find_class("torch.optim.lr_scheduler", "CosineAnnealingLR") is _Inert
    assert u.find_class("torch.optim.sgd", "SGD") is _Inert
    # end to end, protocol 4 (STACK_GLOBAL, the dotted-name path of the C unpickler), inside a real torch zip:
    # partial(os.system, "touch marker")() -- with the old rule `partial` resolved to functools.partial
    def sglobal(m, n):
        return (b"\x8c" + bytes([len(m)]) + m.encode() + b"\x8c" + bytes([len(n)]) + n.encode() + b"\x93")
    cmd = f"touch {marker}".encode()
    evil = (b"\x80\x04" + sglobal("torch.optim.lr_scheduler", "partial") + sglobal("os", "system")
            + b"\x8c" + bytes([len(cmd)]) + cmd + b"\x86R" + b")R.")           # partial(os.system, cmd)()
    f = str(tmp_path / "evil4.pth")
    _torch_zip_with_pickle(f, evil)
    with pytest.raises(pickle.UnpicklingError, match="not allowed"):
        load_checkpoint_file(f)
    assert not marker.exists()
    dotted = b"\x80\x04" + sglobal("torch.optim.lr_scheduler", "types.FunctionType") + b"."
    f = str(tmp_path / "dotted.pth")
    _torch_zip_with_pickle(f, dotted)
    with pytest.raises(pickle.UnpicklingError, match="dotted"):
        load_checkpoint_file(f)
    # `partial` alone (no os.system in reach) is inert: calling it builds nothing callable
    harmless = (b"\x80\x04" + sglobal("torch.optim.lr_scheduler", "partial") + b"K\x01\x85R.")
    f = str(tmp_path / "partial.pth")
    _torch_zip_with_pickle(f, harmless)
    assert type(load_checkpoint_file(f)).__name__ == "_Inert"


def test_gradsync_leaves_the_current_device_alone_outside_a_launcher(monkeypatch):
    """A lone process (no LOCAL_RANK, world size 1) must not have its current device moved by constructing GradSync
    (the trainer builds one by default): only a distributed run pins the process to its local rank's GPU."""
    from rpo_amd import dist as rdist
    calls = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 8)
    monkeypatch.setattr(torch.cuda, "set_device", lambda i: calls.append(i))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RPO_FORCE_DIST", "RPO_ALL_RANKS_ON_GPU0"):
        monkeypatch.delenv(k, raising=False)
    s = rdist.GradSync(init=False)
    assert not s.enabled and calls == []
    monkeypatch.setenv("WORLD_SIZE", "8"); monkeypatch.setenv("RANK", "5"); monkeypatch.setenv("LOCAL_RANK", "5")
    s = rdist.GradSync(init=False)
    assert s.enabled and calls == [5] and s.shard(256) == (160, 32)


def test_config_from_state_dict_and_seeded_init_formula():
    from rpo_amd import synth
    from rpo_amd.config import vit_b16, vit_l14
    from rpo_amd.custom_clip import config_from_state_dict, init_prompts
    for c in (vit_b16(layers_v=2, layers_t=3, K=5), vit_l14(layers_v=1, layers_t=1)):
        sd = synth.clip_state_dict(c, seed=0, token_rows=[49407])
        assert config_from_state_dict(sd, c.K, c.n_cls) == c
    # G7: the reference's own initialisation under torch.manual_seed(3)
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_init_seed3_d1_k4.npz")))
    c = vit_b16(layers_v=1, layers_t=1, K=4)
    sd = synth.clip_state_dict(c, seed=0, logit_scale=float(np.log(100.0)))
    torch.manual_seed(int(g["seed"]))
    tp, ip = init_prompts(sd, 4, c.d_t, c.d_v)
    assert np.abs(tp - g["text_prompt"]).max() <= 1e-7 and np.abs(ip - g["img_prompt"]).max() <= 1e-7


def test_config_dims():
    from rpo_amd.config import vit_b16, vit_l14
    b, l = vit_b16(), vit_l14()
    assert (b.n_frozen, b.seq_v, b.heads_v, b.heads_t, b.patch_dim) == (197, 221, 12, 8, 768)
    assert (l.n_frozen, l.seq_v, l.heads_v, l.heads_t, l.patch_dim) == (257, 281, 16, 12, 588)


# ---- input pipeline host logic (rpo_amd/input_pipeline.py) ------------------------------------------------------

def test_input_pipeline_plans_match_oracle_sampler():
    from oracle import resample_oracle as R
    from rpo_amd import input_pipeline as ip

    class Seq:
        def __init__(self, seed): self.g = np.random.default_rng(seed)
        def uniform(self, a, b): return a + (b - a) * float(self.g.random())
        def randint(self, lo, hi): return int(self.g.integers(lo, hi))
        def rand(self): return float(self.g.random())
    for seed, (h, w) in enumerate([(375, 500), (500, 375), (40, 2000), (2000, 40), (224, 224), (1, 1)]):
        assert ip.random_resized_crop_params(h, w, Seq(seed)) == R.random_resized_crop_params(h, w, Seq(seed))
        assert ip.center_crop_window(h, w, 224) == R.eval_window(h, w, 224)
    assert ip.CLIP_MEAN == R.CLIP_MEAN and ip.CLIP_STD == R.CLIP_STD


def test_torch_rng_crops_are_reproducible_and_inside_the_image():
    import torch
    from rpo_amd import input_pipeline as ip
    torch.manual_seed(123)
    a = [ip.random_resized_crop_params(375, 500, ip.TorchRng()) for _ in range(50)]
    torch.manual_seed(123)
    b = [ip.random_resized_crop_params(375, 500, ip.TorchRng()) for _ in range(50)]
    assert a == b and len(set(a)) > 40
    for i, j, h, w in a:
        assert 0 <= i and i + h <= 375 and 0 <= j and j + w <= 500 and h > 0 and w > 0
        assert 0.08 * 375 * 500 * 0.9 <= h * w <= 375 * 500


def test_subsample_classes_and_fewshot():
    """datasets/oxford_pets.py:140-186 (base = first ceil(n/2) labels, relabelled from 0) and the Dassl few-shot
    sampler it calls at :44-45."""
    import random
    from rpo_amd.input_pipeline import Datum, generate_fewshot_dataset, subsample_classes
    data = [Datum(f"img_{c}_{k}.jpg", c, f"class{c}") for c in range(37) for k in range(6)]
    test = [Datum(f"t_{c}.jpg", c, f"class{c}") for c in range(37)]
    base_tr, base_te = subsample_classes(data, test, subsample="base")
    new_tr, new_te = subsample_classes(data, test, subsample="new")
    assert sorted({d.label for d in base_tr}) == list(range(19)) and len(base_te) == 19
    assert sorted({d.label for d in new_tr}) == list(range(18)) and len(new_te) == 18
    assert {d.classname for d in new_tr} == {f"class{c}" for c in range(19, 37)}
    assert new_te[0].classname == "class19" and new_te[0].label == 0
    allx, = subsample_classes(data, subsample="all")
    assert len(allx) == len(data)
    shots = generate_fewshot_dataset(base_tr, 4, rng=random.Random(1))
    assert len(shots) == 19 * 4
    per = {}
    for d in shots:
        per.setdefault(d.label, set()).add(d.impath)
    assert all(len(v) == 4 for v in per.values())
    again = generate_fewshot_dataset(base_tr, 4, rng=random.Random(1))
    assert [d.impath for d in again] == [d.impath for d in shots]
    few = generate_fewshot_dataset(base_tr[:3], 16)                       # fewer than num_shots: keep all
    assert len(few) == 3
    rep = generate_fewshot_dataset(base_tr[:3], 16, repeat=True, rng=random.Random(0))
    assert len(rep) == 16


def test_prec_mapping():
    import torch
    from rpo_amd.config import act_dtype_for_prec
    assert act_dtype_for_prec("fp32") is torch.float32
    assert act_dtype_for_prec("fp16") is torch.float16 and act_dtype_for_prec("amp") is torch.float16
    with pytest.raises(ValueError):
        act_dtype_for_prec("int8")


def test_generated_k_loops_are_what_the_generators_emit(tmp_path):
    """rpo_amd/csrc/gemm_w4g_asm.inc / gemm_w4k_asm.inc are committed generator output (tools/gen_gemm_w4.py): a hand edit
    of either side without the other would silently change a schedule whose wait counts are derived, not written."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if not k.startswith("W4K_")}
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_gemm_w4.py"), str(tmp_path)], env=env, stdout=subprocess.DEVNULL)
    for inc in ("gemm_w4g_asm.inc", "gemm_w4k_asm.inc"):
        out = tmp_path / inc
        assert out.read_text() == open(os.path.join(ROOT, "rpo_amd", "csrc", inc)).read(), f"{inc} is stale: re-run tools/gen_gemm_w4.py"


def test_stats_group_query_needs_no_gpu():
    """rpo_gemm_stats_group is pure host logic (which partial-statistics layout a BIAS_RESID producer writes): 96 where the
    224x96 / 256x96 kernel applies (ViT-B/16, 32 / 64 images, K <= 59 prompts), 64 for the 288x64 geometry (ViT-L/14, 16 images) and
    wherever the generic tiles run."""
    import torch
    from rpo_amd import ops
    g = ops.gemm_stats_group
    assert g(7072, 768, 768, torch.bfloat16, (197, 24, 6304)) == 96
    assert g(7072, 768, 3072, torch.float16, (197, 24, 6304)) == 96
    assert g(2 * 7072, 768, 3072, torch.bfloat16, (197, 24, 2 * 6304)) == 96          # two rounds
    assert g(7072, 768, 768, torch.bfloat16, None) == 64                               # no row units
    assert g(7072, 768, 768, torch.float32, (197, 24, 6304)) == 64                     # f32 mode: generic kernels
    assert g(32 * 245, 768, 768, torch.bfloat16, (197, 48, 32 * 197)) == 96            # K = 48: 245 rows per image -> 256x96 tiles (round 4)
    assert g(32 * 261, 768, 768, torch.bfloat16, (197, 64, 32 * 197)) == 64            # K = 64: 261 rows: no one-round geometry
    assert g(3536, 768, 768, torch.bfloat16, (197, 24, 3152)) == 64                    # 16 images: half a round
    assert g(16 * 281, 1024, 4096, torch.bfloat16, (257, 24, 16 * 257)) == 64          # ViT-L/14: 288x64 tiles
    assert g(7072, 768, 192, torch.bfloat16, (197, 24, 6304)) == 64                    # K = 192: 3 k-tiles, not admitted


def test_committed_profiles_are_measurements_not_crash_logs():
    """Round 4 committed two Python tracebacks as `r04_*_timeline.txt` (tools/build_debug.sh lacked a translation unit
    and tools/collect_profiles.sh kept whatever a tool printed).  No tracked profile may hold a traceback or compiler
    output; collect_profiles.sh keeps a tool's output only on exit status 0; summarize_profiles.py refuses such files;
    build_debug.sh compiles every source the product library is built from."""
    import glob
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = []
    for f in sorted(glob.glob(os.path.join(root, "profiles", "*.txt"))):
        txt = open(f, errors="replace").read()
        if "Traceback (most recent call last)" in txt or re.search(r"(^|\s)(warning|error):", txt):
            bad.append(os.path.basename(f))
    assert not bad, f"profiles that are not measurements: {bad}"
    # in-kernel timelines of this round onwards: every phase delta is a plausible cycle count (a stamp the kernel does
    # not have once showed up as "+-393995800630558")
    for f in sorted(glob.glob(os.path.join(root, "profiles", "r0[5-9]_*timeline.txt"))):
        for m in re.finditer(r"\+(-?\d+)", open(f).read()):
            assert 0 <= int(m.group(1)) < 10 ** 7, f"{os.path.basename(f)}: phase delta {m.group(1)}"
    sh = open(os.path.join(root, "tools", "collect_profiles.sh")).read()
    assert "keep()" in sh and "exit 1" in sh and "Traceback (most recent call last)" in sh
    assert "REFUSED" in open(os.path.join(root, "tools", "summarize_profiles.py")).read()
    from rpo_amd.build import SOURCES
    dbg = open(os.path.join(root, "tools", "build_debug.sh")).read()
    missing = [s for s in SOURCES if s not in dbg]
    assert not missing, f"tools/build_debug.sh does not compile {missing}: the -DRPO_TIMELINE library would lack ABI symbols"


def test_mfma_busy_figure_is_in_one_clock_domain():
    """The north-star kernel figure in the bench line (roofline.qkv_gemm) is busy shader cycles over (duration x shader
    clock measured in the kernel) whenever the committed summary holds it, and says which summary it came from."""
    import types
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    res = bench.committed_qkv_gemm(types.SimpleNamespace(model="ViT-B/16", K=24, batch=32, dtype="bf16"))
    assert res is not None and res["target"] == 0.70 and res["source"].startswith("profiles/")
    if "stale" not in res and "mfma_busy" in res:
        lo, hi = sorted((res.get("mfma_busy_wall", 0.0), res.get("mfma_busy_lifetime", 1.0)))
        assert lo - 0.05 <= res["mfma_busy"] <= hi + 0.05, res
        assert res["met"] == (res["mfma_busy"] >= 0.70)


def test_golden_manifest_matches_the_committed_fixtures():
    """tests/golden/manifest_fullsize.json is the provenance record of the reference-generated fixtures: its byte counts
    are those of the committed files (a regenerated fixture with a stale record was an advisor finding in round 5)."""
    import json
    gold = os.path.join(ROOT, "tests", "golden")
    man = json.load(open(os.path.join(gold, "manifest_fullsize.json")))
    for name, rec in man["cases"].items():
        path = os.path.join(gold, f"ref_{name}.npz")
        assert os.path.exists(path), path
        assert os.path.getsize(path) == rec["bytes"], (name, os.path.getsize(path), rec["bytes"])


def test_default_import_path_touches_no_experimental_code():
    """The product engine reads none of the experiments' switches and the default import path never loads
    rpo_amd/experimental.py (it subclasses Engine and is imported by engine.make_engine under RPO_EXPERIMENTAL=1 only)."""
    import subprocess
    code = ("import sys, rpo_amd.engine, rpo_amd.trainer, rpo_amd.custom_clip, rpo_amd.coop, rpo_amd.zeroshot;"
            "assert 'rpo_amd.experimental' not in sys.modules; print('clean')")
    env = {k: v for k, v in os.environ.items() if k != "RPO_EXPERIMENTAL"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0 and "clean" in r.stdout, r.stderr[-2000:]
    src = open(os.path.join(ROOT, "rpo_amd", "engine.py")).read()
    exp_switches = ("RPO_CHAIN", "RPO_MLP_FUSED", "RPO_JOINT_BWD", "RPO_TEXT_BWD_FOLD", "RPO_BWD_PARTS", "RPO_BWD_FOLD_R3")
    code_only = "\n".join(line.split("#", 1)[0] for line in src.splitlines())
    for name in exp_switches:
        assert f'"{name}"' not in code_only, f"engine.py reads the experiment switch {name}"
    assert "xenv" not in code_only and len(src.splitlines()) <= 1000


def test_bench_dump_outputs_float32_and_bounded(tmp_path, monkeypatch):
    """bench.py --dump-outputs: every array lands as float32 DIR/<name>.npy; one above its share of the size limit is cut
    to a fixed, seeded sample of its rows -- the same rows on every run."""
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8192)
    big = np.arange(1000 * 8, dtype=np.float64).reshape(1000, 8)
    small = np.linspace(-1, 1, 6, dtype=np.float32).astype(np.float16).reshape(3, 2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a_big, b_big = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    a_small = np.load(tmp_path / "a" / "small.npy")
    assert a_big.dtype == np.float32 and a_small.dtype == np.float32
    assert a_big.nbytes <= 8192 // 2 and a_big.shape[1] == 8 and a_big.shape[0] > 1
    np.testing.assert_array_equal(a_big, b_big)
    rows = (a_big[:, 0] / 8).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(a_big, big[rows].astype(np.float32))
    np.testing.assert_array_equal(a_small, small.astype(np.float32))
