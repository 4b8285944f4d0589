"""Readers of the linear-probe fixtures (tools/make_golden_lp.py writes them, tests/test_lp_host.py and tests/test_gpu_lp.py
read them).

A dense e x e fp32 matrix is 1 MB at e = 512, so the fixtures hold no dense W: every reference gradient of lp_layer.weight
is dz^T . x (rank B) and is stored as its two factors, and the reference's W after SGD steps is the SGD recursion over those
gradients.  The generator checks both reconstructions against the reference's own dense tensors before it writes anything;
a few dense rows and the diagonal of each reference W are stored as well and are compared directly."""
import json
import os

import numpy as np
import torch


def c1_init(e: int):
    """Case c1's starting layer: W = 0.01 eye + N(0, 1e-3), b = N(0, 1e-2) (numpy PCG64, seed 2024)."""
    rng = np.random.default_rng(2024)
    w = (0.01 * np.eye(e) + rng.standard_normal((e, e)) * 1e-3).astype(np.float32)
    b = (rng.standard_normal(e) * 1e-2).astype(np.float32)
    return w, b


def grads(dz: np.ndarray, x: np.ndarray):
    """(weight.grad, bias.grad) of nn.Linear from the gradient of its output dz [B, e] and its input x [B, e], float64."""
    dz, x = np.asarray(dz, np.float64), np.asarray(x, np.float64)
    return dz.T @ x, dz.sum(0)


def sgd_replay(w0, b0, dzs, xs, lr: float, momentum: float, wd: float):
    """torch.optim.SGD (dampening 0, no nesterov) on (W, b) over the steps whose gradient factors are dzs[k], xs[k], in
    float64: (W, b, momentum of W, momentum of b) after the last step."""
    p = [np.asarray(w0, np.float64), np.asarray(b0, np.float64)]
    buf = [None, None]
    for dz, x in zip(dzs, xs):
        for i, g in enumerate(grads(dz, x)):
            g = g + wd * p[i]
            buf[i] = g if buf[i] is None else momentum * buf[i] + g
            p[i] = p[i] - lr * buf[i]
    return p[0], p[1], buf[0], buf[1]


def write_reference_checkpoint(npz_path: str, directory: str) -> str:
    """`<directory>/lp_layer/model.pth.tar-<epoch>` rebuilt from ref_lp_ckpt.npz: the reference's lp_layer after one
    torch.optim.SGD step from the identity, in the dict the reference's run saved -- its keys, optimizer param groups and
    scheduler state exactly as recorded there, its tensors from the step's gradient factors.  Returns the file path."""
    g = np.load(npz_path)
    layout = json.loads(bytes(g["layout"]).decode())
    e = int(g["dz"].shape[1])
    lr, mom, wd = (float(v) for v in g["sgd_hparams"])
    w, b, mw, mb = sgd_replay(np.eye(e), np.zeros(e), [g["dz"]], [g["x"]], lr, mom, wd)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    state = {int(i): {"momentum_buffer": t(m)} for i, m in ((0, mw), (1, mb))}
    ck = {"state_dict": {"weight": t(w), "bias": t(b)}, "epoch": layout["epoch"],
          "optimizer": {"state": state, "param_groups": layout["param_groups"]}, "scheduler": layout["scheduler"],
          "val_result": layout["val_result"]}
    assert list(ck) == layout["keys"], (list(ck), layout["keys"])
    path = os.path.join(directory, "lp_layer", f"model.pth.tar-{layout['epoch']}")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(ck, path)
    return path
