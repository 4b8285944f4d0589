#!/usr/bin/env python3
"""Measurements of DESIGN.md section 9w on one MI355X, one process: writes profiles/logreg_bench.json.

`LogisticProbe` (rpo_amd/logreg.py) on synthetic clustered features (Gaussian class clusters, spread 0.5, seeded; raw,
|f|^2 about 640), e = 512, norm_feat off, l2 log-spaced from 1e-6 to 1 over the S members, two cases:
  small: n 1 600, C 100, S 16          big: n 16 000, C 1 000, S 8

  (a) per-iteration time, every member active (tol far below reach): one replay of the captured chunk of `--chunk`
      iterations (loss_grad + step = four launches each) from the first enqueue to a device synchronise, divided by the
      chunk; and the two calls on their own, enqueued eagerly `--chunk` times.
  (b) whole-fit time: `reset()` + `fit(tol = 1e-4, max_iter)` from the zero start to the last read of the "done" flags,
      the graph captured by an untimed first fit.  max_iter is 20 000 for the small case and `--big-max-iter` for the big
      one (stated in the file): members that have not converged by then are counted, not hidden.
  (c) the baseline, if scikit-learn is importable: LogisticRegression(lbfgs, C = 1 / (l2 Omega), tol = 1e-4: the same
      max-norm on the same objective divided by C) on the same features in float64, the S problems one after the
      other on the threads OMP_NUM_THREADS gives it, capped at `--sk-max-iter` iterations per member; for the big case
      only a per-iteration time of one member (`--sk-big-iters` iterations), again stated in the file.

Every arm runs untimed first; medians of `--repeats` with min .. max.  The flop count of an iteration is the two GEMMs',
4 n C e S, over the replayed per-iteration time, against the fp32 matrix peak DESIGN.md section 2 uses.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"small": (1600, 100, 512, 16), "big": (16000, 1000, 512, 8)}


def timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v, nd=4):
    return dict(median_ms=round(statistics.median(v), nd), min_ms=round(min(v), nd), max_ms=round(max(v), nd), repeats=len(v))


def clustered(n, C, e, seed):
    rng = np.random.default_rng(seed)
    y = (np.arange(n) % C).astype(np.int64)
    rng.shuffle(y)
    centres = rng.standard_normal((C, e))
    return (centres[y] + 0.5 * rng.standard_normal((n, e))).astype(np.float32), y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="small,big")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--big-max-iter", type=int, default=1000)
    ap.add_argument("--sk-max-iter", type=int, default=1000)
    ap.add_argument("--sk-big-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logreg_bench.json"))
    a = ap.parse_args()
    import warnings

    import torch
    from rpo_amd import ops
    from rpo_amd.features import ImageFeatures
    from rpo_amd.logreg import LogisticProbe
    assert torch.cuda.is_available(), "bench_logreg.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    try:
        import sklearn
        from sklearn.linear_model import LogisticRegression
        sk = sklearn.__version__
    except ImportError:
        LogisticRegression, sk = None, None
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, sklearn=sk or "not importable: no baseline",
               threads=os.environ.get("OMP_NUM_THREADS", "unset"), tol=1e-4, chunk=a.chunk, norm_feat=False, fit_bias=True,
               features="synthetic Gaussian class clusters, spread 0.5, seed 2024 + n", cases=[])
    for name in a.cases.split(","):
        n, C, e, S = CASES[name]
        F, y = clustered(n, C, e, 2024 + n)
        l2 = np.logspace(-6, 0, S).tolist()
        feats = ImageFeatures({"n_images": n}, torch.from_numpy(F).to(dev), torch.from_numpy(y).to(dev), y.tolist(), dev)
        probe = LogisticProbe(feats, C, l2)
        max_iter = 20000 if name == "small" else a.big_max_iter
        # (a) per iteration, all members active
        probe.fit(tol=1e-30, max_iter=a.chunk, check_every=a.chunk)          # untimed: code objects, the capture
        g = probe._graphs[a.chunk]
        probe.done.zero_()
        t_it = [timed(g.replay, torch) / a.chunk for _ in range(a.repeats)]

        def only_grad():
            for _ in range(a.chunk):
                ops.logreg_loss_grad_sets(feats.feat, feats.labels_dev, probe.weight, probe.omega, probe.l2_dev, probe.y, C,
                                          probe.grads, probe.loss, probe.ws, False, True, probe.done)

        def only_step():
            for _ in range(a.chunk):
                ops.logreg_step_sets(probe.x, probe.y, probe.grads, probe.count, probe.t, probe.L, probe.tol, probe.done,
                                     probe.iters, probe.grad_inf)
        only_grad(); only_step()
        t_g = [timed(only_grad, torch) / a.chunk for _ in range(a.repeats)]
        t_s = [timed(only_step, torch) / a.chunk for _ in range(a.repeats)]
        it_ms = statistics.median(t_it)
        flop = 4.0 * n * C * e * S
        # (b) whole fit
        probe.reset()
        probe.fit(tol=1e-4, max_iter=max_iter, check_every=a.chunk)
        t_fit, info = [], None
        for _ in range(a.repeats):
            probe.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = probe.fit(tol=1e-4, max_iter=max_iter, check_every=a.chunk)
            t_fit.append((time.perf_counter() - t0) * 1e3)
        case = dict(case=name, n=n, C=C, e=e, S=S, l2=l2, workspace_mb=round(probe.ws.numel() * 4 / 2 ** 20, 1),
                    per_iteration_graph=stats(t_it), loss_grad_eager=stats(t_g), step_eager=stats(t_s),
                    gemm_tflops=round(flop / (it_ms * 1e-3) / 1e12, 2), fit_max_iter=max_iter, whole_fit=stats(t_fit, 2),
                    fit_iters=info["iters"], fit_converged=info["converged"],
                    fit_grad_inf=[float(f"{v:.3e}") for v in info["grad_inf"]])
        # (c) scikit-learn
        if LogisticRegression is not None:
            X = F.astype(np.float64)
            if name == "small":
                per, iters = [], []
                for s in range(S):
                    m = LogisticRegression(C=1.0 / (l2[s] * n), solver="lbfgs", tol=1e-4, max_iter=a.sk_max_iter)
                    t0 = time.perf_counter()
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        m.fit(X, y)
                    per.append((time.perf_counter() - t0) * 1e3)
                    iters.append(int(np.max(m.n_iter_)))
                case["sklearn"] = dict(max_iter=a.sk_max_iter, member_ms=[round(v, 1) for v in per], member_iters=iters,
                                       members_at_max_iter=sum(i >= a.sk_max_iter for i in iters),
                                       all_members_ms=round(sum(per), 1), repeats=1,
                                       ours_over_sklearn=round(statistics.median(t_fit) / sum(per), 4))
            else:
                s = S // 2
                m = LogisticRegression(C=1.0 / (l2[s] * n), solver="lbfgs", tol=1e-4, max_iter=a.sk_big_iters)
                t0 = time.perf_counter()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    m.fit(X, y)
                dt = (time.perf_counter() - t0) * 1e3
                case["sklearn"] = dict(note="per-iteration time only: one member, max_iter = sk_big_iters", member=s,
                                       iters=int(np.max(m.n_iter_)), ms_per_iteration_one_member=round(dt / max(1, int(np.max(m.n_iter_))), 1),
                                       ours_ms_per_iteration_all_members=round(it_ms, 4))
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        del probe, feats
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
