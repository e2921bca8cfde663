#!/usr/bin/env python3
"""Times what carries a trained GBDT onto new data (csrc/gbdt.hip: ptr_gbdt_leaf_sums, ptr_gbdt_predict_leaf, ptr_gbdt_add_by_leaf; GBDT.refit
and predict(pred_leaf=True) of ptranking_amd/gbdt.py) at the "mslr" shape of prof_gbdt.py.

    python profiles/prof_gbdt_lifecycle.py profiles/mi355x_gbdt_lifecycle.json

The data, the parameters (num_leaves 400, max_bin 255) and the objective are prof_gbdt.py's.  TREES trees are grown with update() under
the LambdaMART objective, timed by a host clock around a device synchronise: milliseconds per tree of update(), for scale.  Then, per
round, in the same process: refit of those trees on the training matrix under the same objective (milliseconds per tree, whole: objective,
quantize, leaf sums, the host read, the value rule in Python, add by leaf), the leaf_sums kernel alone under device events for one tree
in each launch form the library reports, and pred_leaf over 100 trees (the grown trees repeated: the walk does not care) on the first
PRED_ROWS rows.  Medians of ROUNDS rounds; all rounds are kept.  The measurement runs in a child process; the parent never opens the GPU.
No LightGBM figure stands beside these: the library is not installed on these machines.
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

ROUNDS = 5
TREES = 5
PRED_ROWS = 262_144


def measure():
    import ctypes
    import numpy as np
    import torch
    import prof_gbdt
    import prof_tree
    import ptranking_amd as pa
    import ptranking_amd.functional as F
    from bench import MSLR_P
    from ptranking_amd import _lib, tree

    assert torch.cuda.is_available(), "prof_gbdt_lifecycle.py measures on the GPU only"
    dev = torch.device("cuda:0")
    nf = prof_gbdt.SHAPES["mslr"]["features"]
    _, _, group = prof_tree.draw()
    n = int(group.sum())
    gen = torch.Generator(device=dev).manual_seed(137)
    X = torch.randn((n, nf), device=dev, generator=gen)
    w = torch.randn(nf, device=dev, generator=gen) / nf ** 0.5
    s = X @ w + 0.8 * X[:, 0] * X[:, 1] + 0.5 * torch.randn(n, device=dev, generator=gen)
    cuts = torch.quantile(s[:1_000_000], torch.tensor(np.cumsum(MSLR_P)[:-1] / np.sum(MSLR_P), device=dev, dtype=torch.float32))
    y = torch.bucketize(s, cuts).float().cpu().numpy()
    params = prof_gbdt.PARAMS
    booster = pa.GBDT(params, X)
    lm = pa.LambdaMART(params)
    res = tree._Resident(y, group, dev)
    gh = (torch.empty_like(booster.scores), torch.empty_like(booster.scores))

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def one_update():
        lm.grad_hess(booster.scores, res, gh)
        booster.update(*gh)

    one_update()                                                           # warm-up: the first tree also pays the first launches
    update_ms = [wall(one_update)[0] for _ in range(TREES - 1)]
    objective = lambda scores: lm.grad_hess(scores, res, gh)
    leaves = [int(t["value"].size) for t in booster.trees]

    def form(nleaves):
        a, o = (ctypes.c_int64 * 2)(n, nleaves), (ctypes.c_int32 * 8)()
        assert _lib.load().ptr_launch_form(b"ptr_gbdt_leaf_sums", a, 2, o, 8) == 0
        return list(o)[:5]

    fl = booster._flat_device(dev)
    hi = int(booster.flat()["tree_offsets"][1])
    qg, qh, _, _ = F.gbdt_quantize(*lm.grad_hess(booster.scores, res))
    leaf = torch.empty(n, device=dev, dtype=torch.int32)
    sums = torch.zeros((leaves[0], 3), device=dev, dtype=torch.int64)
    wide = torch.zeros((2048, 3), device=dev, dtype=torch.int64)          # more cells than the LDS budget: the same tree through the global form
    kernel = {"lds": lambda: F.gbdt_leaf_sums(X, fl["feature"][:hi], fl["threshold"][:hi], fl["left"][:hi], fl["right"][:hi], qg, qh, leaves[0], leaf=leaf,
                                              sums=sums),
              "global": lambda: F.gbdt_leaf_sums(X, fl["feature"][:hi], fl["threshold"][:hi], fl["left"][:hi], fl["right"][:hi], qg, qh, 2048, leaf=leaf,
                                                 sums=wide)}
    hundred = pa.GBDT(params)
    hundred.edges, hundred.nbins = booster.edges, booster.nbins
    hundred.trees = (booster.trees * (100 // len(booster.trees) + 1))[:100]
    Xp = X[:PRED_ROWS].contiguous()
    booster.refit(X, objective), kernel["lds"](), kernel["global"](), hundred.predict(Xp, pred_leaf=True, check_finite=False)      # warm-up
    refit_ms, leaf_ms, kernel_ms = [], [], {k: [] for k in kernel}
    for i in range(ROUNDS):
        print(f"round {i + 1} of {ROUNDS}", file=sys.stderr, flush=True)
        refit_ms.append(wall(lambda: booster.refit(X, objective))[0] / len(booster.trees))
        for k, fn in kernel.items():
            kernel_ms[k].append(events(fn)[0])
        leaf_ms.append(wall(lambda: hundred.predict(Xp, pred_leaf=True, check_finite=False))[0])
    same = (sums[:, 2].sum().item(), wide[:, 2].sum().item())
    out = dict(shape="mslr", documents=n, features=nf, params=params, trees=len(booster.trees), leaves_per_tree=leaves,
               update_ms_per_tree=statistics.median(update_ms), all_update_ms=update_ms,
               refit_ms_per_tree=statistics.median(refit_ms), all_refit_ms_per_tree=refit_ms,
               refit_note="whole refit under the LambdaMART objective over the training matrix, divided by the trees: objective + quantize + "
                          "leaf sums + one host read + the value rule in Python + add by leaf",
               leaf_sums_kernel_ms={k: statistics.median(v) for k, v in kernel_ms.items()}, all_leaf_sums_kernel_ms=kernel_ms,
               leaf_sums_forms={"lds": form(leaves[0]), "global": form(2048)}, leaf_sums_rows_counted=same,
               pred_leaf_rows=PRED_ROWS, pred_leaf_ms_per_100_trees=statistics.median(leaf_ms), all_pred_leaf_ms=leaf_ms,
               pred_leaf_rows_x_trees_per_second=PRED_ROWS * 100 / (statistics.median(leaf_ms) * 1e-3))
    print(json.dumps(out))


def main(out_path):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure"], stdout=subprocess.PIPE, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("the measurement failed")
    result = json.loads(r.stdout.strip().splitlines()[-1])
    with open(out_path, "w") as f:
        json.dump(dict(rounds=ROUNDS, note="no LightGBM comparison exists: the library is not installed on these machines", mslr=result), f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("update_ms_per_tree", "refit_ms_per_tree", "leaf_sums_kernel_ms", "pred_leaf_ms_per_100_trees")}))
    print(f"wrote {out_path}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--measure":
        measure()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_gbdt_lifecycle.json"))
