"""Cost of synchronised 'BN' statistics: default-pointsf LambdaRank train step, 1024 queries x 128 x 136, RCCL group of one,
switch off / on alternating step by step in one process, device events per step."""
import copy, os, statistics, sys, time
import numpy as np
import torch
import torch.distributed as dist

os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29531", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", PTR_DP_INIT_SINGLE="1")
import ptranking_amd as pa
from ptranking_amd import dp

dp.init_from_env()
assert dist.get_backend() == "nccl"
dp.SINGLE_RANK_COLLECTIVES = True
B, L, F = 1024, 128, 136
WARM, STEPS = 30, 250
rng = np.random.default_rng(5)
X = torch.from_numpy(rng.standard_normal((B, L, F)).astype(np.float32)).cuda()
Y = rng.choice(5, size=(B, L), p=[0.5, 0.3, 0.15, 0.03, 0.02]).astype(np.float32)
Y[:, 0] = np.maximum(Y[:, 0], 1)
Y = torch.from_numpy(-np.sort(-Y, axis=1).copy()).cuda()
sf = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-4, "pointsf": dict(num_features=F, num_layers=5, AF="GE", TL_AF="S", apply_tl_af=True, BN=True, bn_type="BN", bn_affine=True, dropout=0.1)}
rk = {}
for on in (False, True):
    torch.manual_seed(21)
    r = pa.LambdaRank(sf_para_dict=copy.deepcopy(sf), model_para_dict=dict(pa.DEFAULT_PARAS["LambdaRank"]), gpu=True, device="cuda:0")
    r.init(); r.train_mode()
    dp.sync_batch_norm(r, on)
    rk[on] = r
step = lambda r: r.train_op(X, Y, epoch_k=1, presort=True, label_type=pa.LABEL_TYPE.MultiLabel)
for _ in range(WARM):
    for on in (False, True):
        step(rk[on])
torch.cuda.synchronize()
ev = {False: [], True: []}
host = {False: [], True: []}
c0 = dp.BN_COLLECTIVES
for i in range(STEPS):
    for on in ((False, True) if i % 2 == 0 else (True, False)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(); step(rk[on]); b.record()
        host[on].append((time.perf_counter() - t0) * 1e3)
        ev[on].append((a, b))
torch.cuda.synchronize()
# wall clock of blocks of 50 steps ending in a synchronise, alternating
wall = {False: [], True: []}
for rep in range(6):
    for on in ((False, True) if rep % 2 == 0 else (True, False)):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(50):
            step(rk[on])
        torch.cuda.synchronize()
        wall[on].append((time.perf_counter() - t0) * 1e3 / 50)
lines = [f"default pointsf (5 x [Linear -> BN(affine) -> GELU] -> Linear -> BN -> Sigmoid, dropout 0.1), LambdaRank train step, {B} queries x {L} x {F}",
         f"RCCL process group of ONE rank (dp.SINGLE_RANK_COLLECTIVES): prices the extra launches and the collectives' fixed cost only; N > 1 over xGMI: not measured",
         f"switch off / on alternating step by step in one process, {WARM} warm-up steps each, {STEPS} timed steps each, device events around train_op",
         f"collectives counted by dp.BN_COLLECTIVES with the switch on: {(dp.BN_COLLECTIVES - c0) / (STEPS + 300):.1f} per step"]
for on in (False, True):
    t = sorted(a.elapsed_time(b) for a, b in ev[on])
    q = lambda f: t[int(f * (len(t) - 1))]
    h = sorted(host[on])
    lines.append(f"sync_batch_norm {'on ' if on else 'off'}: device-event ms/step median {statistics.median(t):.4f}  min {t[0]:.4f}  p10 {q(0.1):.4f}  p90 {q(0.9):.4f}  max {t[-1]:.4f}"
                 f" | host enqueue ms/step median {statistics.median(h):.4f} | wall ms/step over blocks of 50 (sync at the end): " + " ".join(f"{w:.4f}" for w in wall[on]))
m = {on: statistics.median(a.elapsed_time(b) for a, b in ev[on]) for on in (False, True)}
lines.append(f"difference of the medians: {(m[True] - m[False]) * 1e3:.1f} us per step = {(m[True] - m[False]) * 1e3 / 12:.1f} us per collective + its extra launches (12 per step)")
open(sys.argv[1], "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
dist.destroy_process_group()
