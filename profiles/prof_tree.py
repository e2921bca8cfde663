#!/usr/bin/env python3
"""Times one TreeObjective call (csrc/tree.hip behind ptranking_amd/tree.py) on an MSLR-shaped ragged batch against the only alternative a
user has on the same GPU without it: the closed form of the reference's per_query_gradient_hessian_lambda restated in eager torch over
PADDED [chunk, L, L] tensors, one length class at a time, in chunks that fit a byte budget.

    python profiles/prof_tree.py profiles/mi355x_tree_objectives.json
    python profiles/prof_tree.py --xendcg profiles/mi355x_xendcg.json [kernel_stats.csv]    # rank_xendcg's and ListNet's calls side by side
        (CALL time: host enqueue included.  kernel_stats.csv: the *_kernel_stats.csv of a run of the same command under
        `rocprofv3 --kernel-trace --stats`, made first and on its own; its kernel times are folded into the file)

Scenario: QUERIES queries whose lengths follow the mix bench.py's padded batches use (bench.padded_lens, the lengths behind its
pair_statistics rows): Gamma(2.2) with mean 120, here clipped to MSLR-WEB30K's [1, 1251] instead of a padded L, with four lists of 1251 documents
planted (the draw's own tail ends near 700); labels from bench.MSLR_P,
the label histogram of MSLR-WEB30K; scores 0.8 label + N(0, 1.5).  QUERIES = 19 000 is one training fold of MSLR-WEB30K.
Reported per objective: the whole call (host preds in, float64 grad / hess out, wall clock), and inside it the kernel launches and the
two copies separately (device events); medians of ROUNDS rounds with the variants alternating inside a round, every round kept.
pairs/s is ordered pairs (sum of n (n - 1)) per kernel second, against the VALU-issue bound counted from the arithmetic with the
constants of ptranking_amd/peaks.py.  The reference's own cost is NOT measured here (it does not exist on the GPU machine): 0.085 s for one
128-document query with pair_type 'All' was measured on the CPU of the build machine (REFERENCE_CPU below), a Python loop over 8128 pairs.
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ptranking_amd.peaks import NUM_SIMD, PEAK_CLOCK_HZ, TRANS_CYCLES_PER_INSTR, VALU_CYCLES_PER_INSTR  # noqa: E402

QUERIES = 19000
MAX_LEN = 1251
ROUNDS = 7
CHUNK_BYTES = 1 << 28            # budget of one [chunk, L, L] fp32 intermediate of the eager form
REFERENCE_CPU = dict(seconds_per_query=0.085, documents=128, pair_type="All", measured_on="the build machine's CPU, not on the GPU machine",
                     what="ptranking/ltr_tree/util/lightgbm_util.py per_query_gradient_hessian_lambda, numpy 2.2.6")
VARIANTS = {"ranknet_reference": dict(objective="ranknet"), "lambdarank_reference": dict(objective="lambdarank"),
            "lambdamart_sum": dict(objective="lambdarank", weighting="DeltaNDCG", hessian="sum"), "listnet": dict(objective="listnet"),
            "rank_xendcg": dict(objective="rank_xendcg")}
XENDCG_REPS = int(os.environ.get("PROF_XENDCG_REPS", 2000))      # (fewer under a trace, which records every launch)
# launch sets per timed window of --xendcg (one set: every length class once): windows of ~0.2 s


def pair_issue_cycles(weighted):
    """Least issue cycles of one ORDERED pair in the thread-per-document form at epsilon 1, counted from the arithmetic:
    d = s_i - s_j, |d| log2 e, exp, 1 + e, rcp + 2 Newton FMAs, e r, select p, y_i - y_j, clip, target FMA, p - t, x epsilon, the tie compare and
    3 mask operations, select + add into grad; r r, e (r r), x epsilon^2, floor, the rank sign (2 compares, and/or, select), select + add into
    hess -> 27 VALU + 2 transcendental; the Delta-nDCG weight adds 2 subtractions and 3 multiplications."""
    valu = 27 + (5 if weighted else 0)
    return valu * VALU_CYCLES_PER_INSTR + 2 * TRANS_CYCLES_PER_INSTR


def draw(seed=137):
    import numpy as np
    from bench import MSLR_P
    rng = np.random.default_rng(seed)
    group = np.clip(np.round(rng.gamma(2.2, 120.0 / 2.2, QUERIES)), 1, MAX_LEN).astype(np.int32)
    group[::QUERIES // 4] = MAX_LEN                            # the Gamma tail ends near 700: plant the collection's longest list four times
    labels = rng.choice(5, size=int(group.sum()), p=np.asarray(MSLR_P) / np.sum(MSLR_P)).astype(np.float32)
    preds = (0.8 * labels + 1.5 * rng.standard_normal(labels.size)).astype(np.float32)
    return preds, labels, group


def eager_class(S, Y, lens, pair_type, weighted, signed):
    """The closed form over one padded chunk [b, L] (scores, labels, lens) -> grad, hess [b, L]; index tie-break through a stable sort."""
    import torch
    b, L = S.shape
    real = torch.arange(L, device=S.device)[None, :] < lens[:, None]
    order = torch.sort(torch.where(real, S, torch.full_like(S, -float("inf"))), dim=1, descending=True, stable=True)[1]
    rank = torch.empty_like(order).scatter_(1, order, torch.arange(L, device=S.device).expand(b, L))
    d = S[:, :, None] - S[:, None, :]
    p = torch.sigmoid(d)
    dy = Y[:, :, None] - Y[:, None, :]
    M = real[:, :, None] & real[:, None, :] & ~torch.eye(L, dtype=torch.bool, device=S.device)
    if pair_type == "NoTies":
        M = M & (dy != 0)
    w = None
    if weighted:
        disc = 1.0 / torch.log2(torch.arange(L, device=S.device, dtype=torch.float32) + 2.0)
        ideal = torch.sort(torch.where(real, Y, torch.zeros_like(Y)), dim=1, descending=True)[0]
        G = (torch.exp2(Y) - 1.0) / ((torch.exp2(ideal) - 1.0) * disc).sum(1, keepdim=True)
        D = disc[rank]
        w = (G[:, :, None] - G[:, None, :]).abs() * (D[:, :, None] - D[:, None, :]).abs()
    T = p - 0.5 * (1.0 + dy.clamp(-1.0, 1.0))
    h = (p * (1.0 - p)).clamp_min(1e-16)
    if w is not None:
        T, h = T * w, h * w
    if signed:
        h = torch.where(rank[:, None, :] > rank[:, :, None], h, -h)
    zero = torch.zeros((), device=S.device)
    return torch.where(M, T, zero).sum(2), torch.where(M, h, zero).sum(2)


def main(out_path):
    import numpy as np
    import torch
    import ptranking_amd as pa
    import ptranking_amd.functional as F

    assert torch.cuda.is_available(), "prof_tree.py measures on the GPU only"
    dev = torch.device("cuda:0")
    preds, labels, group = draw()
    off = np.concatenate([[0], np.cumsum(group.astype(np.int64))])
    pairs = int((group.astype(np.int64) * (group.astype(np.int64) - 1)).sum())

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    objs = {k: pa.TreeObjective(labels, group, **kw) for k, kw in VARIANTS.items()}

    def parts(obj):
        """The three steps of TreeObjective._run, each under its own device events."""
        res = obj._own
        host = np.ascontiguousarray(preds, dtype=np.float32)
        h2d, p = events(lambda: torch.from_numpy(host).to(dev))
        out = (torch.empty_like(p), torch.empty_like(p))

        def launches():
            for max_len, queries in res.buckets:
                if obj.kind == "pair":
                    F.tree_pair_grad_hess(p, res.labels, res.offsets, obj.pair_type, obj.weighting, obj.epsilon, obj.hessian, queries, max_len, out)
                elif obj.kind == "xendcg":
                    F.tree_xendcg_grad_hess(p, res.labels, res.offsets, obj.objective_seed, 0, None, queries, max_len, out)
                else:
                    F.tree_listnet_grad_hess(p, res.labels, res.offsets, obj.gain_type, obj.hessian, queries, max_len, out)
        kern, _ = events(launches)
        d2h, _ = events(lambda: torch.stack(out).cpu())
        return dict(h2d_ms=h2d, kernel_ms=kern, d2h_ms=d2h)

    def whole(obj):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        obj(preds)
        return (time.perf_counter() - t0) * 1e3

    # the eager form: queries padded per length class of the product's own bucketing
    classes = []
    for max_len, idx in objs["ranknet_reference"]._own.buckets_host:
        S, Y = np.zeros((len(idx), max_len), np.float32), np.zeros((len(idx), max_len), np.float32)
        for r, q in enumerate(idx):
            S[r, :group[q]], Y[r, :group[q]] = preds[off[q]:off[q + 1]], labels[off[q]:off[q + 1]]
        classes.append((torch.from_numpy(S).to(dev), torch.from_numpy(Y).to(dev), torch.from_numpy(group[idx].astype(np.int64)).to(dev), idx, max_len))

    def eager(kw):
        pt = pa.tree.OBJECTIVES[kw["objective"]][1]
        outs = []
        for S, Y, lens, _, L in classes:
            chunk = max(1, CHUNK_BYTES // (L * L * 4))
            outs.append([eager_class(S[lo:lo + chunk], Y[lo:lo + chunk], lens[lo:lo + chunk], pt, kw.get("weighting") == "DeltaNDCG",
                                     kw.get("hessian", "reference") == "reference") for lo in range(0, S.shape[0], chunk)])
        return outs

    # same results first: the eager form against the kernel on every real document (1e-4 of the largest entry, far above fp32 summation order)
    agree = {}
    for k in ("ranknet_reference", "lambdamart_sum"):
        grad, hess = objs[k](preds)
        worst = 0.0
        for (S, Y, lens, idx, L), outs in zip(classes, eager(VARIANTS[k])):
            eg = torch.cat([o[0] for o in outs]).cpu().numpy()
            eh = torch.cat([o[1] for o in outs]).cpu().numpy()
            for r, q in enumerate(idx):
                n = group[q]
                for got, ref in ((grad[off[q]:off[q + 1]], eg[r, :n]), (hess[off[q]:off[q + 1]], eh[r, :n])):
                    worst = max(worst, float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)))
        agree[k] = worst
    assert all(v <= 1e-4 for v in agree.values()), agree

    for obj in objs.values():
        whole(obj); parts(obj)
    eager_keys = ("ranknet_reference", "lambdamart_sum")
    for k in eager_keys:
        eager(VARIANTS[k])
    torch.cuda.synchronize()
    rounds = {k: dict(call_ms=[], h2d_ms=[], kernel_ms=[], d2h_ms=[]) for k in objs}
    eager_rounds = {k: [] for k in eager_keys}
    for _ in range(ROUNDS):
        for k, obj in objs.items():
            rounds[k]["call_ms"].append(whole(obj))
            for name, v in parts(obj).items():
                rounds[k][name].append(v)
        for k in eager_keys:
            eager_rounds[k].append(events(lambda: eager(VARIANTS[k]))[0])
    rows = {}
    for k, r in rounds.items():
        med = {name: statistics.median(v) for name, v in r.items()}
        row = dict(config=VARIANTS[k], median_ms=med, all_rounds_ms=r)
        if objs[k].kind == "pair":
            weighted = VARIANTS[k].get("weighting") == "DeltaNDCG"
            peak = NUM_SIMD * PEAK_CLOCK_HZ * 64.0 / pair_issue_cycles(weighted)
            row.update(pairs_per_s=pairs / (med["kernel_ms"] * 1e-3),
                       valu_issue_bound=dict(cycles_per_ordered_pair=pair_issue_cycles(weighted), peak_pairs_per_s=peak,
                                             bound_ms=pairs / peak * 1e3, share_of_bound=(pairs / peak * 1e3) / med["kernel_ms"]))
        if k in eager_rounds:
            em = statistics.median(eager_rounds[k])
            row.update(eager_padded_ms=em, eager_all_rounds_ms=eager_rounds[k], kernel_speedup_vs_eager=em / med["kernel_ms"],
                       max_rel_diff_vs_eager=agree[k])
            assert med["kernel_ms"] <= em, "the fused launches are slower than padded eager torch"
        rows[k] = row
        print(json.dumps({"variant": k, "median_ms": med, "pairs_per_s": row.get("pairs_per_s"), "eager_padded_ms": row.get("eager_padded_ms")}), flush=True)
    scenario = dict(queries=QUERIES, documents=int(group.sum()), ordered_pairs=pairs, longest=int(group.max()), mean_len=float(group.mean()),
                    lengths="Gamma(2.2), mean 120 (bench.padded_lens), clipped to [1, 1251], four lists of 1251 planted", labels="bench.MSLR_P",
                    length_classes=[(m, len(i)) for m, i in objs["ranknet_reference"]._own.buckets_host], eager_chunk_bytes=CHUNK_BYTES, rounds=ROUNDS)
    ref_s = REFERENCE_CPU["seconds_per_query"] * pairs / (128 * 127)
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, scenario=scenario, variants=rows,
                       reference_cpu=dict(REFERENCE_CPU, extrapolated_seconds_per_round=ref_s,
                                          note="0.085 s x ordered pairs / (128 x 127): an extrapolation from one measured query, not a measurement")),
                  f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


def kernel_stats(path, launches_per_set):
    """Kernel time per launch set from rocprofv3's kernel statistics of a run of main_xendcg, however many sets it made: the instances of
    each kernel template summed, over its launches / launches_per_set."""
    import csv
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for key, kern in (("listnet", "tree_listnet_kernel"), ("rank_xendcg", "tree_xendcg_kernel")):
                if kern in name:
                    o = out.setdefault(key, dict(kernel=kern, launches=0, total_ns=0.0))
                    o["launches"] += int(float(row["Calls"]))
                    o["total_ns"] += float(row["TotalDurationNs"])
    for o in out.values():
        o["kernel_ms_per_launch_set"] = o["total_ns"] * 1e-6 / (o["launches"] / launches_per_set)
    return out


def main_xendcg(out_path, stats_path=None):
    """rank_xendcg's calls against ListNet's on the same batch, at the same commit: both are a softmax per query; rank_xendcg reads the
    same 8 bytes and writes the same 8 bytes per document, hashes a uniform and does three more tree sums.  A timed window is XENDCG_REPS
    launch sets between two device events; ROUNDS windows per objective, alternating; every window kept.  What the events bracket is CALL
    time: six short launches per set, each entered through Python and ctypes, so the host's enqueue is in it.  Kernel time comes from a
    trace (kernel_stats)."""
    import numpy as np
    import torch
    import ptranking_amd as pa
    import ptranking_amd.functional as F

    assert torch.cuda.is_available(), "prof_tree.py measures on the GPU only"
    dev = torch.device("cuda:0")
    preds, labels, group = draw()
    res = pa.TreeObjective(labels, group, "rank_xendcg")._own
    p = torch.from_numpy(preds).to(dev)
    out = (torch.empty_like(p), torch.empty_like(p))

    def listnet():
        for max_len, queries in res.buckets:
            F.tree_listnet_grad_hess(p, res.labels, res.offsets, "Power", "reference", queries, max_len, out)

    def xendcg():
        for max_len, queries in res.buckets:
            F.tree_xendcg_grad_hess(p, res.labels, res.offsets, 5, 0, None, queries, max_len, out)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(XENDCG_REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / XENDCG_REPS

    fns = {"listnet": listnet, "rank_xendcg": xendcg}
    for fn in fns.values():
        window(fn)
    rounds = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            rounds[k].append(window(fn))
    docs = int(group.sum())
    rows = {}
    for k, v in rounds.items():
        med = statistics.median(v)
        rows[k] = dict(call_median_ms_per_launch_set=med, call_all_windows_ms=v)
        print(json.dumps({"variant": k, "call_median_ms_per_launch_set": med}), flush=True)
    ratio = rows["rank_xendcg"]["call_median_ms_per_launch_set"] / rows["listnet"]["call_median_ms_per_launch_set"]
    trace = None
    if stats_path:
        trace = kernel_stats(stats_path, len(res.buckets))
        trace["rank_xendcg_over_listnet"] = trace["rank_xendcg"]["kernel_ms_per_launch_set"] / trace["listnet"]["kernel_ms_per_launch_set"]
        print(json.dumps({"kernel_trace": trace}), flush=True)
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__,
                       scenario=dict(queries=QUERIES, documents=docs, longest=int(group.max()), mean_len=float(group.mean()),
                                     length_classes=[(m, len(i)) for m, i in res.buckets_host], launches_per_set=len(res.buckets),
                                     sets_per_window=XENDCG_REPS, windows=ROUNDS,
                                     bytes_per_document=16,
                                     what="CALL time: device events around XENDCG_REPS launch sets (one launch per length class), host "
                                          "enqueue through Python and ctypes included; kernel_trace: kernel time from rocprofv3 "
                                          "--kernel-trace --stats in a run of its own, summed over each kernel's instances"),
                       variants=rows, call_rank_xendcg_over_listnet=ratio, kernel_trace=trace), f, indent=1)
        f.write("\n")
    print(f"call time: rank_xendcg / listnet = {ratio:.3f}; wrote {out_path}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--xendcg":
        main_xendcg(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mi355x_xendcg.json"), sys.argv[3] if len(sys.argv) > 3 else None)
        sys.exit(0)
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_tree_objectives.json"))
