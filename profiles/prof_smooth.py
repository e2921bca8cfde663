#!/usr/bin/env python3
"""Times the smooth-rank metric objectives (csrc/smoothmetric.hip, ptr_smoothmetric_fwd_bwd) against
  (a) ptr_approxndcg_fwd_bwd in its per-query form at the same shape — the nDCG / opt_ideal / no-cut-off objective does the same pair work plus
      an O(L) step, so its ratio to (a) is what the generalisation costs;
  (b) the reference's composition (get_approx_ranks, approxNDCG.py:19-27, then metric_as_opt_objective.py, then autograd) restated in eager
      torch on the same GPU, batched in chunks whose [chunk, L, L] intermediate fits in memory.

    python profiles/prof_smooth.py profiles/mi355x_smooth_metric.json

Shapes: B = 4096 at L = 128 and B = 1024 at L = 512, full lists, alpha = 10, every metric in both modes with top_k in {None, 10}.  Every variant
is warmed up on the shape it is timed on and timed with device events over whole launches, ROUNDS times with the variants alternating inside
a round; the JSON keeps every round and reports the median.  Hardware constants come from ptranking_amd/peaks.py only.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ptranking_amd.peaks import NUM_SIMD, PEAK_CLOCK_HZ, TRANS_CYCLES_PER_INSTR, VALU_CYCLES_PER_INSTR  # noqa: E402

SHAPES = [(4096, 128), (1024, 512)]
METRICS = ("P", "AP", "nERR", "nDCG")
ROUNDS = 7
ALPHA = 10.0
CHUNK_BYTES = 1 << 30

# Issue count per UNORDERED pair over both passes of the ring kernel: (vector instructions, of which quarter-rate transcendentals), counted in
# the gfx950 code hipcc emits for smooth_ring_kernel (-O3): the bodies of the two 15-step ring loops divided by the pair evaluations of a
# step (2 DPT^2).  L = 128 (DPT 2): (80 + 117) / 8; L = 512 (DPT 8): (1184 + 1713) / 128; exp2 and rcp in each pass.  An ordered pair is half.
ISSUE_PER_UNORDERED_PAIR = {128: (24.6, 4.0), 512: (22.6, 4.0)}


def pair_issue_cycles(L):
    valu, trans = ISSUE_PER_UNORDERED_PAIR[L]
    return 0.5 * ((valu - trans) * VALU_CYCLES_PER_INSTR + trans * TRANS_CYCLES_PER_INSTR)      # per ORDERED pair


def eager_loss_grad(metric, preds, labels, top_k, opt_ideal, max_label=4.0, alpha=ALPHA):
    """The reference's composition for a batch [b, L] of full lists + autograd -> (loss_q, grad, same_order [b]).  Each query divides by its
    own ideal value (the reference's batched nERR couples the queries through a [b] / [b, 1] broadcast; the kernel's contract is one query at
    a time).  same_order: the re-sorted forms sort the fp32 smooth ranks, and two scores a few ulp apart can get equal or inverted fp32 ranks;
    the kernel ranks by the scores themselves.  Queries where the two orders differ are timed but left out of the agreement check."""
    import torch
    s = preds.detach().requires_grad_(True)
    y = labels
    b, n = s.shape
    x = alpha * (s.unsqueeze(1) - s.unsqueeze(2))
    e = torch.exp(-x.abs())
    r = torch.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e)).sum(2) + 0.5
    nat = torch.arange(n, dtype=s.dtype, device=s.device).view(1, -1) + 1.0
    k = n if not top_k else min(top_k, n)
    kdiv = n if not top_k else top_k
    yb = y.clamp(0, 1)
    same = torch.ones(b, dtype=torch.bool, device=s.device)
    if opt_ideal:
        rr, yy, bb = r, y, yb
    else:
        rr, idx = torch.sort(r, dim=1)
        yy, bb = torch.gather(y, 1, idx), torch.gather(yb, 1, idx)
        same = (idx == torch.sort(s.detach(), dim=1, descending=True, stable=True)[1]).all(1)
    gains = torch.pow(2.0, yy) - 1.0
    keep = torch.ones(b, dtype=torch.bool, device=s.device)
    if not opt_ideal and top_k:
        keep = {"P": bb, "AP": bb, "nERR": yy, "nDCG": gains}[metric][:, :k].sum(1) != 0
    if metric == "P":
        val = (nat[:, :k] / rr[:, :k] * bb[:, :k]).sum(1) / kdiv
    elif metric == "AP" and not opt_ideal and not top_k:
        val = (torch.cumsum(bb, 1) / rr * bb).sum(1) / bb.sum(1)
    elif metric == "AP":
        den = bb[:, :k].sum(1)
        val = ((torch.cumsum(nat / rr, 1) / nat)[:, :k] * bb[:, :k]).sum(1) / torch.where(keep, den, torch.ones_like(den))   # (a dropped row: no 0 / 0)
    elif metric == "nERR":
        def err(lab, inv_rank):
            sat = (torch.pow(2.0, lab[:, :k]) - 1.0) / 2.0 ** max_label
            cas = torch.cat([torch.ones_like(sat[:, :1]), torch.cumprod(1.0 - sat, 1)[:, :-1]], 1)
            return (inv_rank[:, :k] * sat * cas).sum(1)
        val = err(yy, 1.0 / rr) / err(y, (1.0 / nat).expand_as(y))
    else:
        idcg = ((torch.pow(2.0, y) - 1.0) / torch.log2(nat + 1.0)).sum(1)
        val = (gains / torch.log2(rr + 1.0))[:, :k].sum(1) / idcg
    (-val[keep].sum()).backward()                              # the reference's pos_inds: dropped queries pass no gradient
    return -torch.where(keep, val.detach(), torch.zeros_like(val)), s.grad, same


def main(out_path):
    import numpy as np
    import torch
    import ptranking_amd.functional as F

    assert torch.cuda.is_available(), "prof_smooth.py measures on the GPU only"
    dev = torch.device("cuda:0")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    results = []
    for B, L in SHAPES:
        rng = np.random.default_rng(137 + L)
        y = rng.choice(5, size=(B, L), p=[0.5147, 0.3250, 0.1339, 0.0183, 0.0081]).astype(np.float32)
        y[:, 0] = np.maximum(y[:, 0], 1)
        y = -np.sort(-y, axis=1)
        preds = torch.from_numpy((0.3 * y + 0.5 * rng.standard_normal((B, L))).astype(np.float32)).to(dev)
        labels = torch.from_numpy(y.copy()).to(dev)
        chunk = max(1, min(B, CHUNK_BYTES // (L * L * 4)))

        def approx():
            p = preds.detach().requires_grad_(True)
            F.approxndcg_loss(p, labels, alpha=ALPHA, presort=True, couple_batch=False).backward()
            return p.grad

        for fn in (approx, approx):
            fn()
        for metric in METRICS:
            for opt_ideal in (True, False):
                for top_k in (None, 10):
                    def fused():
                        p = preds.detach().requires_grad_(True)
                        loss, parts = F.smooth_metric_objective(p, labels, metric, alpha=ALPHA, top_k=top_k, opt_ideal=opt_ideal, max_label=4.0,
                                                                return_parts=True)
                        loss.backward()
                        return parts["loss_q"], p.grad

                    def eager():
                        out = [eager_loss_grad(metric, preds[lo:lo + chunk], labels[lo:lo + chunk], top_k, opt_ideal) for lo in range(0, B, chunk)]
                        return tuple(torch.cat([o[k] for o in out]) for k in range(3))

                    lq_f, g_f = fused()
                    lq_e, g_e, same = eager()
                    torch.cuda.synchronize()
                    agree = {k: float((a[same] - b[same]).abs().max() / b[same].abs().max().clamp_min(1e-30)) for k, (a, b) in
                             dict(loss_q=(lq_f, lq_e), grad=(g_f, g_e)).items()}
                    agree["queries_compared"] = int(same.sum())
                    assert agree["loss_q"] <= 1e-4 and agree["grad"] <= 1e-4 and agree["queries_compared"] >= 0.9 * B, (metric, opt_ideal, top_k, agree)
                    variants = {"fused_ms": fused, "approxndcg_per_query_ms": approx, "eager_batched_ms": eager}
                    for fn in variants.values():
                        fn(); fn()
                    torch.cuda.synchronize()
                    rounds = {k: [] for k in variants}
                    for _ in range(ROUNDS):
                        for k, fn in variants.items():
                            inner = 1 if k.startswith("eager") else 10
                            rounds[k].append(timed(lambda: [fn() for _ in range(inner)]) / inner)
                    med = {k: statistics.median(v) for k, v in rounds.items()}
                    pairs = B * L * L
                    cycles = pair_issue_cycles(L)
                    peak = NUM_SIMD * PEAK_CLOCK_HZ * 64.0 / cycles
                    row = dict(metric=metric, opt_ideal=opt_ideal, top_k=top_k, B=B, L=L, alpha=ALPHA, eager_chunk_queries=chunk, rounds=ROUNDS,
                               median_ms=med, all_rounds_ms=rounds, max_rel_diff_fused_vs_eager=agree,
                               ratio_to_approxndcg=med["fused_ms"] / med["approxndcg_per_query_ms"],
                               speedup_vs_eager_batched=med["eager_batched_ms"] / med["fused_ms"],
                               ordered_pairs=pairs, pairs_per_s=pairs / (med["fused_ms"] * 1e-3),
                               valu_issue_bound=dict(vector_instructions_per_unordered_pair=ISSUE_PER_UNORDERED_PAIR[L][0],
                                                     transcendentals_per_unordered_pair=ISSUE_PER_UNORDERED_PAIR[L][1],
                                                     cycles_per_ordered_pair=cycles, peak_pairs_per_s=peak, bound_ms=pairs / peak * 1e3,
                                                     share_of_bound=(pairs / peak * 1e3) / med["fused_ms"]),
                               note="fused_ms and approxndcg_per_query_ms are whole autograd calls: the kernel, the loss-slot sum or finish kernel, "
                                    "the output allocations and the backward's scaling")
                    print(json.dumps({k: row[k] for k in ("metric", "opt_ideal", "top_k", "B", "L", "median_ms", "ratio_to_approxndcg",
                                                          "speedup_vs_eager_batched", "pairs_per_s")}), flush=True)
                    results.append(row)
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, shapes=results), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_smooth_metric.json"))
