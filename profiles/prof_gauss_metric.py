#!/usr/bin/env python3
"""Times the Gaussian expected-rank metric objectives (csrc/gaussmetric.hip, ptr_gaussmetric_fwd_bwd) against
  (a) the reference's composition (get_expected_rank, prob_utils.py:62-80, then metric_as_opt_objective.py, then autograd in the means and
      the variances) restated in eager torch on the same GPU, batched in chunks whose [chunk, L, L] intermediate fits in memory;
  (b) smooth_metric_objective (csrc/smoothmetric.hip) at the same shape: the same objective on sigmoid ranks, one exponential per unordered
      pair and pass out of a register ring, where this kernel's ring spends an erfcx and two exponentials per unordered pair and carries two
      gradients with compensated sums.

    python profiles/prof_gauss_metric.py profiles/mi355x_gauss_metric.json

Shapes: B = 4096 at L = 128 and B = 1024 at L = 512, full lists, means 2 N(0, 1), variances U(0.05, 1.05), every metric in both modes with
top_k in {None, 10}.  Every variant is warmed up on the shape it is timed on and timed with device events over whole autograd calls, ROUNDS
times with the variants alternating inside a round; the JSON keeps every round and reports the median.  The one condition: the fused call is
not slower than the eager restatement at either shape.  Hardware constants come from ptranking_amd/peaks.py only.
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
CHUNK_BYTES = 1 << 30

# Issue count per UNORDERED pair over both passes of the ring kernel: (vector instructions, of which quarter-rate transcendentals), counted in
# the gfx950 code hipcc emits for gauss_ring_kernel (-O3): the bodies of the two 31-step ring loops divided by the pair evaluations of a step
# (DPT^2).  The bodies are straight-line (erfcx's range cases are computed and selected, so every counted instruction issues).
# L = 128 (DPT 2): (287 + 165) / 4 with (18 + 8) / 4 transcendentals; L = 512 (DPT 8): (4887 + 2506) / 64 with (318 + 128) / 64.
# An ordered pair is half.
ISSUE_PER_UNORDERED_PAIR = {128: (113.0, 6.5), 512: (115.5, 7.0)}


def pair_issue_cycles(L):
    valu, trans = ISSUE_PER_UNORDERED_PAIR[L]
    return 0.5 * ((valu - trans) * VALU_CYCLES_PER_INSTR + trans * TRANS_CYCLES_PER_INSTR)      # per ORDERED pair


def eager_loss_grad(metric, mus, vars_, labels, top_k, opt_ideal, max_label=4.0):
    """The reference's composition for a batch [b, L] of full lists + autograd -> (loss_q, grad_mu, grad_var, order [b, L]).  Each query
    divides by its own ideal value (the kernel's contract is the reference one query at a time)."""
    import torch
    m, v = mus.detach().requires_grad_(True), vars_.detach().requires_grad_(True)
    y = labels
    b, n = m.shape
    phi = 0.5 * torch.erfc((m.unsqueeze(2) - m.unsqueeze(1)) / torch.sqrt(2.0 * (v.unsqueeze(2) + v.unsqueeze(1))))
    r = (torch.triu(phi, diagonal=1) + torch.tril(phi, diagonal=-1)).sum(2) + 1.0
    nat = torch.arange(n, dtype=m.dtype, device=m.device).view(1, -1) + 1.0
    k = n if not top_k else min(top_k, n)
    kdiv = n if not top_k else top_k
    yb = y.clamp(0, 1)
    idx = torch.arange(n, device=m.device).expand(b, n)
    if opt_ideal:
        rr, yy, bb = r, y, yb
    else:
        rr, idx = torch.sort(r, dim=1, stable=True)
        yy, bb = torch.gather(y, 1, idx), torch.gather(yb, 1, idx)
    gains = torch.pow(2.0, yy) - 1.0
    keep = torch.ones(b, dtype=torch.bool, device=m.device)
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
    return -torch.where(keep, val.detach(), torch.zeros_like(val)), m.grad, v.grad, idx


def main(out_path):
    import numpy as np
    import torch
    import ptranking_amd.functional as F

    assert torch.cuda.is_available(), "prof_gauss_metric.py measures on the GPU only"
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
        mus = torch.from_numpy((0.6 * y + 2.0 * rng.standard_normal((B, L))).astype(np.float32)).to(dev)
        vars_ = torch.from_numpy(rng.uniform(0.05, 1.05, (B, L)).astype(np.float32)).to(dev)
        labels = torch.from_numpy(y.copy()).to(dev)
        chunk = max(1, min(B, CHUNK_BYTES // (L * L * 4)))
        for metric in METRICS:
            for opt_ideal in (True, False):
                for top_k in (None, 10):
                    def fused():
                        m, v = mus.detach().requires_grad_(True), vars_.detach().requires_grad_(True)
                        loss, parts = F.gaussian_metric_objective(m, v, labels, metric, top_k=top_k, opt_ideal=opt_ideal, max_label=4.0,
                                                                  return_parts=True)
                        loss.backward()
                        return parts["loss_q"], m.grad, v.grad, parts["pos"]

                    def smooth():
                        p = mus.detach().requires_grad_(True)
                        F.smooth_metric_objective(p, labels, metric, alpha=10.0, top_k=top_k, opt_ideal=opt_ideal, max_label=4.0).backward()
                        return p.grad

                    def eager():
                        out = [eager_loss_grad(metric, mus[lo:lo + chunk], vars_[lo:lo + chunk], labels[lo:lo + chunk], top_k, opt_ideal)
                               for lo in range(0, B, chunk)]
                        return tuple(torch.cat([o[k] for o in out]) for k in range(4))

                    lq_f, gm_f, gv_f, pos_f = fused()
                    lq_e, gm_e, gv_e, idx_e = eager()
                    torch.cuda.synchronize()
                    # the re-sorted forms sort fp32 ranks that two evaluations round differently: compare the queries whose orders agree
                    same = (torch.argsort(pos_f.long(), dim=1) == idx_e).all(1)
                    agree = {k: float((a[same] - b[same]).abs().max() / b[same].abs().max().clamp_min(1e-30)) for k, (a, b) in
                             dict(loss_q=(lq_f, lq_e), grad_mu=(gm_f, gm_e), grad_var=(gv_f, gv_e)).items()}
                    agree["queries_compared"] = int(same.sum())
                    assert all(agree[k] <= 1e-4 for k in ("loss_q", "grad_mu", "grad_var")) and agree["queries_compared"] >= 0.9 * B, \
                        (metric, opt_ideal, top_k, agree)
                    variants = {"fused_ms": fused, "smooth_metric_ms": smooth, "eager_batched_ms": eager}
                    for fn in variants.values():
                        fn(); fn()
                    torch.cuda.synchronize()
                    rounds = {k: [] for k in variants}
                    for _ in range(ROUNDS):
                        for k, fn in variants.items():
                            inner = 1 if k.startswith("eager") else 10
                            rounds[k].append(timed(lambda: [fn() for _ in range(inner)]) / inner)
                    med = {k: statistics.median(v) for k, v in rounds.items()}
                    assert med["fused_ms"] <= med["eager_batched_ms"], (metric, opt_ideal, top_k, B, L, med)
                    pairs = B * L * L
                    cycles = pair_issue_cycles(L)
                    peak = NUM_SIMD * PEAK_CLOCK_HZ * 64.0 / cycles
                    row = dict(metric=metric, opt_ideal=opt_ideal, top_k=top_k, B=B, L=L, eager_chunk_queries=chunk, rounds=ROUNDS,
                               median_ms=med, all_rounds_ms=rounds, max_rel_diff_fused_vs_eager=agree,
                               ratio_to_smooth_metric=med["fused_ms"] / med["smooth_metric_ms"],
                               speedup_vs_eager_batched=med["eager_batched_ms"] / med["fused_ms"],
                               ordered_pairs=pairs, pairs_per_s=pairs / (med["fused_ms"] * 1e-3),
                               valu_issue_bound=dict(vector_instructions_per_unordered_pair=ISSUE_PER_UNORDERED_PAIR[L][0],
                                                     transcendentals_per_unordered_pair=ISSUE_PER_UNORDERED_PAIR[L][1],
                                                     cycles_per_ordered_pair=cycles, peak_pairs_per_s=peak, bound_ms=pairs / peak * 1e3,
                                                     share_of_bound=(pairs / peak * 1e3) / med["fused_ms"]),
                               note="fused_ms and smooth_metric_ms are whole autograd calls: the kernel, the loss-slot sum, the output "
                                    "allocations and the backward's scaling")
                    print(json.dumps({k: row[k] for k in ("metric", "opt_ideal", "top_k", "B", "L", "median_ms", "ratio_to_smooth_metric",
                                                          "speedup_vs_eager_batched", "pairs_per_s")}), flush=True)
                    results.append(row)
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, shapes=results), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_gauss_metric.json"))
