#!/usr/bin/env python3
"""Times the diversification kernels (csrc/diversity.hip) against the only alternative a user has without them: the reference's op sequence
(ptranking/ltr_diversification/score_and_sort/daletor.py:9-38, forward + autograd backward) restated in eager torch on the same GPU —
looped over queries as the reference runs it, and batched in chunks whose [chunk, T, L, L] intermediate fits in memory.

    python profiles/prof_diversity.py profiles/mi355x_diversity_kernels.json

Shapes: B = 4096, L = 128, T = 8 and B = 1024, L = 512, T = 16 (rt = 10, alpha = 0.5, top_k = 10, the reference's subtopic cut-off).  Every
variant is warmed up on the shape it is timed on, timed with device events over whole launches, ROUNDS times with the variants alternating
inside a round; the JSON keeps every round and reports the median.  The per-query loop is timed on LOOP_QUERIES queries and scaled to B
(named `*_extrapolated_ms`).  Results are compared before anything is timed.  Hardware constants come from ptranking_amd/peaks.py only.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ptranking_amd.peaks import NUM_SIMD, PEAK_CLOCK_HZ, TRANS_CYCLES_PER_INSTR, VALU_CYCLES_PER_INSTR  # noqa: E402

SHAPES = [(4096, 128, 8), (1024, 512, 16)]
KS = [1, 5, 10, 20]
ROUNDS = 7
LOOP_QUERIES = 32
CHUNK_BYTES = 1 << 30            # budget of one [chunk, T, L, L] fp32 intermediate of the batched eager form
RT, ALPHA, TOP_K = 10.0, 0.5, 10


def pair_issue_cycles(T):
    """Least issue cycles of one ORDERED pair (i, j) through both passes of the thread-per-document form, counted from the arithmetic:
    pass 1: s_j - s_i, |.| * rt, exp, 1 + e, rcp, e * r, select, pi += y, T cover FMAs          -> 6 + T VALU, 2 transcendental
    pass 2: the same indicator pair (6 VALU, 2 transcendental), y (1 - y), A_j - A_i, 2 T dot FMAs, acc FMA -> 9 + 2 T VALU"""
    valu = (6 + T) + (9 + 2 * T)
    return valu * VALU_CYCLES_PER_INSTR + 4 * TRANS_CYCLES_PER_INSTR


def eager_loss_grad(preds, rele, rt=RT, alpha=ALPHA, top_k=TOP_K):
    """daletor.py:9-38 for a batch [b, L] / [b, T, L] (torch.sigmoid is the numerically robust sigmoid) + autograd -> (loss_q, grad)."""
    import torch
    p = preds.detach().requires_grad_(True)
    diffs = p.unsqueeze(2) - p.unsqueeze(1)
    ind = torch.sigmoid(rt * diffs.transpose(1, 2))                                   # [b, L, L]
    pis = ind.sum(dim=2) + 0.5
    cover = (ind.unsqueeze(1) * rele.unsqueeze(2)).sum(dim=3) - rele / 2.0            # [b, T, L] via [b, T, L, L]
    gains = rele * torch.pow(1.0 - alpha, cover) / torch.log2(1.0 + pis).unsqueeze(1)
    loss_q = -gains.sum(dim=2)[:, :top_k].sum(dim=1)
    loss_q.sum().backward()
    return loss_q.detach(), p.grad


def eager_metrics(preds, rele, ks, alpha=ALPHA, max_label=1.0):
    """ranker.py:413-475 + diversity_metric.py for a batch of full lists: sort, gather, the three metrics at ks."""
    import torch
    B, T, L = rele.shape
    kmax = max(ks)
    idx = torch.sort(preds, dim=1, descending=True)[1]
    sys_R = torch.gather(rele, 2, idx.unsqueeze(1).expand(-1, T, -1))[:, :, :kmax]
    ideal_R = rele[:, :, :kmax]
    disc = torch.log2(torch.arange(kmax, device=preds.device, dtype=torch.float32) + 2.0)
    rr = 1.0 / (torch.arange(kmax, device=preds.device, dtype=torch.float32) + 1.0)

    def adcg(R):
        prior = torch.cumsum(R, dim=2) - R
        return torch.cumsum((torch.pow(1.0 - alpha, prior) * R / disc).sum(dim=1), dim=1)

    def err(R):
        satis = (torch.pow(2.0, R) - 1.0) / 2.0 ** max_label
        uns = torch.cumprod(1.0 - satis, dim=2)
        casc = torch.cat([torch.ones_like(uns[:, :, :1]), uns[:, :, :-1]], dim=2)
        return torch.cumsum(satis * casc * rr, dim=2).sum(dim=1) / T

    sel = torch.tensor([k - 1 for k in ks], device=preds.device)
    ds, di, es, ei = adcg(sys_R)[:, sel], adcg(ideal_R)[:, sel], err(sys_R)[:, sel], err(ideal_R)[:, sel]
    return torch.where(di > 0, ds / di, torch.zeros_like(ds)), es, torch.where(ei > 0, es / ei, torch.zeros_like(es))


def main(out_path):
    import torch
    import ptranking_amd.functional as F

    assert torch.cuda.is_available(), "prof_diversity.py measures on the GPU only"
    dev = torch.device("cuda:0")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    results = []
    for B, L, T in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(137 + L)
        preds = torch.randn(B, L, generator=g).to(dev)
        rele = (torch.rand(B, T, L, generator=g) < 0.1).float().to(dev)
        chunk = max(1, min(B, CHUNK_BYTES // (T * L * L * 4)))

        def fused():
            return F.alphadcg_loss(preds, rele, rt=RT, alpha=ALPHA, top_k=TOP_K, return_loss_q=True)

        def fused_grad():
            p = preds.detach().requires_grad_(True)
            F.alphadcg_loss(p, rele, rt=RT, alpha=ALPHA, top_k=TOP_K).backward()
            return p.grad

        def eager_batched():
            out = [eager_loss_grad(preds[lo:lo + chunk], rele[lo:lo + chunk]) for lo in range(0, B, chunk)]
            return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])

        def eager_loop(nq=LOOP_QUERIES):
            for q in range(nq):
                eager_loss_grad(preds[q:q + 1], rele[q:q + 1])

        def fused_metrics():
            return F.div_metrics_at_ks(preds, rele, KS, alpha=ALPHA, max_label=1.0)

        def eager_metrics_batched():
            return eager_metrics(preds, rele, KS)

        # same results first (fp32 summation order differs: 1e-4 relative of the largest entry is far above it and far below a wrong kernel)
        lq_e, g_e = eager_batched()
        _, lq_f = fused()
        g_f = fused_grad()
        a_f, e_f, n_f, _ = fused_metrics()
        a_e, e_e, n_e = eager_metrics_batched()
        torch.cuda.synchronize()
        checks = {"loss_q": (lq_f, lq_e), "grad": (g_f, g_e), "andcg": (a_f, a_e), "err_ia": (e_f, e_e), "nerr_ia": (n_f, n_e)}
        agree = {k: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for k, (a, b) in checks.items()}
        assert all(v <= 1e-4 for v in agree.values()), agree

        variants = {"fused_loss_ms": fused, "eager_batched_loss_ms": eager_batched, "eager_loop_loss_ms": eager_loop,
                    "fused_metrics_ms": fused_metrics, "eager_batched_metrics_ms": eager_metrics_batched}
        for fn in variants.values():          # warm-up on the timed shapes
            fn(); fn()
        torch.cuda.synchronize()
        rounds = {k: [] for k in variants}
        for _ in range(ROUNDS):
            for k, fn in variants.items():
                inner = 20 if k.startswith("fused") else 1
                rounds[k].append(timed(lambda: [fn() for _ in range(inner)]) / inner)
        med = {k: statistics.median(v) for k, v in rounds.items()}
        pairs = B * L * L
        peak_pairs_per_s = NUM_SIMD * PEAK_CLOCK_HZ * 64.0 / pair_issue_cycles(T)
        row = dict(B=B, L=L, T=T, rt=RT, alpha=ALPHA, top_k=TOP_K, ks=KS, eager_chunk_queries=chunk, rounds=ROUNDS, loop_queries=LOOP_QUERIES,
                   median_ms=med, all_rounds_ms=rounds, max_rel_diff_fused_vs_eager=agree,
                   eager_loop_loss_extrapolated_ms=med["eager_loop_loss_ms"] * B / LOOP_QUERIES,
                   speedup_vs_eager_batched=med["eager_batched_loss_ms"] / med["fused_loss_ms"],
                   metrics_speedup_vs_eager_batched=med["eager_batched_metrics_ms"] / med["fused_metrics_ms"],
                   ordered_pairs=pairs, pairs_per_s=pairs / (med["fused_loss_ms"] * 1e-3),
                   valu_issue_bound=dict(cycles_per_ordered_pair=pair_issue_cycles(T), peak_pairs_per_s=peak_pairs_per_s,
                                         bound_ms=pairs / peak_pairs_per_s * 1e3,
                                         share_of_bound=(pairs / peak_pairs_per_s * 1e3) / med["fused_loss_ms"]),
                   note="fused_loss_ms includes the ptr_sum_f32 launch over loss_q and the output allocations of functional.alphadcg_loss")
        print(json.dumps({k: row[k] for k in ("B", "L", "T", "median_ms", "speedup_vs_eager_batched", "metrics_speedup_vs_eager_batched",
                                              "pairs_per_s")}), flush=True)
        assert med["fused_loss_ms"] <= med["eager_batched_loss_ms"], "the fused loss launch is slower than batched eager torch"
        assert med["fused_metrics_ms"] <= med["eager_batched_metrics_ms"], "the fused metric launch is slower than batched eager torch"
        results.append(row)
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, shapes=results), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_diversity_kernels.json"))
