#!/usr/bin/env python3
"""Times the DivProbRanker loss kernel (csrc/divprob.hip) against the only alternative a user has without it: the reference's op sequences
(ptranking/ltr_diversification/score_and_sort/div_prob_ranker.py:29-202, forward + autograd backward) restated in eager torch on the same
GPU — looped over queries as the reference runs it, and batched in chunks whose [chunk, T, L, L] intermediate fits in memory.

    python profiles/prof_divprob.py profiles/mi355x_divprob_kernels.json

Shapes: B = 4096, L = 128, T = 8 and B = 1024, L = 512, T = 16, each of the four objectives (beta = 0.5, top_k = 10 on the reference's
subtopic axis for aNDCG and on documents for nERR-IA, max_label = 1, norm = True).  Means N(0, 1), variances U(0.5, 2).  Before anything is timed the fused results are compared, over EVERY query, with the same eager code run
in float64 on the GPU — for the pairwise objectives in the form the kernel documents (`check=True`: each logarithm from log_ndtr, clamped
at -100, tests/divprob_ref.py `stable`), because the reference's fp32 `P = 1 - erfc(x) / 2` rounds to 1 from |x| = 3.8 on and a few of the
B L^2 pairs reach that: its logarithm then sits at the clamp and its backward divides by the 1e-12 floor.  What is TIMED is the reference's
own fp32 arithmetic.  Every variant is
warmed up on the shape it is timed on, timed with device events over whole launches, ROUNDS times with the variants alternating inside a
round; the JSON keeps every round and reports the median.  The per-query loop is timed on LOOP_QUERIES queries and scaled to B (named
`*_extrapolated_ms`).  Hardware constants come from ptranking_amd/peaks.py only.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ptranking_amd.peaks import NUM_SIMD, PEAK_CLOCK_HZ, TRANS_CYCLES_PER_INSTR, VALU_CYCLES_PER_INSTR  # noqa: E402

SHAPES = [(4096, 128, 8), (1024, 512, 16)]
OBJECTIVES = ("aNDCG", "nERR-IA", "PairCLS", "LambdaPairCLS")
ROUNDS = 7
LOOP_QUERIES = 32
CHUNK_BYTES = 1 << 30            # budget of one [chunk, T, L, L] fp32 intermediate of the batched eager form
BETA, TOP_K = 0.5, 10

# The kernel's issue count per ORDERED pair (i, j): (vector instructions, of which quarter-rate transcendentals), counted in the gfx950 code
# hipcc emits for csrc/divprob.hip (-O3) — the instructions between the label and the backward branch of each pair loop (both passes of the two
# SuperSoft objectives added up), divided by the unroll factor 2.  Keyed by the subtopic tile TP (T = 8 -> 8, T = 16 -> 16); the group size
# changes no loop body.  The library functions (expf, erfcxf, logf, log1pf) are inlined and counted as emitted, both sides of their branches.
ISSUE_PER_PAIR = {8: {"aNDCG": (116.5, 6.0), "nERR-IA": (95.0, 6.0), "PairCLS": (243.0, 8.0), "LambdaPairCLS": (268.0, 8.0)},
                  16: {"aNDCG": (136.5, 6.0), "nERR-IA": (95.0, 6.0), "PairCLS": (267.0, 8.0), "LambdaPairCLS": (316.0, 8.0)}}


def pair_issue_cycles(objective, T):
    valu, trans = ISSUE_PER_PAIR[8 if T <= 8 else 16][objective]
    return (valu - trans) * VALU_CYCLES_PER_INSTR + trans * TRANS_CYCLES_PER_INSTR


def eager_loss_grad(objective, mus, vars_, rele, beta=BETA, top_k=TOP_K, check=False):
    """div_prob_ranker.py:29-202 (opt_ideal) for a batch [b, L] / [b, T, L] + autograd -> (loss_q, grad_mu, grad_var), in the precision of
    the inputs.  check: the pairwise terms as -[t log P + (1 - t) log Q] with log P = log_ndtr(sqrt(2) x), log Q = log_ndtr(-sqrt(2) x), each
    clamped at -100 — what the kernel computes — instead of F.binary_cross_entropy on 1 - erfc(x) / 2."""
    import torch
    import torch.nn.functional as F
    m, v = mus.detach().requires_grad_(True), vars_.detach().requires_grad_(True)
    b, T, L = rele.shape
    x = (m.unsqueeze(2) - m.unsqueeze(1)) / torch.sqrt(2.0 * (v.unsqueeze(2) + v.unsqueeze(1)))                          # [b, L, L]
    phi = 0.5 * torch.erfc(x)
    if objective in ("aNDCG", "nERR-IA"):
        phi0 = torch.triu(phi, diagonal=1) + torch.tril(phi, diagonal=-1)
        ranks = phi0.sum(dim=2) + 1.0
        if objective == "aNDCG":
            cover = (phi0.unsqueeze(1) * rele.unsqueeze(2)).sum(dim=3)                                                     # via [b, T, L, L]
            gains = rele * torch.pow(1.0 - beta, cover) / torch.log2(1.0 + ranks).unsqueeze(1)
            loss_q = -gains.sum(dim=2)[:, :top_k].sum(dim=1)
        else:
            satis = (torch.pow(2.0, rele[:, :, :top_k]) - 1.0) / 2.0
            uns = torch.cumprod(1.0 - satis, dim=2)
            casc = torch.cat([torch.ones_like(uns[:, :, :1]), uns[:, :, :-1]], dim=2)
            loss_q = -(satis * casc / ranks[:, :top_k].unsqueeze(1)).sum(dim=(1, 2))
    else:
        tb = (0.5 * (1.0 + torch.clamp(rele.unsqueeze(3) - rele.unsqueeze(2), -1.0, 1.0))).mean(dim=1)                      # via [b, T, L, L]
        weight = None
        if objective == "LambdaPairCLS":
            prior = torch.cumsum(rele, dim=2) - rele
            focus = torch.pow(1.0 - beta, prior)
            disc = 1.0 / torch.log2(torch.arange(L, device=rele.device, dtype=torch.float32) + 2.0)
            gains = torch.pow(2.0, rele) - 1.0
            gd = gains.unsqueeze(3) - gains.unsqueeze(2)
            h = focus * disc
            delta = torch.abs((gd * h.unsqueeze(3)).sum(dim=1) - (gd * h.unsqueeze(2)).sum(dim=1))
            ideal = (focus * rele * disc).sum(dim=(1, 2))
            weight = torch.triu(delta / ideal.view(-1, 1, 1), diagonal=1)
        if check:
            root2 = 2.0 ** 0.5
            log_p = torch.clamp(torch.special.log_ndtr(root2 * x), min=-100.0)
            log_q = torch.clamp(torch.special.log_ndtr(-root2 * x), min=-100.0)
            terms = torch.triu(-(tb * log_p + (1.0 - tb) * log_q), diagonal=1)
            loss_q = (terms if weight is None else terms * weight).sum(dim=(1, 2))
        else:
            bce = F.binary_cross_entropy(input=torch.triu(1.0 - phi, diagonal=1), target=torch.triu(tb, diagonal=1), weight=weight,
                                         reduction="none")
            loss_q = bce.sum(dim=(1, 2))
    loss_q.sum().backward()
    return loss_q.detach(), m.grad, v.grad


def main(out_path):
    import torch
    import ptranking_amd.functional as F

    assert torch.cuda.is_available(), "prof_divprob.py measures on the GPU only"
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
        mus = torch.randn(B, L, generator=g).to(dev)
        vars_ = (0.5 + 1.5 * torch.rand(B, L, generator=g)).to(dev)
        rele = (torch.rand(B, T, L, generator=g) < 0.1).float()
        rele[:, 0, 0] = 1.0                                     # every query has a relevant document: the reference divides by the ideal value
        rele = rele.to(dev)
        chunk = max(1, min(B, CHUNK_BYTES // (T * L * L * 4)))
        for objective in OBJECTIVES:
            top_axis = "reference" if objective == "aNDCG" else "documents"

            def fused():
                return F.divprob_loss(mus, vars_, rele, objective, beta=BETA, top_k=TOP_K, top_k_axis=top_axis, max_label=1.0, norm=True,
                                      return_loss_q=True)

            def fused_grad():
                m, v = mus.detach().requires_grad_(True), vars_.detach().requires_grad_(True)
                F.divprob_loss(m, v, rele, objective, beta=BETA, top_k=TOP_K, top_k_axis=top_axis, max_label=1.0, norm=True).backward()
                return m.grad, v.grad

            def eager_batched():
                out = [eager_loss_grad(objective, mus[lo:lo + chunk], vars_[lo:lo + chunk], rele[lo:lo + chunk]) for lo in range(0, B, chunk)]
                return tuple(torch.cat([o[k] for o in out]) for k in range(3))

            def eager_loop(nq=LOOP_QUERIES):
                for q in range(nq):
                    eager_loss_grad(objective, mus[q:q + 1], vars_[q:q + 1], rele[q:q + 1])

            def eager_check():
                half = max(1, chunk // 2)
                out = [eager_loss_grad(objective, mus[lo:lo + half].double(), vars_[lo:lo + half].double(), rele[lo:lo + half].double(), check=True)
                       for lo in range(0, B, half)]
                return tuple(torch.cat([o[k] for o in out]) for k in range(3))

            # same results first, over every query, against float64 (1e-4 relative of the largest entry is far above fp32 rounding and far
            # below a wrong kernel)
            lq_e, gm_e, gv_e = eager_check()
            _, lq_f = fused()
            gm_f, gv_f = fused_grad()
            torch.cuda.synchronize()
            checks = {"loss_q": (lq_f, lq_e), "grad_mu": (gm_f, gm_e), "grad_var": (gv_f, gv_e)}
            agree = {k: float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30)) for k, (a, b) in checks.items()}
            assert all(x <= 1e-4 for x in agree.values()), (objective, agree)

            variants = {"fused_loss_ms": fused, "eager_batched_loss_ms": eager_batched, "eager_loop_loss_ms": eager_loop}
            for fn in variants.values():          # warm-up on the timed shapes
                fn(); fn()
            torch.cuda.synchronize()
            rounds = {k: [] for k in variants}
            for _ in range(ROUNDS):
                for k, fn in variants.items():
                    inner = 10 if k.startswith("fused") else 1
                    rounds[k].append(timed(lambda: [fn() for _ in range(inner)]) / inner)
            med = {k: statistics.median(x) for k, x in rounds.items()}
            pairs = B * L * L
            cycles = pair_issue_cycles(objective, T)
            peak_pairs_per_s = NUM_SIMD * PEAK_CLOCK_HZ * 64.0 / cycles
            row = dict(objective=objective, B=B, L=L, T=T, beta=BETA, top_k=TOP_K, top_k_axis=top_axis, eager_chunk_queries=chunk, rounds=ROUNDS,
                       loop_queries=LOOP_QUERIES, median_ms=med, all_rounds_ms=rounds, max_rel_diff_fused_vs_float64_eager=agree,
                       eager_loop_loss_extrapolated_ms=med["eager_loop_loss_ms"] * B / LOOP_QUERIES,
                       speedup_vs_eager_batched=med["eager_batched_loss_ms"] / med["fused_loss_ms"],
                       ordered_pairs=pairs, pairs_per_s=pairs / (med["fused_loss_ms"] * 1e-3),
                       valu_issue_bound=dict(vector_instructions_per_ordered_pair=ISSUE_PER_PAIR[8 if T <= 8 else 16][objective][0],
                                             transcendentals_per_ordered_pair=ISSUE_PER_PAIR[8 if T <= 8 else 16][objective][1],
                                             cycles_per_ordered_pair=cycles, peak_pairs_per_s=peak_pairs_per_s,
                                             bound_ms=pairs / peak_pairs_per_s * 1e3,
                                             share_of_bound=(pairs / peak_pairs_per_s * 1e3) / med["fused_loss_ms"]),
                       note="fused_loss_ms includes the ptr_sum_f32 launch over loss_q and the output allocations of functional.divprob_loss")
            print(json.dumps({k: row[k] for k in ("objective", "B", "L", "T", "median_ms", "speedup_vs_eager_batched", "pairs_per_s")}), flush=True)
            results.append(row)
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, shapes=results), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_divprob_kernels.json"))
