#!/usr/bin/env python3
"""Times the attention core on heads wider than 128 (csrc/listsf_wide.hip, through listsf.mhsa_core_packed) against the only alternative
a user had before them: the reference's op sequence (ptranking/base/list_ranker.py:216-240: split heads, Q K^T / sqrt(dh), softmax,
Dropout, . V, merge heads; forward + autograd backward) restated in eager torch on the same GPU.

    python profiles/prof_wide_heads.py profiles/mi355x_wide_head_attention.json

Shapes (B = 256 queries of L = 128 documents): F = 700 with 2 heads (the reference's stock listsf scorer on the Yahoo! sets: dh 350);
F = 256 with 1 head (wide, dh 256) beside 2 heads (the narrow D = 8 kernels, dh 128); F = 704 with 2 heads (dh 352, the limit) beside 8
heads (dh 88).  Inside the last two pairs the attention flops are identical, so fused wide / fused narrow is the price of the wide form.
Each shape runs in eval mode and with dropout 0.1 + ragged `lens` (eager: masked_fill of the padded keys + F.dropout).  Every variant is
warmed up on the shape it is timed on and timed forward + backward with device events, ROUNDS times with the variants alternating inside
a round; the JSON keeps every round and reports medians.  Results are compared before anything is timed.  The gate: at every WIDE shape
and mode the fused median may exceed the eager median by at most the fused path's own spread between rounds (max - min).
`share_of_fp32_mfma_peak` counts 7 GEMM units of 2 B H L^2 dh flops (forward S, P V; backward S, dP, dV, dK, dQ) against peaks.py; the wide
forms execute 8 with the stored dS (S is recomputed by the dK and by the dV launch), the narrow ones 7.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ptranking_amd.peaks import MFMA_F32_PEAK_TFLOPS  # noqa: E402

B, L = 256, 128
# (name, F, heads, gated against eager torch)
SHAPES = [("yahoo_700_h2", 700, 2, True), ("f256_h1", 256, 1, True), ("f256_h2", 256, 2, False), ("f704_h2", 704, 2, True),
          ("f704_h8", 704, 8, False)]
PAIRS = [("f256_h1", "f256_h2"), ("f704_h2", "f704_h8")]          # (wide, narrow) at identical attention flops
ROUNDS, INNER = 7, 5
P_DROP = 0.1
GEMM_UNITS = 7


def eager_core(Q, K, V, H, p, lens):
    """list_ranker.py:216-240 on the three projections [B, L, F]; lens: padded keys masked out of the softmax."""
    import torch
    import torch.nn.functional as Fn
    Bn, Ln, Fd = Q.shape
    dh = Fd // H
    q, k, v = (t.view(Bn, Ln, H, dh).permute(0, 2, 1, 3) for t in (Q, K, V))
    att = torch.matmul(q, k.permute(0, 1, 3, 2)) / dh ** 0.5
    if lens is not None:
        att = att.masked_fill(torch.arange(Ln, device=Q.device)[None, None, None, :] >= lens[:, None, None, None], float("-inf"))
    att = Fn.dropout(torch.softmax(att, dim=-1), p=p, training=p > 0)
    return torch.matmul(att, v).permute(0, 2, 1, 3).contiguous().view(Bn, Ln, Fd)


def main(out_path):
    import torch
    from ptranking_amd import listsf as LS

    assert torch.cuda.is_available(), "prof_wide_heads.py measures on the GPU only"
    dev = torch.device("cuda:0")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / INNER

    rows = {}
    for name, Fd, H, gated in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(137 + Fd + H)
        qkv = torch.randn(B, L, 3 * Fd, generator=g).to(dev).requires_grad_(True)
        Q, K, V = (qkv.detach()[..., i * Fd:(i + 1) * Fd].contiguous().requires_grad_(True) for i in range(3))
        dO = torch.randn(B, L, Fd, generator=g).to(dev)
        lens = torch.randint(L // 4, L + 1, (B,), generator=g).to(dev, torch.int32)

        def fused(p, ln):
            qkv.grad = None
            LS.mhsa_core_packed(qkv, H, p_drop=p, seed=11, site=0, lens=ln).backward(dO)
            return qkv.grad

        def eager(p, ln):
            Q.grad = K.grad = V.grad = None
            eager_core(Q, K, V, H, p, ln).backward(dO)
            return Q.grad

        # same results first (eval, with and without lens; dropout draws differ by generator): 1e-4 of the largest entry is far above the fp32
        # summation-order difference and far below a wrong kernel
        agree = {}
        for tag, ln in (("eval", None), ("lens", lens)):
            with torch.no_grad():
                o_f = LS.mhsa_core_packed(qkv.detach(), H, lens=ln)
                o_e = eager_core(Q.detach(), K.detach(), V.detach(), H, 0.0, ln)
            g_f = fused(0.0, ln).clone()
            eager(0.0, ln)
            g_e = torch.cat([Q.grad, K.grad, V.grad], dim=-1)
            agree[tag] = {"O": float((o_f - o_e).abs().max() / o_e.abs().max()), "dqkv": float((g_f - g_e).abs().max() / g_e.abs().max())}
        assert all(v <= 1e-4 for d in agree.values() for v in d.values()), agree

        variants = {"fused_eval_ms": lambda: fused(0.0, None), "eager_eval_ms": lambda: eager(0.0, None),
                    "fused_dropout_lens_ms": lambda: fused(P_DROP, lens), "eager_dropout_lens_ms": lambda: eager(P_DROP, lens)}
        for fn in variants.values():          # warm-up on the timed shapes
            fn(); fn()
        torch.cuda.synchronize()
        rounds = {k: [] for k in variants}
        for _ in range(ROUNDS):
            for k, fn in variants.items():
                rounds[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in rounds.items()}
        spread = {k: max(v) - min(v) for k, v in rounds.items()}
        flops = GEMM_UNITS * 2.0 * B * H * L * L * (Fd // H)
        row = dict(name=name, B=B, L=L, F=Fd, heads=H, head_dim=Fd // H, wide=Fd // H > 128, gated=gated, rounds=ROUNDS, inner=INNER,
                   median_ms=med, spread_ms=spread, all_rounds_ms=rounds, max_rel_diff_fused_vs_eager=agree,
                   speedup_vs_eager={m: med[f"eager_{m}_ms"] / med[f"fused_{m}_ms"] for m in ("eval", "dropout_lens")},
                   gemm_units_counted=GEMM_UNITS, flops_counted=flops,
                   share_of_fp32_mfma_peak={m: flops / (med[f"fused_{m}_ms"] * 1e-3) / (MFMA_F32_PEAK_TFLOPS * 1e12) for m in ("eval",)})
        print(json.dumps({k: row[k] for k in ("name", "head_dim", "median_ms", "spread_ms", "speedup_vs_eager", "share_of_fp32_mfma_peak")}), flush=True)
        rows[name] = row
    ratios = {f"{w}_over_{n}": {m: rows[w]["median_ms"][f"fused_{m}_ms"] / rows[n]["median_ms"][f"fused_{m}_ms"] for m in ("eval", "dropout_lens")}
              for w, n in PAIRS}
    print(json.dumps(dict(wide_over_narrow=ratios)), flush=True)
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, mfma_f32_peak_tflops=MFMA_F32_PEAK_TFLOPS,
                       wide_over_narrow=ratios, shapes=list(rows.values())), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")
    for row in rows.values():
        if row["gated"]:
            for m in ("eval", "dropout_lens"):
                fu, ea, sp = row["median_ms"][f"fused_{m}_ms"], row["median_ms"][f"eager_{m}_ms"], row["spread_ms"][f"fused_{m}_ms"]
                assert fu <= ea + sp, f"{row['name']} {m}: the fused path ({fu:.3f} ms, spread {sp:.3f}) is slower than eager torch ({ea:.3f} ms)"


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_wide_head_attention.json"))
