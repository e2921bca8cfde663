#!/usr/bin/env python3
"""Times the device Plackett-Luce sampler and the fused multi-sample MDPRank loss (csrc/plsample.hip) against the routes they replace:
  (a) the sampler alone (functional.sample_rankings_pl) against eager torch on the same GPU — 'PL': exp, clamp, torch.multinomial without
      replacement (one call per sample); 'STPL': torch.rand, two logarithms, torch.sort over [B * S, L];
  (b) the fused loss (functional.mdprank_sampled_loss + backward) against the MDPRank ranker's 'torch' sampler route: the eager sampling
      above, then ptr_mdprank_fwd_bwd through functional.mdprank_loss, and backward — once per sample.

    python profiles/prof_plsample.py profiles/mi355x_plsample.json

Shapes: B = 4096 at L = 128 and B = 1024 at L = 512, full lists, S in {1, 4}, both distributions (T = 1, top_k = 10, gamma = 1).  Every
variant is warmed up on the shape it is timed on and timed with device events over whole calls, ROUNDS times with the variants alternating
inside a round; the JSON keeps every round and reports the median.  HBM traffic of the fused call: preds + labels in, grad out (perm is not
requested).  Hardware constants come from ptranking_amd/peaks.py only.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ptranking_amd.peaks import HBM_PEAK_GBPS  # noqa: E402

SHAPES = [(4096, 128), (1024, 512)]
SAMPLES = (1, 4)
ROUNDS = 7
INNER = 10


def main(out_path):
    import numpy as np
    import torch
    import ptranking_amd.functional as F

    assert torch.cuda.is_available(), "prof_plsample.py measures on the GPU only"
    dev = torch.device("cuda:0")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / INNER

    def torch_sample(det, dist):
        """The ranker's 'torch' route (rankers.MDPRankLoss, full lists, T = 1) -> (perm, noise or None)."""
        if dist == "PL":
            probs = torch.exp(det - torch.max(det, dim=1, keepdim=True)[0]).clamp_min(1e-38)
            return torch.multinomial(probs, num_samples=det.size(1), replacement=False), None
        noise = -torch.log(-torch.log(torch.rand(det.size(), device=det.device) + 1e-20) + 1e-20)
        return torch.sort(det + noise, dim=1, descending=True)[1], noise

    results = []
    for B, L in SHAPES:
        rng = np.random.default_rng(137 + L)
        y = rng.choice(5, size=(B, L), p=[0.5147, 0.3250, 0.1339, 0.0183, 0.0081]).astype(np.float32)
        y[:, 0] = np.maximum(y[:, 0], 1)
        y = -np.sort(-y, axis=1)
        preds = torch.from_numpy((0.3 * y + 0.5 * rng.standard_normal((B, L))).astype(np.float32)).to(dev)
        labels = torch.from_numpy(y.copy()).to(dev)
        for dist in ("PL", "STPL"):
            for S in SAMPLES:
                seed = [0]

                def dev_sampler():
                    seed[0] += 1
                    return F.sample_rankings_pl(preds, samples=S, distribution=dist, seed=seed[0])

                def torch_sampler():
                    if dist == "PL":
                        return [torch_sample(preds, dist)[0] for _ in range(S)]
                    return torch_sample(preds.repeat_interleave(S, 0), dist)[0]

                def fused():
                    seed[0] += 1
                    p = preds.detach().requires_grad_(True)
                    F.mdprank_sampled_loss(p, labels, top_k=10, gamma=1.0, distribution=dist, samples=S, seed=seed[0]).backward()
                    return p.grad

                def parent():
                    p = preds.detach().requires_grad_(True)
                    total = 0.0
                    for _ in range(S):
                        with torch.no_grad():
                            perm, noise = torch_sample(p.detach(), dist)
                        total = total + F.mdprank_loss(p if noise is None else p + noise, labels, perm, top_k=10, gamma=1.0) / S
                    total.backward()
                    return p.grad

                variants = {"device_sampler_ms": dev_sampler, "torch_sampler_ms": torch_sampler, "fused_loss_ms": fused, "parent_route_ms": parent}
                for fn in variants.values():
                    fn(); fn()
                torch.cuda.synchronize()
                rounds = {k: [] for k in variants}
                for _ in range(ROUNDS):
                    for k, fn in variants.items():
                        rounds[k].append(timed(fn))
                med = {k: statistics.median(v) for k, v in rounds.items()}
                traffic = 3 * B * L * 4
                bound_ms = traffic / (HBM_PEAK_GBPS * 1e9) * 1e3
                row = dict(B=B, L=L, samples=S, distribution=dist, rounds=ROUNDS, calls_per_round=INNER, median_ms=med, all_rounds_ms=rounds,
                           sampler_speedup_vs_torch=med["torch_sampler_ms"] / med["device_sampler_ms"],
                           fused_speedup_vs_parent_route=med["parent_route_ms"] / med["fused_loss_ms"],
                           sampled_documents_per_s=dict(sampler=B * S * L / (med["device_sampler_ms"] * 1e-3), fused=B * S * L / (med["fused_loss_ms"] * 1e-3)),
                           hbm_bound=dict(bytes=traffic, bound_ms=bound_ms, share_of_bound=bound_ms / med["fused_loss_ms"]),
                           note="whole calls: kernel, loss-slot sum, output allocations, autograd's backward scaling; the parent route runs its "
                                "sampling and ptr_mdprank_fwd_bwd once per sample")
                print(json.dumps({k: row[k] for k in ("B", "L", "samples", "distribution", "median_ms", "sampler_speedup_vs_torch",
                                                      "fused_speedup_vs_parent_route")}), flush=True)
                results.append(row)
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, shapes=results), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")
    slow = [(r["B"], r["L"], r["distribution"]) for r in results if r["samples"] == 1 and r["fused_speedup_vs_parent_route"] < 1.0]
    assert not slow, f"the fused call is slower than the parent route at one sample per query: {slow}"


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_plsample.json"))
