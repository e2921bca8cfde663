#!/usr/bin/env python3
"""Times the list machines' kernels (csrc/adlist.hip) at 4096 x 128 and 1024 x 512 (queries x documents), S = 10 samples per query, top_k = 10
and the whole list:
  (a) functional.adlist_sample — the standard and the generated rankings of a batch, one launch;
  (b) functional.adlist_loss 'D' with its backward — the discriminator's Plackett-Luce loss on those rankings (family IRGAN);
  (c) functional.adlist_loss 'G' with its backward — the generator's step: draws, ranks, softmax, the PL of the top probabilities, the reward
      -lp (repTrick True, dropLog False: finite for whole lists, where exp(1 - lp) overflows in any fp32) and the gradient, one launch;
against an eager-torch BATCHED restatement on the same GPU of the reference's per-query route (ptranking/ltr_adversarial/listwise/
irgan_list.py:230-291, :315-341, :344-395): torch.rand, the Gumbel transform, softmax and torch.sort over [B, S, L], gathers, logcumsumexp
and autograd.  (The reference runs these lines once per QUERY with a Python loop per sample; the batched restatement is the faster thing
to compare against.)

    python profiles/prof_adlist.py profiles/mi355x_adlist.json

Full lists, labels 0 .. 4.  Before anything is timed the two sides are compared over EVERY query on shared uniforms: the rankings index
for index, the per-query losses to 1e-4 of their scale (a ranking whose two closest keys lie within an ulp of the two sides' logarithms
may differ: with 512 keys a few in a hundred do; the fraction is recorded, must stay below 5e-2, and such queries leave the loss check).
Every variant is warmed up on the shape it is timed on, then timed with device events over whole calls, ROUNDS times with the variants
alternating inside a round; the JSON keeps every round and reports the medians.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((4096, 128), (1024, 512))
S, TOP_KS, T = 10, (10, None), 0.5
ROUNDS, INNER = 7, 3
EPS = 1e-20


def measure(B, L, K):
    import torch
    import ptranking_amd.functional as F

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(137)
    g_preds = torch.randn((B, L), device=dev, generator=gen)
    d_preds = torch.rand((B, L), device=dev, generator=gen)                   # the discriminator ends in a sigmoid
    labels = torch.randint(0, 5, (B, L), device=dev, generator=gen).float()
    Kq = L if K is None else K
    seed = [0]

    def next_seed():
        seed[0] += 1
        return seed[0]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / INNER

    def gumbel(u):
        return -torch.log(-torch.log(u + EPS) + EPS)

    def pl(v):                                                                # log_ranking_prob_Plackett_Luce over the last axis
        return (v - torch.flip(torch.logcumsumexp(torch.flip(v, dims=[-1]), dim=-1), dims=[-1])).sum(-1)

    # ---- the two sides on shared uniforms, every query
    unif = F.adlist_uniforms(B, L, S, seed=99)

    def sample_torch(u=None):
        u = torch.rand((B, 2 * S, L), device=dev) if u is None else u
        gen_idx = torch.sort(g_preds[:, None, :] + gumbel(u[:, :S]), dim=-1, descending=True, stable=True)[1][:, :, :Kq]
        std_idx = torch.sort(labels[:, None, :].double() + u[:, S:].double(), dim=-1, descending=True, stable=True)[1][:, :, :Kq]   # integer labels
        return std_idx, gen_idx

    std, gen_idx, kq = F.adlist_sample(g_preds, labels, S, top_k=K, unif=unif)
    std_t, gen_t = sample_torch(unif)
    differ = dict(std=float((std != std_t).any(-1).float().mean()), gen=float((gen_idx != gen_t).any(-1).float().mean()))
    assert differ["std"] == 0.0 and differ["gen"] < 5e-2, differ

    def d_torch(x, std_i, gen_i):
        xs = x[:, None, :].expand(-1, S, -1)
        return -(pl(xs.gather(2, std_i)).sum(1) + torch.log(1.0 - pl(xs.gather(2, gen_i))).sum(1))      # irgan_list.py:336-337

    def g_torch(x, u=None):
        u = torch.rand((B, S, L), device=dev) if u is None else u
        y = torch.softmax((x[:, None, :] + gumbel(u)) / T, dim=-1)
        probs, inds = torch.sort(y, dim=-1, descending=True, stable=True)
        probs, inds = probs[:, :, :Kq], inds[:, :, :Kq]
        reward = -pl(d_preds[:, None, :].expand(-1, S, -1).gather(2, inds))
        return (pl(probs) * reward.detach()).mean(1), inds

    _, parts = F.adlist_loss(d_preds, "D", std_idx=std, gen_idx=gen_idx, kq=kq, top_k=K, return_parts=True)
    ref = d_torch(d_preds, std, gen_idx)
    err_d = float(((parts["loss_q"] - ref).abs() / ref.abs().clamp(min=1.0)).max())
    _, parts = F.adlist_loss(g_preds, "G", reward="neg_lp", d_preds=d_preds, samples_per_query=S, top_k=K, temperature=T, unif=unif[:, :S].contiguous(),
                             return_parts=True)
    ref, inds = g_torch(g_preds, unif[:, :S])
    same = (parts["gen_idx"] == inds).all(-1).all(-1)
    err_g = float(((parts["loss_q"] - ref).abs() / ref.abs().clamp(min=1.0))[same].max())
    assert err_d < 1e-4 and err_g < 1e-4 and float((~same).float().mean()) < 5e-2, (err_d, err_g, float((~same).float().mean()))

    # ---- timing: whole calls, the kernels on the counter hash, the torch side on torch.rand
    def k_sample():
        return F.adlist_sample(g_preds, labels, S, top_k=K, seed=next_seed())

    def k_d():
        x = d_preds.detach().requires_grad_(True)
        F.adlist_loss(x, "D", std_idx=std, gen_idx=gen_idx, kq=kq, top_k=K).backward()
        return x.grad

    def k_g():
        x = g_preds.detach().requires_grad_(True)
        F.adlist_loss(x, "G", reward="neg_lp", d_preds=d_preds, samples_per_query=S, top_k=K, temperature=T, seed=next_seed()).backward()
        return x.grad

    def t_d():
        x = d_preds.detach().requires_grad_(True)
        d_torch(x, std, gen_idx).sum().backward()
        return x.grad

    def t_g():
        x = g_preds.detach().requires_grad_(True)
        g_torch(x)[0].sum().backward()
        return x.grad

    variants = dict(sample_ms=k_sample, sample_torch_ms=sample_torch, d_ms=k_d, d_torch_ms=t_d, g_ms=k_g, g_torch_ms=t_g)
    for fn in variants.values():
        fn(); fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            rounds[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    return dict(B=B, L=L, samples_per_query=S, top_k=K, temperature=T, rounds=ROUNDS, calls_per_round=INNER, median_ms=med,
                sample_vs_torch=med["sample_torch_ms"] / med["sample_ms"], d_vs_torch=med["d_torch_ms"] / med["d_ms"],
                g_vs_torch=med["g_torch_ms"] / med["g_ms"], rankings_that_differ=differ, generator_rankings_that_differ=float((~same).float().mean()),
                loss_q_max_rel_err=dict(d=err_d, g=err_g), all_rounds_ms=rounds,
                note="whole calls: kernels, loss-slot sums, output allocations, autograd's backward scaling; the torch side is a BATCHED eager "
                     "restatement of the reference's per-query route")


def main(out_path):
    import torch
    assert torch.cuda.is_available(), "prof_adlist.py measures on the GPU only"
    shapes = []
    for B, L in SHAPES:
        for K in TOP_KS:
            row = measure(B, L, K)
            print(json.dumps({k: row[k] for k in ("B", "L", "top_k", "median_ms", "sample_vs_torch", "d_vs_torch", "g_vs_torch")}), flush=True)
            shapes.append(row)
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, shapes=shapes), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_adlist.json"))
