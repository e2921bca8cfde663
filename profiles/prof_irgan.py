#!/usr/bin/env python3
"""Times the IRGAN point and pair kernels (csrc/irgan.hip):
  (a) the three entry points at 4096 x 128 — functional.irgan_sample in its three modes, functional.irgan_point_generator with its backward,
      functional.irgan_selected in its five forms with their backward;
  (b) one generator step of each machine, from the players' scores to the gradient with respect to the generator's scores (the scorer
      passes are the same on both sides and stay out), against an eager-torch BATCHED restatement of the same step on the same GPU:
      IRGAN_Point  softmax, the importance distribution, torch.multinomial(replacement=True) of 5 P draws, gather, reward, loss, backward
      IRGAN_Pair   sigmoid, torch.multinomial(replacement=False) of V negatives, gather, reward, loss, backward
      (the reference itself runs these lines once per QUERY; the batched restatement is the faster thing to compare against).

    python profiles/prof_irgan.py profiles/mi355x_irgan.json

Full lists, P = 8 relevant documents per query (the batched torch.multinomial needs one draw count per batch), S = 5, T = 0.5.  Every
variant is warmed up on the shape it is timed on and timed with device events over whole calls, ROUNDS times with the variants alternating
inside a round; the JSON keeps every round and reports the median.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, L, P, S, T, LAM, DPP = 4096, 128, 8, 5, 0.5, 0.5, 5
ROUNDS = 7
INNER = 10


def main(out_path):
    import torch
    import ptranking_amd.functional as F

    assert torch.cuda.is_available(), "prof_irgan.py measures on the GPU only"
    dev = torch.device("cuda:0")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / INNER

    gen = torch.Generator(device=dev).manual_seed(137)
    g_preds = torch.rand((B, L), device=dev, generator=gen)                  # apply_tl_af: the generator ends in a sigmoid
    d_preds = torch.rand((B, L), device=dev, generator=gen)
    d_sel = torch.randn((B, 2 * S), device=dev, generator=gen)
    num_pos = torch.full((B,), P, dtype=torch.int32, device=dev)
    seed = [0]

    def next_seed():
        seed[0] += 1
        return seed[0]

    variants = {}
    for mode in F.IRGAN_SAMPLE_MODES:
        variants[f"sample_{mode}_ms"] = lambda mode=mode: F.irgan_sample(g_preds, num_pos, S, mode, temperature=T, seed=next_seed())

    def point_step():
        p = g_preds.detach().requires_grad_(True)
        F.irgan_point_generator(p, d_preds, num_pos, temperature=T, lam=LAM, draws_per_pos=DPP, seed=next_seed()).backward()
        return p.grad

    def point_step_torch():
        p = g_preds.detach().requires_grad_(True)
        probs = torch.softmax(p / T, dim=1)
        prob_is = probs * (1.0 - LAM)
        prob_is = torch.cat([prob_is[:, :P] + LAM / P, prob_is[:, P:]], dim=1)
        choose = torch.multinomial(prob_is.detach(), DPP * P, replacement=True)
        pc, qc = probs.gather(1, choose), prob_is.gather(1, choose)
        reward = 2.0 * (d_preds.gather(1, choose) - 0.5)
        (-(torch.log(pc) * reward * (pc / qc)).mean(dim=1)).sum().backward()
        return p.grad

    pos_neg = F.irgan_sample(g_preds, num_pos, S, "PAIR_G", temperature=T, seed=1)
    for mode in F.IRGAN_SELECTED_MODES:
        def sel(mode=mode):
            if mode.startswith("PAIR_G"):
                x = g_preds.detach().requires_grad_(True)
                F.irgan_selected(x, pos_neg[2], mode, d_sel=d_sel, neg_idx=pos_neg[1], temperature=T).backward()
            else:
                x = d_sel.detach().requires_grad_(True)
                F.irgan_selected(x, pos_neg[2], mode).backward()
            return x.grad
        variants[f"selected_{mode}_ms"] = sel

    def pair_step():
        p = g_preds.detach().requires_grad_(True)
        _, neg, nsel = F.irgan_sample(p, num_pos, S, "PAIR_G", temperature=T, seed=next_seed())
        F.irgan_selected(p, nsel, "PAIR_G_SVM", d_sel=d_sel, neg_idx=neg, temperature=T).backward()
        return p.grad

    def pair_step_torch():
        p = g_preds.detach().requires_grad_(True)
        probs = torch.sigmoid(p / T)
        neg = torch.multinomial(probs.detach(), S, replacement=False)
        reward = torch.sigmoid(torch.clamp_min(1.0 - (d_sel[:, :S] - d_sel[:, S:]), 0.0))
        (-(torch.log(probs.gather(1, neg)) * reward).mean(dim=1)).sum().backward()
        return p.grad

    variants.update(point_generator_step_ms=point_step, point_generator_step_torch_ms=point_step_torch,
                    pair_generator_step_ms=pair_step, pair_generator_step_torch_ms=pair_step_torch)
    for fn in variants.values():
        fn(); fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            rounds[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    row = dict(B=B, L=L, num_pos=P, samples_per_query=S, temperature=T, rounds=ROUNDS, calls_per_round=INNER, median_ms=med, all_rounds_ms=rounds,
               point_generator_step_vs_torch=med["point_generator_step_torch_ms"] / med["point_generator_step_ms"],
               pair_generator_step_vs_torch=med["pair_generator_step_torch_ms"] / med["pair_generator_step_ms"],
               note="whole calls: kernels, loss-slot sums, output allocations, autograd's backward scaling; the torch side is a BATCHED eager "
                    "restatement of the reference's per-query lines, scorer passes excluded on both sides")
    print(json.dumps({k: row[k] for k in ("B", "L", "median_ms", "point_generator_step_vs_torch", "pair_generator_step_vs_torch")}), flush=True)
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, shapes=[row]), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_irgan.json"))
