#!/usr/bin/env python3
"""Times the IRFGAN kernels (csrc/irfgan.hip) at 1024 x 128 and 256 x 1024 (queries x documents):
  (a) functional.irfgan_pair_sample — the true pairs and the fake pairs of a batch, one launch, nothing of size n x n;
  (b) the two loss launches of a pair step with their backward, functional.irfgan_loss 'PAIR_D' and 'PAIR_G' (f_div GAN);
against an eager-torch BATCHED restatement, on the same GPU, of the reference's n x n route (ptranking/ltr_adversarial/util/pair_sampling.py
:26-77, :111-122; pairwise/irfgan_pair.py:127-130, :143-166): the P x n weight matrix and torch.multinomial over it, the n x n matrix of
Bradley-Terry probabilities, torch.bernoulli over it, torch.multinomial over the flattened mask; and the two losses through the literal
conjugate_f(activation_f(v)) with autograd (the reference runs these lines once per QUERY; the batched restatement is the faster thing to
compare against).

    python profiles/prof_irfgan.py profiles/mi355x_irfgan.json

Full lists, the first P = 8 documents relevant with labels 2 and 1, S = 5.  Every shape is timed in PROCS fresh processes, one after the
other; inside a process every variant is warmed up on the shape it is timed on, then timed with device events over whole calls, ROUNDS
times with the variants alternating inside a round.  The JSON keeps every round of every process and reports the median of the processes'
medians.
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1024, 128), (256, 1024))
P, S = 8, 5
PROCS, ROUNDS, INNER = 3, 5, 5


def child(B, L):
    import torch
    import ptranking_amd.functional as F

    assert torch.cuda.is_available(), "prof_irfgan.py measures on the GPU only"
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
    labels = torch.zeros((B, L), device=dev)
    labels[:, :P // 2], labels[:, P // 2:P] = 2.0, 1.0
    num_pos = torch.full((B,), P, dtype=torch.int32, device=dev)
    d_sel = torch.randn((B, 4 * S), device=dev, generator=gen)
    seed = [0]

    def next_seed():
        seed[0] += 1
        return seed[0]

    def sample():
        return F.irfgan_pair_sample(g_preds, labels, num_pos, S, seed=next_seed())

    disc = 1.0 / torch.log2(2.0 + torch.arange(L, device=dev))

    def sample_torch():
        w = torch.clamp_min(labels[:, :P, None] - labels[:, None, :], 0.0) * disc[None, None, :] * disc[None, :P, None]
        true = torch.multinomial(w.view(B, -1), S, replacement=True)
        probs = torch.sigmoid(g_preds[:, :, None] - g_preds[:, None, :])
        fake = torch.multinomial(torch.bernoulli(probs).view(B, -1), S, replacement=True)
        return torch.div(true, L, rounding_mode='floor'), true % L, torch.div(fake, L, rounding_mode='floor'), fake % L

    th, tt, fh, ft, nsel = sample()
    assert int(nsel.min()) == S

    def losses():
        x = d_sel.detach().requires_grad_(True)
        F.irfgan_loss(x, nsel, "PAIR_D", "GAN").backward()
        p = g_preds.detach().requires_grad_(True)
        F.irfgan_loss(p, nsel, "PAIR_G", "GAN", d_fake=d_sel[:, 2 * S:], idx_a=fh, idx_b=ft).backward()
        return x.grad, p.grad

    def losses_torch():
        act = lambda v: -torch.log(1.0 + torch.exp(-v))                     # f_divergence.py:69-74
        conj = lambda t: -torch.log(1.0 - torch.exp(t))
        x = d_sel.detach().requires_grad_(True)
        (torch.mean(conj(act(x[:, 2 * S:3 * S] - x[:, 3 * S:])), dim=1) - torch.mean(act(x[:, :S] - x[:, S:2 * S]), dim=1)).sum().backward()
        p = g_preds.detach().requires_grad_(True)
        probs = torch.sigmoid(p[:, :, None] - p[:, None, :])                 # the generator's loss reads the n x n matrix again (:162)
        picked = probs.view(B, -1).gather(1, fh * L + ft)
        c = conj(act(d_sel[:, 2 * S:3 * S] - d_sel[:, 3 * S:]))
        (-torch.mean(torch.log(picked) * c, dim=1)).sum().backward()
        return x.grad, p.grad

    variants = dict(pair_sample_ms=sample, pair_sample_torch_ms=sample_torch, pair_losses_ms=losses, pair_losses_torch_ms=losses_torch)
    for fn in variants.values():
        fn(); fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            rounds[k].append(timed(fn))
    print(json.dumps(dict(B=B, L=L, device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds_ms=rounds)), flush=True)


def main(out_path):
    shapes = []
    for B, L in SHAPES:
        procs = []
        for _ in range(PROCS):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(B), str(L)], capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                raise SystemExit(f"child {B} x {L} failed ({out.returncode}):\n{out.stderr[-2000:]}")
            procs.append(json.loads(out.stdout.strip().splitlines()[-1]))
        med = {k: statistics.median(statistics.median(p["rounds_ms"][k]) for p in procs) for k in procs[0]["rounds_ms"]}
        row = dict(B=B, L=L, num_pos=P, samples_per_query=S, f_div="GAN", processes=PROCS, rounds=ROUNDS, calls_per_round=INNER, median_ms=med,
                   pair_sample_vs_torch=med["pair_sample_torch_ms"] / med["pair_sample_ms"],
                   pair_losses_vs_torch=med["pair_losses_torch_ms"] / med["pair_losses_ms"], all_rounds_ms=[p["rounds_ms"] for p in procs],
                   note="whole calls: kernels, loss-slot sums, output allocations, autograd's backward scaling; the torch side is a BATCHED eager "
                        "restatement of the reference's per-query n x n route")
        print(json.dumps({k: row[k] for k in ("B", "L", "median_ms", "pair_sample_vs_torch", "pair_losses_vs_torch")}), flush=True)
        shapes.append(row)
    with open(out_path, "w") as f:
        json.dump(dict(device=procs[0]["device"], torch=procs[0]["torch"], shapes=shapes), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_irfgan.json"))
