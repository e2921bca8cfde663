"""Entry-point time of ptr_neuralndcg_fwd_bwd beside the same rule as fp32 eager torch with autograd, on the same GPU -> profiles/mi355x_neuralndcg.json.

    python profiles/prof_neuralndcg.py            # parent: fresh child processes, the two sides alternated, three rounds per shape
Each child warms up, then times `reps` calls between two device events (loss and gradient, as a training step needs them)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((4096, 128), (1024, 256))
ITERS, TAU = 50, 1.0


def eager(s, y):
    """tests/neuralndcg_ref.py batched over [B, L] in fp32 (full lists, the whole list as the cut-off)."""
    import torch
    B, L = s.shape
    g = torch.pow(2.0, y) - 1.0
    d = 1.0 / torch.log2(torch.arange(L, device=s.device, dtype=s.dtype) + 2.0)
    idcg = (torch.sort(g, dim=1, descending=True).values * d).sum(1)
    Bj = (s[:, :, None] - s[:, None, :]).abs().sum(2)
    c = L - 1 - 2 * torch.arange(L, device=s.device, dtype=s.dtype)
    P = torch.softmax((c[None, :, None] * s[:, None, :] - Bj[:, None, :]) / TAU, dim=2)
    for _ in range(ITERS):
        P = P / P.sum(dim=1, keepdim=True).clamp(min=1e-10)
        P = P / P.sum(dim=2, keepdim=True).clamp(min=1e-10)
    return -((d[None, :] * (P * g[:, None, :]).sum(2)).sum(1) / idcg).sum()


def child(mode, B, L, reps):
    import torch
    import ptranking_amd.functional as F
    g = torch.Generator().manual_seed(1)
    s = torch.randn(B, L, generator=g).cuda().requires_grad_(True)
    y = torch.randint(0, 5, (B, L), generator=g).float().cuda()
    y[:, 0] = 1.0
    step = (lambda: F.neuralndcg_loss(s, y, temperature=TAU, iters=ITERS)) if mode == "fused" else (lambda: eager(s, y))
    for _ in range(2):
        s.grad = None
        step().backward()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        s.grad = None
        loss = step()
        loss.backward()
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps(dict(ms=e0.elapsed_time(e1) / reps, loss=float(loss), peak_bytes=torch.cuda.max_memory_allocated())))


def main():
    if len(sys.argv) > 1:
        return child(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    import ptranking_amd.functional as F
    out = dict(device="MI355X", iters=ITERS, tau=TAU, what="entry-point time per launch, loss and gradient; fresh processes, alternated", shapes=[])
    for B, L in SHAPES:
        rec = dict(B=B, L=L, form=F.neuralndcg_form(L, ITERS), fused_ms=[], eager_ms=[])
        for _ in range(3):
            for mode, reps in (("fused", 10), ("eager", 3)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, str(B), str(L), str(reps)], capture_output=True, text=True, timeout=280)
                if r.returncode != 0:
                    raise SystemExit(f"{mode} {B}x{L} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
                res = json.loads(r.stdout.strip().splitlines()[-1])
                rec[f"{mode}_ms"].append(round(res["ms"], 4))
                rec[f"{mode}_loss"], rec[f"{mode}_peak_bytes"] = res["loss"], res["peak_bytes"]
        rec["lds_bytes_per_query"], rec["ws_bytes_per_query"] = rec["form"]["lds_bytes"], rec["form"]["ws_bytes"]
        out["shapes"].append(rec)
        print(rec, flush=True)
    dest = os.environ.get("PROF_OUT", os.path.join(ROOT, "profiles", "mi355x_neuralndcg.json"))
    with open(dest, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
