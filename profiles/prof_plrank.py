"""Entry-point time of ptr_plrank_fwd_bwd beside the same rule as fp32 eager torch (Gumbel keys, one sort, cumulative sums, gathers and one
scatter_add over [B, S, L]) on the same GPU -> profiles/mi355x_plrank.json.

    python profiles/prof_plrank.py            # parent: fresh child processes, the two sides alternated, three rounds per shape
Each child warms up, sizes its window to about 0.6 s from a first estimate, then times that many calls between two device events (value and
gradient, as a training step needs them).  The ratio is reported, not gated."""
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((4096, 128, 32), (256, 512, 256))
TOP_K = 10


def eager(s, y, u):
    """tests/plrank_ref.py in fp32 on full lists, the draw included: nDCG@TOP_K reward -> (loss, grad)."""
    import torch
    B, S, L = u.shape
    perm = torch.sort(s[:, None, :] - torch.log(-torch.log(u + 1e-20) + 1e-20), dim=2, descending=True, stable=True).indices
    rho = torch.pow(2.0, y) - 1.0
    theta = torch.zeros(L, device=s.device)
    theta[:TOP_K] = 1.0 / torch.log2(torch.arange(TOP_K, device=s.device) + 2.0)
    theta = theta[None, :] / (torch.sort(rho, dim=1, descending=True).values * theta).sum(1, keepdim=True)
    e = torch.exp(s - s.max(1, keepdim=True).values)
    ey, ry = (torch.gather(x[:, None, :].expand(B, S, L), 2, perm) for x in (e, rho))
    suffix = lambda x: torch.flip(torch.cumsum(torch.flip(x, (2,)), 2), (2,))
    D, a = suffix(ey), theta[:, None, :] * ry
    PR = suffix(a)
    inv = torch.zeros_like(D)
    inv[:, :, :TOP_K] = 1.0 / D[:, :, :TOP_K]
    RI, DR = torch.cumsum(PR * inv, 2), torch.cumsum(theta[:, None, :] * inv, 2)
    g = torch.cat((PR[:, :, 1:], torch.zeros_like(PR[:, :, :1])), 2) + ey * (ry * DR - RI)
    grad = torch.zeros_like(s).scatter_add_(1, perm.reshape(B, S * L), g.reshape(B, S * L)) / -S
    return -a.sum() / S, grad


def child(mode, B, L, S):
    import torch
    import ptranking_amd.functional as F
    g = torch.Generator().manual_seed(1)
    s = torch.randn(B, L, generator=g).cuda()
    y = torch.randint(0, 5, (B, L), generator=g).float().cuda()
    y[:, 0] = 1.0
    u = F.pl_uniforms(B, L, samples=S, seed=3)
    fused = lambda: F.plrank_objective(s, y, samples=S, top_k=TOP_K, normalize=True, seed=3, return_parts=True)
    step = (lambda: fused()[0]) if mode == "fused" else (lambda: eager(s, y, u)[0])

    def timed(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            loss = step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, float(loss)

    for _ in range(3):
        step()
    reps = min(5000, max(10, math.ceil(600.0 / timed(5)[0])))
    ms, loss = timed(reps)
    print(json.dumps(dict(ms=ms, reps=reps, loss=loss, peak_bytes=torch.cuda.max_memory_allocated())))


def main():
    if len(sys.argv) > 1:
        return child(sys.argv[1], *map(int, sys.argv[2:5]))
    import ptranking_amd.functional as F
    out = dict(device="MI355X", top_k=TOP_K, what="entry-point time per call, value and gradient; fresh processes, alternated", shapes=[])
    for B, L, S in SHAPES:
        rec = dict(B=B, L=L, S=S, form=F.plrank_form(L, S), fused_ms=[], eager_ms=[])
        for _ in range(3):
            for mode in ("fused", "eager"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, str(B), str(L), str(S)], capture_output=True, text=True, timeout=280)
                if r.returncode != 0:
                    raise SystemExit(f"{mode} {B}x{L}x{S} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
                res = json.loads(r.stdout.strip().splitlines()[-1])
                rec[f"{mode}_ms"].append(round(res["ms"], 4))
                rec[f"{mode}_reps"], rec[f"{mode}_loss"], rec[f"{mode}_peak_bytes"] = res["reps"], res["loss"], res["peak_bytes"]
        rec["eager_over_fused"] = round(sorted(rec["eager_ms"])[1] / sorted(rec["fused_ms"])[1], 2)
        out["shapes"].append(rec)
        print(rec, flush=True)
    dest = os.environ.get("PROF_OUT", os.path.join(ROOT, "profiles", "mi355x_plrank.json"))
    with open(dest, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
