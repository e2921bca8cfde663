"""Entry-point time of ptr_fastsoftrank_fwd_bwd (loss, ranks and gradient) and, where it serves the shape (L <= 1024), of
functional.neuralndcg_loss for scale, on the same GPU -> profiles/mi355x_fastsoftrank.json.

    python profiles/prof_fastsoftrank.py            # parent: fresh child processes, three rounds per shape, the median of the process medians
    python profiles/prof_fastsoftrank.py B L        # one child: prints one JSON line
Each child warms up, then times five batches of launches between two device events each and reports their median.  eps = 0.3 (score range) / L,
the regime of mixed block sizes.  The cut-over between the wavefront and the workgroup form was chosen from the same child run on two
builds that differ in kFsrWaveMaxLen alone (PTR_LIB selects the library); their times are kept under "cutover" in the JSON."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((4096, 128), (1024, 1024), (256, 4096))


def child(B, L):
    import torch
    import ptranking_amd.functional as F
    g = torch.Generator().manual_seed(1)
    s = torch.randn(B, L, generator=g).cuda()
    y = torch.randint(0, 5, (B, L), generator=g).float().cuda()
    eps = 0.3 * float(s.max() - s.min()) / L
    x = s.clone().requires_grad_(True)

    def fsr():
        x.grad = None
        F.fastsoftrank_objective(x, y, eps=eps, objective="nDCG").backward()

    def neural():
        x.grad = None
        F.neuralndcg_loss(x, y, temperature=1.0, iters=50).backward()

    def timed(step, reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    out = dict(B=B, L=L, form=F.fastsoftrank_form(L))
    for name, step in (("fastsoftrank", fsr),) + ((("neuralndcg", neural),) if L <= F.NEURALNDCG_MAX_LEN else ()):
        for _ in range(3):
            step()
        reps = min(2000, max(5, int(120.0 / timed(step, 3))))
        out[name + "_ms"] = round(statistics.median(timed(step, reps) for _ in range(5)), 4)
    print(json.dumps(out))


def main():
    if len(sys.argv) > 2:
        return child(int(sys.argv[1]), int(sys.argv[2]))
    out = dict(device="MI355X", what="entry-point time per call, loss + ranks + gradient; fresh processes, median of three process medians", shapes=[])
    for B, L in SHAPES:
        runs = []
        for _ in range(3):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), str(B), str(L)], capture_output=True, text=True, timeout=280)
            if r.returncode != 0:
                raise SystemExit(f"{B}x{L} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        rec = dict(B=B, L=L, form=runs[0]["form"])
        for k in ("fastsoftrank_ms", "neuralndcg_ms"):
            if k in runs[0]:
                rec[k] = statistics.median(x[k] for x in runs)
        out["shapes"].append(rec)
        print(rec, flush=True)
    dest = os.environ.get("PROF_OUT", os.path.join(ROOT, "profiles", "mi355x_fastsoftrank.json"))
    with open(dest, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
