#!/usr/bin/env python3
"""Times forward + backward of the two rectangular attention calls of one IMSAB (csrc/xattn.hip: the n_induce = 32 inducing points attend
to the L documents — short queries, Q shared with batch stride 0 — and the documents attend to the 32 results — short keys) against the
project's own square core (ptr_mhsa_forward / ptr_mhsa_backward, with the dS scratch listsf.py would give it) at the same B = 256, F = 136,
H = 2 and L in {128, 512, 1024}, on the same commit.

    python profiles/prof_setrank.py profiles/mi355x_setrank.json

Entry points are called through the C ABI on preallocated buffers (no autograd, no allocation inside the timed region).  Each L runs in a
FRESH process; inside it every variant is warmed up on its shape, then timed with device events over INNER whole calls, ROUNDS times with
the variants alternating inside a round.  The JSON keeps every round and reports medians.  The expectation — the pair is cheaper than the
square core from L = 512 upward — comes from the operation counts (L M against L^2) alone; the JSON records whether it held.
"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, F, H, M = 256, 136, 2, 32
LS = (128, 512, 1024)
ROUNDS, INNER = 7, 5


def child(L):
    import torch
    from ptranking_amd import _lib, listsf
    dev = torch.device("cuda:0")
    st = _lib.current_stream(dev)
    gen = torch.Generator(device=dev).manual_seed(L)
    r = lambda *s: torch.randn(s, device=dev, generator=gen)
    e = lambda *s: torch.empty(s, device=dev)
    p = _lib.ptr

    def xattn(Q, qbs, kv, Lq, Lk):
        """forward + backward closure of one rectangular call on the packed K|V projection kv [B, Lk, 2F]"""
        O, lse, dvec, dO = e(B, Lq, F), e(B * H * Lq), e(B * H * Lq), r(B, Lq, F)
        dQ, dkv = e(B, Lq, F), torch.empty_like(kv)
        head = (p(Q), F, C.c_int64(qbs), listsf._voff(kv, 0), listsf._voff(kv, F), 2 * F, None, None, B, Lq, Lk, F, H)

        def run():
            _lib.call("ptr_xattn_forward", *head, p(O), p(lse), st)
            _lib.call("ptr_xattn_backward", *head, p(O), p(dO), p(lse), p(dvec), p(dQ), listsf._voff(dkv, 0), listsf._voff(dkv, F), st)
        return run

    induce = xattn(r(M, F), 0, r(B, L, 2 * F), M, L)            # MAB(I, X): short queries
    docs = xattn(r(B, L, F), L * F, r(B, M, 2 * F), L, M)       # MAB(X, H): short keys

    qkv, dqkv = r(B, L, 3 * F), e(B, L, 3 * F)
    O, lse, dvec, dO = e(B, L, F), e(B * H * L), e(B * H * L), r(B, L, F)
    ds_ws = listsf._ds_scratch(B, H, L, dev)
    ptrs, gptrs = [listsf._voff(qkv, i * F) for i in range(3)], [listsf._voff(dqkv, i * F) for i in range(3)]

    def square():
        _lib.call("ptr_mhsa_forward", *ptrs, 3 * F, None, B, L, F, H, C.c_float(0.0), C.c_uint64(0), 0, p(O), p(lse), st)
        _lib.call("ptr_mhsa_backward", *ptrs, 3 * F, p(O), p(dO), p(lse), None, B, L, F, H, C.c_float(0.0), C.c_uint64(0), 0, p(dvec), *gptrs,
                  p(ds_ws), st)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / INNER

    variants = dict(induce_ms=induce, docs_ms=docs, square_ms=square)
    for fn in variants.values():
        fn(); fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            rounds[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    pair = med["induce_ms"] + med["docs_ms"]
    print(json.dumps(dict(B=B, L=L, F=F, heads=H, n_induce=M, median_ms=med, pair_ms=pair, square_over_pair=med["square_ms"] / pair,
                          square_ds_scratch=ds_ws is not None, rounds=ROUNDS, calls_per_round=INNER, all_rounds_ms=rounds,
                          device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)


def main(out_path):
    rows = []
    for L in LS:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(L)], check=True, stdout=subprocess.PIPE, text=True).stdout
        row = json.loads(out.strip().splitlines()[-1])
        print(json.dumps({k: row[k] for k in ("L", "median_ms", "pair_ms", "square_over_pair")}), flush=True)
        rows.append(row)
    held = all(r["square_over_pair"] > 1.0 for r in rows if r["L"] >= 512)
    with open(out_path, "w") as f:
        json.dump(dict(expectation="the rectangular pair is cheaper than the square core from L = 512 upward (from operation counts alone)",
                       expectation_held=held, shapes=rows), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_setrank.json"))
