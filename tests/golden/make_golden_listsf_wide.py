#!/usr/bin/env python3
"""Golden fixtures for attention heads WIDER than 128 in the listwise scorer (listsf), produced by RUNNING THE REFERENCE's modules on
CPU (build container only), in the manner of make_golden_listsf.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_listsf_wide.py

Reference entry points exercised (ptranking/base/list_ranker.py):
  :176-254  MultiheadAttention.forward, eval mode, ONE head over 136 (MSLR-WEB30K) and 176 features
  :284-378  ListNeuralRanker.ini_listsf / forward: 136 features, n_heads = 1, one AttnDIN encoder layer, ff_dims = [16], no batch norm
For every case the fixture holds the module's state_dict, the input, the output and the gradients of  sum(output * R)  (R a fixed random
tensor) with respect to the input and to every parameter — autograd of the reference itself.  The head of 350 (700 Yahoo! features, 2
heads) is NOT here: one 700 x 700 layer is 2 MB of weights; tests/test_listsf_wide_gpu.py pins it against float64 instead.

The cases go into one archive each — listsf_wide.npz (head 136), listsf_wide_d176.npz, listsf_wide_ranker.npz — because their dense
F x F weights and weight gradients do not compress and no committed file may exceed 1 MiB; load() merges them.  write_npz() gives every
archive member a fixed date, so the same arrays give the same bytes (tests/test_listsf_wide_cpu.py rewrites the committed archives
through it and compares the files).
"""
import io
import os
import sys
import zipfile

import numpy as np

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = {"mhsa/c0_d136": "listsf_wide.npz", "mhsa/c1_d176": "listsf_wide_d176.npz", "listsf/AttnDIN_d136": "listsf_wide_ranker.npz"}   # case -> archive
SEED = 352
MHSA_CASES = [(2, 10, 136, 1), (2, 21, 176, 1)]                  # (B, L, F, heads)
RANKER = dict(num_features=136, ff_dims=[16], AF='R', TL_AF='GE', apply_tl_af=False, BN=False, bn_type='BN2', bn_affine=False, n_heads=1,
              encoder_layers=1, encoder_type='AttnDIN')


def write_npz(path, store):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(store):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.array(store[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def split(store):
    """{archive name: {key: array}} of a merged store."""
    parts = {f: {} for f in FILES.values()}
    for k, v in store.items():
        parts[FILES["/".join(k.split("/")[:2])]][k] = v
    return parts


def load():
    """The merged fixture: {family: {case: {field (may contain '/'): array}}}."""
    fams = {}
    for f in FILES.values():
        z = np.load(os.path.join(HERE, f), allow_pickle=False)
        for key in z.files:
            fam, case, field = key.split("/", 2)
            fams.setdefault(fam, {}).setdefault(case, {})[field] = z[key]
    return fams


def main():
    ref = os.environ.get("PTRANKING_REF") or "/root/reference"         # a wildltr/ptranking checkout
    if not os.path.isdir(ref):
        raise SystemExit(f"no wildltr/ptranking checkout at {ref} (set PTRANKING_REF)")
    sys.path.insert(0, ref)
    import torch
    from ptranking.base.list_ranker import MultiheadAttention, ListNeuralRanker

    torch.manual_seed(SEED)
    store = {}
    for ci, (B, L, F, H) in enumerate(MHSA_CASES):
        m = MultiheadAttention(hid_dim=F, n_heads=H, dropout=0.1, device="cpu")
        m.eval()
        x, R = torch.randn(B, L, F).requires_grad_(True), torch.randn(B, L, F)
        y = m(x)
        (y * R).sum().backward()
        tag = f"mhsa/c{ci}_d{F // H}"
        store.update({f"{tag}/x": x.detach().numpy(), f"{tag}/R": R.numpy(), f"{tag}/y": y.detach().numpy(), f"{tag}/dx": x.grad.numpy(),
                      f"{tag}/n_heads": np.int32(H)})
        for k, v in m.state_dict().items():
            store[f"{tag}/sd/{k}"] = v.numpy()
        for k, p in m.named_parameters():
            store[f"{tag}/grad/{k}"] = p.grad.numpy()
    sf = dict(sf_id='listsf', opt='Adagrad', lr=0.001, listsf=dict(RANKER))
    r = ListNeuralRanker(sf_para_dict=sf, gpu=False, device="cpu")
    r.init()
    r.eval_mode()
    x, R = torch.randn(2, 9, RANKER["num_features"]), torch.randn(2, 9)
    preds = r.forward(x)
    (preds * R).sum().backward()
    tag = "listsf/AttnDIN_d136"
    store.update({f"{tag}/x": x.numpy(), f"{tag}/R": R.numpy(), f"{tag}/preds": preds.detach().numpy()})
    for part in ("head_ffnns", "encoder", "tail_ffnns"):
        for k, v in r.list_sf[part].state_dict().items():
            store[f"{tag}/sd/{part}/{k}"] = v.numpy()
        for k, p in r.list_sf[part].named_parameters():
            store[f"{tag}/grad/{part}/{k}"] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    for f, part in split(store).items():
        write_npz(os.path.join(HERE, f), part)
        print(f"{f}: {len(part)} arrays, {os.path.getsize(os.path.join(HERE, f))} bytes, torch {torch.__version__}")


if __name__ == "__main__":
    main()
