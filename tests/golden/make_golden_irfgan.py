"""Golden fixtures of the adversarial frame's IRFGAN point and pair machines: tests/golden/irfgan.npz.

Runs the reference's OWN f-divergence pairs — get_f_divergence_functions (ptranking/ltr_adversarial/util/f_divergence.py) for the eight
divergences that work ('JSW' raises TypeError at its first use) — through the four losses exactly as the two machines write them
(pointwise/irfgan_point.py:205, :213-216; pairwise/irfgan_pair.py:143-150, :157-166), with autograd, in float32 and in float64, and its own
get_weighted_clipped_pos_diffs (util/pair_sampling.py:26-50) on presorted label lists.

It imports wildltr/ptranking read-only from $PTRANKING_REF, default /root/reference.  Layout (<kind>/<family>/<field>), family 'moderate'
(|v| <= 3) or 'steep' (|v| up to 30, v the argument of activation_f), the cases of a family concatenated in the order of `shape`:
  point_d  shape [cases, 1] = V;  x_true, x_fake [sum V]
  pair_d   shape [cases, 1] = V;  th, tt, fh, ft [sum V] (the discriminator on true heads / true tails / fake heads / fake tails)
  point_g  shape [cases, 2] = (n, V), V <= n;  g_preds [sum n], idx [sum V] (distinct), d_fake [sum V]
  pair_g   shape [cases, 2] = (n, V);  g_preds [sum n], head, tail [sum V] (repeats and head = tail among them), d_head, d_tail [sum V]
  every kind: loss32 float32 / loss64 float64 [8, cases] and grad32 / grad64 [8, sum] in the order of DIVS; the gradient is with respect
  to the concatenation of the input fields in the order given above (generator kinds: g_preds alone).
  weights/<list>/labels [n], num_pos, w [P, n] float32.
The archive is written with fixed time stamps, so a second run reproduces the file byte for byte.
Usage: python tests/golden/make_golden_irfgan.py
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

REF = os.environ.get("PTRANKING_REF") or "/root/reference"
if not os.path.isdir(os.path.join(REF, "ptranking")):
    raise SystemExit(f"no wildltr/ptranking checkout at {REF} (set PTRANKING_REF)")
sys.path.insert(0, REF)

from ptranking.ltr_adversarial.util.f_divergence import get_f_divergence_functions   # noqa: E402
from ptranking.ltr_adversarial.util.pair_sampling import get_weighted_clipped_pos_diffs   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 137
DIVS = ("TVar", "KL", "RKL", "PC", "NC", "SH", "JS", "GAN")
NS = (1, 2, 3, 17, 64, 65, 130, 300)
VS = (1, 2, 5)
FAMILIES = {"moderate": 3.0, "steep": 30.0}
LABEL_LISTS = {"graded": [4, 3, 3, 1, 1, 1, 1, 0, 0, 0, 0, 0], "all_equal": [2, 2, 2, 2], "all_positive": [3, 2, 2, 1, 1], "ties": [2, 2, 1, 1, 0, 0, 0],
               "one": [1], "no_positive": [0, 0, 0], "binary_17": [1] * 5 + [0] * 12}


def point_d(f_div, dt, x_true, x_fake):
    activation_f, conjugate_f = get_f_divergence_functions(f_div)
    true_preds = torch.tensor(x_true[None], dtype=dt, requires_grad=True)
    fake_preds = torch.tensor(x_fake[None], dtype=dt, requires_grad=True)
    dis_loss = torch.mean(conjugate_f(activation_f(fake_preds))) - torch.mean(activation_f(true_preds))       # irfgan_point.py:205
    dis_loss.backward()
    return dis_loss, [true_preds.grad, fake_preds.grad]


def pair_d(f_div, dt, th, tt, fh, ft):
    activation_f, conjugate_f = get_f_divergence_functions(f_div)
    t = [torch.tensor(a[None], dtype=dt, requires_grad=True) for a in (th, tt, fh, ft)]
    true_preds = t[0] - t[1]                                                                                  # irfgan_pair.py:143-148
    fake_preds = t[2] - t[3]
    dis_loss = torch.mean(conjugate_f(activation_f(fake_preds))) - torch.mean(activation_f(true_preds))       # :150
    dis_loss.backward()
    return dis_loss, [a.grad for a in t]


def point_g(f_div, dt, g_preds, idx, d_fake):
    activation_f, conjugate_f = get_f_divergence_functions(f_div)
    batch_preds = torch.tensor(g_preds[None], dtype=dt, requires_grad=True)
    fake_inds = torch.from_numpy(idx)
    pred_probs = torch.nn.functional.softmax(batch_preds.view(-1), dim=0)            # :186 (torch.squeeze leaves a 0-d tensor at n = 1)
    d_fake_preds = conjugate_f(activation_f(torch.tensor(d_fake[None], dtype=dt)))   # :213-214
    ger_loss = -torch.mean((torch.log(pred_probs[fake_inds]) * d_fake_preds))       # :216
    ger_loss.backward()
    return ger_loss, [batch_preds.grad]


def pair_g(f_div, dt, g_preds, head, tail, d_head, d_tail):
    activation_f, conjugate_f = get_f_divergence_functions(f_div)
    batch_preds = torch.tensor(g_preds[None], dtype=dt, requires_grad=True)
    point_preds = batch_preds.view(-1)                                               # :118
    mat_diffs = torch.unsqueeze(point_preds, dim=1) - torch.unsqueeze(point_preds, dim=0)   # :127-128
    mat_bt_probs = torch.sigmoid(mat_diffs)
    d_fake_preds = conjugate_f(activation_f(torch.tensor(d_head[None], dtype=dt) - torch.tensor(d_tail[None], dtype=dt)))   # :157-159
    log_g_probs = torch.log(mat_bt_probs[torch.from_numpy(head), torch.from_numpy(tail)].view(1, -1))   # :162
    g_batch_loss = -torch.mean(log_g_probs * d_fake_preds)                           # :166
    g_batch_loss.backward()
    return g_batch_loss, [batch_preds.grad]


def spread(rng, size, bound):
    """fp32 values over (-bound, bound) with both ends reached."""
    v = rng.uniform(-bound, bound, size=size)
    if size >= 2:
        v[0], v[-1] = bound, -bound
    return v.astype(np.float32)


def head_tail(rng, size, bound):
    """fp32 (head, tail) with head - tail spread over (-bound, bound)."""
    tail = rng.uniform(-1.0, 1.0, size=size).astype(np.float32)
    return (tail + spread(rng, size, bound)).astype(np.float32), tail


def kind_cases(kind, bound, rng):
    """[(shape row, {field: array})] of one kind and family."""
    cases = []
    if kind in ("point_d", "pair_d"):
        for V in VS:
            if kind == "point_d":
                cases.append(((V,), dict(x_true=spread(rng, V, bound), x_fake=spread(rng, V, bound))))
            else:
                (th, tt), (fh, ft) = head_tail(rng, V, bound), head_tail(rng, V, bound)
                cases.append(((V,), dict(th=th, tt=tt, fh=fh, ft=ft)))
        return cases
    for n in NS:
        for V in VS:
            g = np.clip(1.5 * rng.standard_normal(n), -3.0, 3.0).astype(np.float32)
            if kind == "point_g":
                if V > n:
                    continue                                                         # torch.multinomial(replacement=False) of V <= P <= n
                cases.append(((n, V), dict(g_preds=g, idx=rng.permutation(n)[:V].astype(np.int64), d_fake=spread(rng, V, bound))))
            else:
                head, tail = rng.integers(0, n, size=V), rng.integers(0, n, size=V)
                if V >= 2:
                    head[1], tail[1] = head[0], tail[0]                              # a repeated pair
                if V >= 5:
                    tail[4] = head[4]                                                # head = tail: the diagonal of the mask
                d_head, d_tail = head_tail(rng, V, bound)
                cases.append(((n, V), dict(g_preds=g, head=head.astype(np.int64), tail=tail.astype(np.int64), d_head=d_head, d_tail=d_tail)))
    return cases


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    torch.manual_seed(SEED)
    torch.set_num_threads(1)
    out = {}
    runs = dict(point_d=point_d, pair_d=pair_d, point_g=point_g, pair_g=pair_g)
    for ki, kind in enumerate(runs):
        for fi, (family, bound) in enumerate(FAMILIES.items()):
            rng = np.random.default_rng(SEED + 100 * ki + fi)
            cases = kind_cases(kind, bound, rng)
            pre = f"{kind}/{family}/"
            out[pre + "shape"] = np.array([s for s, _ in cases], np.int64)
            for field in cases[0][1]:
                out[pre + field] = np.concatenate([c[field] for _, c in cases])
            for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
                losses, grads = [], []
                for f_div in DIVS:
                    res = [runs[kind](f_div, dt, **c) for _, c in cases]
                    losses.append([float(l.detach()) for l, _ in res])
                    grads.append(np.concatenate([g.detach().reshape(-1).numpy() for _, gs in res for g in gs]))
                npdt = np.float32 if tag == "32" else np.float64
                with np.errstate(over="ignore"):
                    out[pre + "loss" + tag] = np.array(losses, npdt)
                out[pre + "grad" + tag] = np.stack(grads).astype(npdt)
    for name, labels in LABEL_LISTS.items():
        y = torch.tensor(labels, dtype=torch.float32)
        P = int((y > 0).sum())
        buf = {name: (P, len(labels), len(labels) - P, 0, int(torch.unique(y).numel()))}
        w, total, items = get_weighted_clipped_pos_diffs(qid=name, sorted_std_labels=y, global_buffer=buf)
        assert items == len(labels) and tuple(w.shape) == (P, len(labels))
        out[f"weights/{name}/labels"] = y.numpy()
        out[f"weights/{name}/num_pos"] = np.int64(P)
        out[f"weights/{name}/w"] = w.numpy().astype(np.float32).reshape(P, len(labels))
    path = os.path.join(HERE, "irfgan.npz")
    write_npz(path, out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
