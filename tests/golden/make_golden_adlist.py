"""Golden fixtures of the adversarial frame's list machines: tests/golden/adlist.npz.

Runs the reference's OWN pieces — gumbel_softmax (ptranking/ltr_adversarial/util/list_sampling.py:16-36, its torch.rand replaced by
captured uniforms), log_ranking_prob_Plackett_Luce / _Bradley_Terry (util/list_probability.py), IRGAN_List.get_reward and
IRFGAN_List.get_reward (listwise/irgan_list.py:294-312, irfgan_list.py:275-297) and get_f_divergence_functions — through the discriminator's
and the generator's loss lines exactly as the two machines write them (irgan_list.py:336-337, :379-391; irfgan_list.py:322, :375), with
autograd, in float32 and in float64.

It imports wildltr/ptranking read-only from $PTRANKING_REF, default /root/reference.  Cases: n in NS x top_k in (None, 1, 2, 5, n + 3), S
alternating between 1 and 5.  Layout, the cases concatenated in the order of `shape`:
  shape [cases, 4] = (n, S, top_k or 0 for None, Kq = min(top_k, n));  temperature [1]
  x [sum n] the generator's scores, d [sum n] the discriminator's, unif [sum S n] the captured uniforms (case-major, then sample-major)
  gen_idx [sum S Kq] the reference's torch.sort(gumbel_softmax, descending)[:, :top_k], std_idx [sum S Kq] permutations standing in for the
  shuffled label order (the loss lines do not care where a standard ranking comes from)
  D/<PL|BT>/loss32, loss64 [9, cases], grad32, grad64 [9, sum n]: rows IRGAN, then the eight divergences in the order of DIVS; the gradient
  is with respect to d.   G/<PL|BT>/...: [12, cases] and [12, sum n]: rows the four rewards in the order of REWARDS (repTrick, dropLog),
  then the divergences; the gradient is with respect to x.
Draws are screened: a case is redrawn until the sorted probabilities of every sample are pairwise distinct in float32 and order alike in
both precisions.  The archive is written with fixed time stamps, so a second run reproduces the file byte for byte.
Usage: python tests/golden/make_golden_adlist.py
"""
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

REF = os.environ.get("PTRANKING_REF") or "/root/reference"
if not os.path.isdir(os.path.join(REF, "ptranking")):
    raise SystemExit(f"no wildltr/ptranking checkout at {REF} (set PTRANKING_REF)")
sys.path.insert(0, REF)

from ptranking.ltr_adversarial.listwise.irfgan_list import IRFGAN_List   # noqa: E402
from ptranking.ltr_adversarial.listwise.irgan_list import IRGAN_List   # noqa: E402
from ptranking.ltr_adversarial.util import list_sampling   # noqa: E402
from ptranking.ltr_adversarial.util.f_divergence import get_f_divergence_functions   # noqa: E402
from ptranking.ltr_adversarial.util.list_probability import log_ranking_prob_Bradley_Terry, log_ranking_prob_Plackett_Luce   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 137
DIVS = ("TVar", "KL", "RKL", "PC", "NC", "SH", "JS", "GAN")
REWARDS = ((True, True), (True, False), (False, True), (False, False))      # (repTrick, dropLog): -exp(lp), -lp, exp(1 - lp), log(1 - lp)
NS = (1, 2, 3, 17, 64, 65, 130)
TEMPERATURE = 0.5


def top_ks(n):
    return (None, 1, 2, 5, n + 3)


def gumbel_probs(x, unif, dt):
    """The reference's gumbel_softmax on the captured uniforms -> (sorted probabilities, their indices), [S, n] each."""
    real = list_sampling.torch.rand
    list_sampling.torch.rand = lambda *size: torch.from_numpy(unif).to(dt)
    try:
        y = list_sampling.gumbel_softmax(x, samples_per_query=unif.shape[0], temperature=TEMPERATURE)
    finally:
        list_sampling.torch.rand = real
    return torch.sort(y, dim=1, descending=True)                                # irgan_list.py:237


def lp_of(pl):
    return log_ranking_prob_Plackett_Luce if pl else log_ranking_prob_Bradley_Terry


def d_loss(family, pl, dt, d, std_idx, gen_idx):
    d_preds = torch.tensor(d, dtype=dt, requires_grad=True)
    lp_std = lp_of(pl)(d_preds[torch.from_numpy(std_idx)])                      # the discriminator on the gathered rankings, [S, K]
    lp_gen = lp_of(pl)(d_preds[torch.from_numpy(gen_idx)])
    if family == "IRGAN":
        dis_loss = - (torch.sum(lp_std) + torch.sum(torch.log(1.0 - lp_gen)))  # irgan_list.py:336-337
    else:
        activation_f, conjugate_f = get_f_divergence_functions(family)
        dis_loss = torch.mean(conjugate_f(activation_f(lp_gen))) - torch.mean(activation_f(lp_std))   # irfgan_list.py:322
    dis_loss.backward()
    return dis_loss, d_preds.grad


def g_loss(family, pl, dt, x, d, unif, top_k):
    g_preds = torch.tensor(x[None], dtype=dt, requires_grad=True)
    probs, inds = gumbel_probs(g_preds, unif, dt)
    if top_k is not None:                                                       # irgan_list.py:282-291
        probs, inds = probs[:, 0:top_k], inds[:, 0:top_k]
    reward_d = torch.tensor(d, dtype=dt)[inds]                                  # :356-375
    g_log_prob = log_ranking_prob_Plackett_Luce(probs)                          # :379
    if isinstance(family, tuple):
        rewards = IRGAN_List.get_reward(None, reward_d, PL_discriminator=pl, replace_trick_4_generator=family[0],
                                        drop_discriminator_log_4_reward=family[1])
        loss = torch.mean(g_log_prob * rewards.detach())                        # :391
    else:
        activation_f, conjugate_f = get_f_divergence_functions(family)
        me = types.SimpleNamespace(activation_f=activation_f, conjugate_f=conjugate_f)
        rewards = IRFGAN_List.get_reward(me, reward_d, PL_discriminator=pl, replace_trick_4_generator=True, drop_discriminator_log_4_reward=True)
        loss = -torch.mean(g_log_prob * rewards.detach())                       # irfgan_list.py:375
    loss.backward()
    return loss, g_preds.grad.view(-1)


def draw_case(rng, n, S):
    """(x, d, unif, order [S, n]) with the sorted probabilities pairwise distinct in float32 and one order in both precisions."""
    while True:
        x = np.clip(rng.standard_normal(n), -2.0, 2.0).astype(np.float32)
        d = rng.uniform(0.02, 0.98, size=n).astype(np.float32)                 # the discriminator ends in a sigmoid
        unif = (rng.integers(0, 2 ** 24, size=(S, n)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
        p32, i32 = gumbel_probs(torch.tensor(x[None]), unif, torch.float32)
        p64, i64 = gumbel_probs(torch.tensor(x[None], dtype=torch.float64), unif, torch.float64)
        if bool((p32[:, :-1] > p32[:, 1:]).all()) and bool((i32 == i64).all()):
            return x, d, unif, i64.numpy()


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
    rng = np.random.default_rng(SEED)
    cases = []
    for a, n in enumerate(NS):
        for b, top_k in enumerate(top_ks(n)):
            S = 1 if (a + b) % 2 == 0 else 5
            x, d, unif, order = draw_case(rng, n, S)
            K = n if top_k is None else min(top_k, n)
            std = np.stack([rng.permutation(n)[:K] for _ in range(S)]).astype(np.int64)
            cases.append(dict(n=n, S=S, top_k=top_k, K=K, x=x, d=d, unif=unif, gen=np.ascontiguousarray(order[:, :K]), std=std))
    out = {"shape": np.array([(c["n"], c["S"], c["top_k"] or 0, c["K"]) for c in cases], np.int64), "temperature": np.array([TEMPERATURE], np.float32)}
    for field, key in (("x", "x"), ("d", "d"), ("unif", "unif"), ("gen_idx", "gen"), ("std_idx", "std")):
        out[field] = np.concatenate([c[key].reshape(-1) for c in cases])
    for pl, pname in ((True, "PL"), (False, "BT")):
        for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
            npdt = np.float32 if tag == "32" else np.float64
            for mode, families in (("D", ("IRGAN",) + DIVS), ("G", REWARDS + DIVS)):
                losses, grads = [], []
                for family in families:
                    if mode == "D":
                        res = [d_loss(family, pl, dt, c["d"], c["std"], c["gen"]) for c in cases]
                    else:
                        res = [g_loss(family, pl, dt, c["x"], c["d"], c["unif"], c["top_k"]) for c in cases]
                    losses.append([float(l.detach()) for l, _ in res])
                    grads.append(np.concatenate([g.detach().reshape(-1).numpy() for _, g in res]))
                with np.errstate(over="ignore"):
                    out[f"{mode}/{pname}/loss{tag}"] = np.array(losses, npdt)
                    out[f"{mode}/{pname}/grad{tag}"] = np.stack(grads).astype(npdt)
    path = os.path.join(HERE, "adlist.npz")
    write_npz(path, out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
