"""Golden fixtures of the adversarial frame's IRGAN point and pair machines: tests/golden/irgan.npz.

Runs the reference's OWN machines on the CPU — IRGAN_Point / IRGAN_Pair (ptranking/ltr_adversarial/pointwise/irgan_point.py,
pairwise/irgan_pair.py): per_query_generation, train_discriminator, train_generator — on a handful of presorted queries, with recording
wrappers around torch.multinomial and torch.randperm (the indices the machines drew) and taps on the two players' forward passes (their
predictions, and after the machine's backward the gradient with respect to them).  The losses are read off the machines' own reductions:
torch.mean inside irgan_pair.py and the generator's step, the module-level BCEWithLogitsLoss of irgan_point.py.

It imports wildltr/ptranking read-only from $PTRANKING_REF, default /root/reference.  Layout (<family>/<case>/<field>):
  gen_point / gen_pair   <T>_q<i>: num_pos, n, S, pos_inds, neg_inds, g_preds (the generator's forward output, before / T)
  point_d                <T>_q<i>: d_sel [2 V] (the discriminator's output on [positives | negatives]), loss, grad [2 V]
  point_g                <T>_q<i>: num_pos, g_preds [n], d_preds [n] (the discriminator on the whole list), choose_inds [5 P], loss, grad [n]
  pair_d                 <loss_type>_q<i>: d_pos [V], d_neg [V], loss, grad_pos, grad_neg
  pair_g                 <loss_type>_<T>_q<i>: g_preds [n], neg_inds [V], d_pos [V], d_neg [V], loss, grad [n]
plus the scalar temperature in every case.  Usage: python tests/golden/make_golden_irgan.py
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("PTRANKING_REF") or "/root/reference"
if not os.path.isdir(os.path.join(REF, "ptranking")):
    raise SystemExit(f"no wildltr/ptranking checkout at {REF} (set PTRANKING_REF)")
sys.path.insert(0, REF)

import ptranking.ltr_adversarial.pairwise.irgan_pair as ref_pair      # noqa: E402
import ptranking.ltr_adversarial.pointwise.irgan_point as ref_point   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 137
F = 10
QUERIES = ((7, 2), (12, 5), (20, 1), (9, 8), (15, 0), (6, 6))          # (documents, relevant documents): 0 and all among them


def sf_para(apply_tl_af):
    return {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-2,
            "pointsf": dict(num_features=F, num_layers=3, AF="R", TL_AF="S", apply_tl_af=apply_tl_af, BN=False, bn_type=None, bn_affine=False)}


def train_data(rng):
    data = []
    for i, (n, p) in enumerate(QUERIES):
        x = torch.from_numpy(rng.standard_normal((1, n, F)).astype(np.float32))
        y = torch.zeros(1, n)
        y[0, :p] = torch.from_numpy(-np.sort(-rng.integers(1, 5, size=p)).astype(np.float32))
        data.append((f"q{i}", x, y))
    return data


class Tap:
    """Records the outputs of player.forward (retaining their gradients)."""

    def __init__(self, player):
        self.log, self.player, self.orig = [], player, player.forward
        player.forward = self

    def __call__(self, x):
        out = self.orig(x)
        if out.requires_grad:
            out.retain_grad()
        self.log.append(out)
        return out


class Spy:
    """Records the results of a torch function while installed."""

    def __init__(self, name):
        self.name, self.log, self.orig = name, [], getattr(torch, name)

    def __enter__(self):
        def f(*a, **k):
            r = self.orig(*a, **k)
            self.log.append(r)
            return r
        setattr(torch, self.name, f)
        return self

    def __exit__(self, *exc):
        setattr(torch, self.name, self.orig)


def np32(t):
    return t.detach().reshape(-1).numpy().astype(np.float32).copy()


def run_point(out, T, rng):
    ad = dict(model_id="IRGAN_Point", ad_training_order="DG", d_epoches=1, g_epoches=1, temperature=T, samples_per_query=5)
    m = ref_point.IRGAN_Point(eval_dict=None, data_dict=dict(train_presort=True), sf_para_dict=sf_para(True), ad_para_dict=ad, gpu=False, device="cpu")
    torch.manual_seed(SEED)
    m.reset_generator()
    m.reset_discriminator()
    data = train_data(rng)
    buf = {}
    m.fill_global_buffer(data, dict_buffer=buf)
    g, d = m.get_generator(), m.get_discriminator()
    gtap, dtap = Tap(g), Tap(d)
    tag = f"T{T:g}"
    for qid, x, y in data:
        n, P = x.size(1), int(buf[qid])
        # ---- per_query_generation (irgan_point.py:130-146)
        g.eval_mode()
        gtap.log.clear()
        with Spy("multinomial") as mn, Spy("randperm") as rp, torch.no_grad():
            s = m.per_query_generation(qid=qid, batch_ranking=x, generator=g, global_buffer=buf)
        case = dict(num_pos=np.int64(P), n=np.int64(n), S=np.int64(5), temperature=np.float32(T))
        if s is None:
            assert P == 0
            case.update(pos_inds=np.zeros(0, np.int64), neg_inds=np.zeros(0, np.int64), g_preds=np.zeros(0, np.float32))
        else:
            assert len(mn.log) == 1 and len(rp.log) == 1
            case.update(pos_inds=s[0].numpy().astype(np.int64), neg_inds=s[1].numpy().astype(np.int64), g_preds=np32(gtap.log[0]))
        out[f"gen_point/{tag}_{qid}"] = case
        if s is None:
            continue
        # ---- train_discriminator (:149-173) on this query alone
        dtap.log.clear()
        losses = []
        orig = ref_point.dis_loss_function
        ref_point.dis_loss_function = lambda p, t: (losses.append(orig(p, t)), losses[-1])[1]
        try:
            m.train_discriminator(train_data=[(qid, x, y)], generated_data={qid: s}, discriminator=d)
        finally:
            ref_point.dis_loss_function = orig
        assert len(dtap.log) == 1 and len(losses) == 1
        out[f"point_d/{tag}_{qid}"] = dict(d_sel=np32(dtap.log[0]), loss=np32(losses[0]), grad=np32(dtap.log[0].grad), temperature=np.float32(T))
        # ---- train_generator (:176-220) on this query alone; the discriminator's outputs on the whole list first (eval mode, no step)
        d.eval_mode()
        with torch.no_grad():
            d_all = np32(dtap.orig(x))
        gtap.log.clear()
        with Spy("multinomial") as mn, Spy("mean") as mean:
            stop = m.train_generator(train_data=[(qid, x, y)], generator=g, discriminator=d, global_buffer=buf)
        assert stop is False and len(gtap.log) == 1 and len(mn.log) == 1 and len(mean.log) == 1
        out[f"point_g/{tag}_{qid}"] = dict(num_pos=np.int64(P), g_preds=np32(gtap.log[0]), d_preds=d_all, choose_inds=mn.log[0].numpy().astype(np.int64),
                                            loss=-np32(mean.log[0]), grad=np32(gtap.log[0].grad), temperature=np.float32(T))


def run_pair(out, loss_type, T, rng):
    ad = dict(model_id="IRGAN_Pair", loss_type=loss_type, ad_training_order="DG", d_epoches=1, g_epoches=1, temperature=T, samples_per_query=5)
    m = ref_pair.IRGAN_Pair(eval_dict=None, data_dict=dict(train_presort=True), sf_para_dict=sf_para(False), ad_para_dict=ad, gpu=False, device="cpu")
    torch.manual_seed(SEED + 1)
    m.reset_generator()
    m.reset_discriminator()
    data = train_data(rng)
    buf = {}
    m.fill_global_buffer(data, dict_buffer=buf)
    g, d = m.get_generator(), m.get_discriminator()
    gtap, dtap = Tap(g), Tap(d)
    tag = f"{loss_type}_T{T:g}"
    for qid, x, y in data:
        n, P = x.size(1), int(buf[qid][0])
        g.eval_mode()
        gtap.log.clear()
        with Spy("multinomial") as mn, Spy("randperm") as rp, torch.no_grad():
            s = m.per_query_generation(qid=qid, batch_ranking=x, generator=g, global_buffer=buf)
        case = dict(num_pos=np.int64(P), n=np.int64(n), S=np.int64(5), temperature=np.float32(T))
        if s is None:
            assert min(P, n - P) == 0
            case.update(pos_inds=np.zeros(0, np.int64), neg_inds=np.zeros(0, np.int64), g_preds=np.zeros(0, np.float32))
        else:
            case.update(pos_inds=s[0].numpy().astype(np.int64), neg_inds=s[1].numpy().astype(np.int64), g_preds=np32(gtap.log[0]))
        out[f"gen_pair/{tag}_{qid}"] = case
        if s is None:
            continue
        # ---- train_discriminator (irgan_pair.py:164-190)
        dtap.log.clear()
        with Spy("mean") as mean:
            m.train_discriminator(train_data=[(qid, x, y)], generated_data={qid: s}, discriminator=d)
        assert len(dtap.log) == 2 and len(mean.log) == 1
        sign = 1.0 if loss_type == "svm" else -1.0
        out[f"pair_d/{tag}_{qid}"] = dict(d_pos=np32(dtap.log[0]), d_neg=np32(dtap.log[1]), loss=sign * np32(mean.log[0]),
                                          grad_pos=np32(dtap.log[0].grad), grad_neg=np32(dtap.log[1].grad), temperature=np.float32(T))
        # ---- train_generator (:193-222)
        gtap.log.clear()
        dtap.log.clear()
        with Spy("multinomial") as mn, Spy("mean") as mean:
            m.train_generator(train_data=[(qid, x, y)], generator=g, discriminator=d, global_buffer=buf)
        assert len(gtap.log) == 1 and len(dtap.log) == 2 and len(mn.log) == 1 and len(mean.log) == 1
        out[f"pair_g/{tag}_{qid}"] = dict(g_preds=np32(gtap.log[0]), neg_inds=mn.log[0].numpy().astype(np.int64), d_pos=np32(dtap.log[0]),
                                          d_neg=np32(dtap.log[1]), loss=-np32(mean.log[0]), grad=np32(gtap.log[0].grad), temperature=np.float32(T))


def main():
    out = {}
    for T in (0.5, 1.0):
        run_point(out, T, np.random.default_rng(SEED))
        for loss_type in ("svm", "log"):
            run_pair(out, loss_type, T, np.random.default_rng(SEED + 7))
    flat = {f"{k}/{f}": np.asarray(v) for k, c in out.items() for f, v in c.items()}
    path = os.path.join(HERE, "irgan.npz")
    np.savez_compressed(path, **flat)
    fams = sorted({k.split("/")[0] for k in out})
    print(f"wrote {path}: {len(out)} cases, {os.path.getsize(path)} bytes; " + ", ".join(f"{f} {sum(k.startswith(f + '/') for k in out)}" for f in fams))


if __name__ == "__main__":
    main()
