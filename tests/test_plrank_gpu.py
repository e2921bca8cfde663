"""GPU: the PL-Rank kernel (ptr_plrank_fwd_bwd, csrc/plrank.hip) against the float64 restatement of the rule (tests/plrank_ref.py) on the
kernel's own rankings, element by element.

The gate: value_q, the loss and every gradient element within C_PLRANK x the reference's rounding bound (2^-24 x the sum of the absolute values
of the terms the output is built from); a zero bound (all-zero labels, padding, n = 0) wants an exact 0.  C_PLRANK is twice the largest
need of the SAME rule in fp32 eager torch on the CPU on these cases and rankings, rounded up to a half:
    fp32 restatement, worst need over CELLS:  FP32_NEED = 33.778   (L = 1024, S = 3, peaked scores)
    kernel, worst need over CELLS:            KERNEL_NEED = 34.485 (L = 65, S = 3, peaked scores)
Both sides need 31 .. 35 on every peaked cell and at most 7.5 elsewhere: a score 40 units below the maximum rounds the exponent's argument by
up to 2^-24 x 20, a relative error of e that the bound (the terms' absolute values alone) does not carry.
"""
import functools

import pytest
import torch

import plrank_ref as R

pytestmark = pytest.mark.gpu

C_PLRANK = 68.0         # 2 * FP32_NEED, rounded up to a half
LENGTHS, SAMPLES, KINDS = (1, 2, 63, 64, 65, 130, 257, 1024), (1, 3, 9), ("normal", "equal", "peaked")
CELLS = [(L, S) for L in LENGTHS for S in SAMPLES]


@functools.lru_cache(maxsize=None)
def make(L, S):
    """A cell's batch on the CPU: (preds, labels, lens, kw).  top_k, normalize and the score kind alternate over the cells; garbage beyond lens."""
    idx = CELLS.index((L, S))
    g = torch.Generator().manual_seed(500 + idx)
    lens = torch.tensor([L, 0, 1, max(1, L // 2), L, min(L, 7)], dtype=torch.int32)
    labels = torch.randint(0, 5, (6, L), generator=g).float()
    kind = KINDS[(idx // 3 + idx) % 3]                                       # every kind meets every S and, over the lengths, every form
    preds = torch.randn(6, L, generator=g)
    if kind == "equal":
        preds[:] = 0.75
    elif kind == "peaked":                                                   # 40 units of spread, the largest scores on the relevant documents
        preds = 10.0 * labels + 0.25 * preds
    for q, n in enumerate(lens.tolist()):
        preds[q, n:], labels[q, n:] = float("nan"), 1e30
    return preds, labels, lens, dict(top_k=(1, 5, L, L + 3, 0)[idx % 5], normalize=idx % 2 == 0, seed=77 + idx, q0=1000 * idx)


@functools.lru_cache(maxsize=None)
def run(L, S):
    import ptranking_amd.functional as F
    preds, labels, lens, kw = make(L, S)
    loss, parts = F.plrank_objective(preds.cuda(), labels.cuda(), samples=S, lens=lens.cuda(), return_parts=True, **kw)
    return loss.cpu(), {k: v.cpu() for k, v in parts.items()}


def need(L, S, dtype=None):
    """The largest |got - ref| / bound over value_q, grad and the loss: of the kernel, or of the restatement at `dtype` on the kernel's rankings."""
    preds, labels, lens, kw = make(L, S)
    loss, parts = run(L, S)
    ref_v, ref_g, bv, bg = R.plrank(preds, labels, parts["perm"], lens, kw["top_k"], kw["normalize"])
    if dtype is None:
        got_v, got_g, got_loss = parts["value_q"].double(), parts["grad"].double(), loss.double()
    else:
        got_v, got_g = (x.double() for x in R.plrank(preds, labels, parts["perm"], lens, kw["top_k"], kw["normalize"], dtype=dtype)[:2])
        got_loss = -got_v.to(dtype).sum().double()
    worst = float((got_loss + ref_v.sum()).abs() / (bv.sum() + R.EPS32 * ref_v.abs().sum()))
    for got, ref, bound in ((got_v, ref_v, bv), (got_g, ref_g, bg)):
        assert torch.isfinite(got).all()
        err = (got - ref).abs()
        assert torch.all(err[bound == 0] == 0), "non-zero where the reference is exactly 0"
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    return worst


@pytest.mark.parametrize("L, S", CELLS)
def test_float64_gate(L, S):
    n = need(L, S)
    print(f"L={L} S={S} {make(L, S)[3]}: kernel need {n:.3f}, fp32 restatement need {need(L, S, torch.float32):.3f} (C = {C_PLRANK})")
    assert n <= C_PLRANK, f"need {n:.3f} > C = {C_PLRANK}"


@pytest.mark.parametrize("given", [False, True], ids=["hash", "unif"])
@pytest.mark.parametrize("L", LENGTHS)
def test_the_rankings_are_the_samplers(L, given):
    import ptranking_amd.functional as F
    preds, labels, lens, kw = make(L, 3)
    unif = torch.rand(6, 3, L, generator=torch.Generator().manual_seed(L)).cuda() if given else None
    _, parts = F.plrank_objective(preds.cuda(), labels.cuda(), samples=3, lens=lens.cuda(), unif=unif, return_parts=True, **kw)
    want = F.sample_rankings_pl(preds.cuda(), samples=3, seed=kw["seed"], q0=kw["q0"], lens=lens.cuda(), unif=unif)
    assert torch.equal(parts["perm"], want)


@pytest.mark.parametrize("L", [64, 257])
def test_exact_zeros_nan_confinement_and_stable_bits(L):
    import ptranking_amd.functional as F
    preds, labels, lens, kw = (x.clone() if isinstance(x, torch.Tensor) else x for x in make(L, 9))
    preds[0], labels[4, :L] = torch.randn(L, generator=torch.Generator().manual_seed(3)), 0.0
    call = lambda p, y, n, **over: F.plrank_objective(p.cuda(), y.cuda(), samples=9, lens=n.cuda(), return_parts=True, **{**kw, **over})[1]
    a, b = call(preds, labels, lens), call(preds, labels, lens)
    assert all(torch.equal(a[k], b[k]) for k in a), "two calls differ"
    assert torch.all(a["grad"][4] == 0) and a["value_q"][4] == 0 and a["value_q"][1] == 0
    assert torch.all(a["grad"][torch.arange(L).cuda()[None, :] >= lens.cuda()[:, None]] == 0)
    poisoned = preds.clone()
    poisoned[3, 0] = float("nan")
    c = call(poisoned, labels, lens)
    n3, rest = int(lens[3]), [0, 1, 2, 4, 5]
    assert torch.isnan(c["value_q"][3]) and torch.isnan(c["grad"][3, :n3]).all() and torch.all(c["grad"][3, n3:] == 0)
    assert torch.equal(c["perm"][3], torch.arange(L).cuda().expand(9, L))
    assert all(torch.equal(c[k][rest], a[k][rest]) for k in a)
    moved = call(preds[[5, 0]], labels[[5, 0]], lens[[5, 0]], q0=kw["q0"] - 1)      # query 0 as row 1 of another batch: q0 + q is unchanged
    assert all(torch.equal(moved[k][1], a[k][0]) for k in a)


def test_the_hash_path_is_unbiased():
    """5 documents, top 3, 4096 draws: every gradient element within 6 standard errors (sigma_i / sqrt(S), sigma_i from the enumeration of the
    60 top-3 rankings) of the exact gradient of the expected DCG@3."""
    import ptranking_amd.functional as F
    s, labels, S = torch.tensor([[0.3, -0.8, 1.1, 0.0, -0.2]]), torch.tensor([[2.0, 0.0, 1.0, 3.0, 0.0]]), 4096
    exact, sigma = R.exact_gradient(s[0], torch.pow(2.0, labels[0]) - 1.0, 3)
    _, parts = F.plrank_objective(s.cuda(), labels.cuda(), samples=S, top_k=3, normalize=False, seed=11, return_parts=True)
    assert torch.all((-parts["grad"][0].cpu().double() - exact).abs() <= 6.0 * sigma / S ** 0.5)


def test_autograd_and_the_ranker_step():
    import ptranking_amd as pa
    preds, labels, lens, kw = make(65, 3)
    x = preds.cuda().requires_grad_(True)
    loss, parts = pa.functional.plrank_objective(x, labels.cuda(), samples=3, lens=lens.cuda(), return_parts=True, **kw)
    (2.5 * loss).backward()
    assert torch.equal(x.grad, 2.5 * parts["grad"])
    point = dict(num_features=24, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False, dropout=0.0)
    g = torch.Generator().manual_seed(5)
    X, Y = torch.randn(6, 40, 24, generator=g).cuda(), torch.randint(0, 5, (6, 40), generator=g).float().cuda()

    def ranker():
        torch.manual_seed(11)
        r = pa.PLRank(sf_para_dict={"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3, "pointsf": dict(point)}, model_para_dict=dict(samples=8, top_k=5), gpu=True, device="cuda:0")
        r.init(); r.train_mode()
        return r

    a, b = ranker(), ranker()
    before = a.point_sf.flat.detach().clone()
    for step in (1, 2):                                                      # b: the functional's gradient pushed through the scorer by hand
        la, _ = a.train_op(X, Y, epoch_k=1, presort=True, label_type=pa.LABEL_TYPE.MultiLabel)
        lb = pa.functional.plrank_objective(b.forward(X), Y, samples=8, top_k=5, normalize=True, seed=137 * 0x9E3779B1 + step, q0=0)
        b.optimizer.zero_grad(); lb.backward(); b.optimizer.step()
        assert torch.equal(la.reshape(()), lb.detach().reshape(())) and torch.equal(a.point_sf.flat, b.point_sf.flat)
    assert a._pl_calls == 2 and not torch.equal(a.point_sf.flat, before)
