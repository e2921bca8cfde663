"""GPU: the NeuralNDCG kernel (ptr_neuralndcg_fwd_bwd, csrc/neuralndcg.hip) against the float64 restatement of the rule
(tests/neuralndcg_ref.py), element by element.

The gate (the float64 convention of tests/f64_loss_bounds.py): every loss_q and every gradient element within C * 2^-24 * (|ref| + the query's
max |ref|).  C = C_NEURAL is twice the largest need of the SAME rule in fp32 eager torch on the CPU on these inputs, rounded up to a half:
    fp32 restatement, worst need over CASES:  FP32_NEED = 2199.56 (tau = 0.1: |logits| reach 1e4 and fp32 loses 1e-3 in the exponent)
    kernel, worst need over CASES:            KERNEL_NEED = 312.83 (fp32 forward, fp64 exponent and fp64 reverse sweep)
A zero reference (all-zero labels, padding, n = 0) leaves a zero bound: those outputs are exactly 0.
"""
import functools

import pytest
import torch

import neuralndcg_ref as R
from launch_form import launch_form

pytestmark = pytest.mark.gpu

FP32_NEED = 2199.56      # measured on the CPU: case 'it1_tau0.1' (then 'it0_tau0.1' 1338, 'scale30' 504; tau = 1 cases at most 102)
KERNEL_NEED = 312.83     # measured on the MI355X: case 'scale30' (then 'it50_tau0.1' 255, 'L3' 111; every other case below 35)
C_NEURAL = 4399.5        # 2 * FP32_NEED, rounded up to a half
ENTRY = "ptr_neuralndcg_fwd_bwd"
CUT = launch_form(ENTRY, 1, 50)[5]                                          # the longest list of the resident form


def _case(L, B=None, lens=None, scale=1.0, ties=None, zero_labels=False, **kw):
    return dict(L=L, B=B or (3 if L > 65 else 5), lens=lens, scale=scale, ties=ties, zero_labels=zero_labels,
                kw={"tau": 1.0, "iters": 50, "top_k": None, "powered": True, **kw})


CASES = {f"L{L}": _case(L) for L in (1, 2, 3, 63, 64, 65)}
CASES.update({"cut": _case(CUT), "cut+1": _case(CUT + 1), "ragged": _case(65, lens=[0, 1, 65, 33, 2]),
              "ragged_cut+1": _case(CUT + 1, lens=[CUT + 1, 0, 100])})
CASES.update({f"it{T}_tau{tau}": _case(65, iters=T, tau=tau) for T in (0, 1, 50) for tau in (1.0, 0.1)})
CASES.update({f"k{k}_pow{int(p)}": _case(20, top_k=k, powered=p) for k in (None, 1, 5, 23) for p in (True, False)})
CASES.update({"ties": _case(65, ties="some"), "all_equal": _case(33, ties="all"), "zero_labels": _case(17, zero_labels=True),
              "scale30": _case(65, scale=30.0), "hist_ws": _case(150, B=2)})


@functools.lru_cache(maxsize=None)
def make(name):
    """(preds, labels, lens or None, kw) on the CPU, seeded by the case; garbage beyond lens."""
    c, g = CASES[name], torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    preds = torch.randn(c["B"], c["L"], generator=g) * c["scale"]
    labels = torch.randint(0, 5, (c["B"], c["L"]), generator=g).float()
    preds = (preds * 2).round() / 2 if c["ties"] == "some" else preds   # many equal scores
    if c["ties"] == "all":
        preds[0] = 0.75                                                     # one whole list of equal scores
    labels[1] *= 0.0 if c["zero_labels"] else 1.0
    lens = None if c["lens"] is None else torch.tensor(c["lens"], dtype=torch.int32)
    if lens is not None:
        for q, n in enumerate(c["lens"]):
            preds[q, n:] = float("nan")
            labels[q, n:] = 1e30
    return preds, labels, lens, c["kw"]


reference = functools.lru_cache(maxsize=None)(lambda name: R.loss_and_grad(*make(name)[:3], torch.float64, **make(name)[3]))


def need(got_q, got_g, name):
    """The largest |got - ref| / (2^-24 (|ref| + the query's max |ref|)) over loss_q and grad; a zero bound (padding too) wants an exact 0."""
    ref_q, ref_g = reference(name)
    worst = 0.0
    for got, ref, qmax in ((got_q.double(), ref_q, ref_q.abs()), (got_g.double(), ref_g, ref_g.abs().amax(dim=1, keepdim=True))):
        assert torch.isfinite(got).all(), name
        bound = 2.0 ** -24 * (ref.abs() + qmax)
        err = (got - ref).abs()
        assert torch.all(err[bound == 0] == 0), f"{name}: non-zero where the reference is exactly 0"
        if (bound > 0).any():
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    return worst


def run(name):
    import ptranking_amd.functional as F
    preds, labels, lens, kw = make(name)
    x = preds.cuda().requires_grad_(True)
    loss, parts = F.neuralndcg_loss(x, labels.cuda(), temperature=kw["tau"], iters=kw["iters"], top_k=kw["top_k"], powered=kw["powered"],
                                    lens=None if lens is None else lens.cuda(), return_parts=True)
    loss.backward()
    return loss.detach().cpu(), parts["loss_q"].cpu(), x.grad.cpu()


@pytest.mark.parametrize("name", sorted(CASES))
def test_float64_gate(name):
    loss, loss_q, grad = run(name)
    n = need(loss_q, grad, name)
    print(f"{name}: kernel need {n:.3f} (C = {C_NEURAL})")
    assert n <= C_NEURAL, f"{name}: need {n:.3f} > C = {C_NEURAL}"
    assert abs(float(loss) - float(loss_q.double().sum())) <= 2.0 ** -22 * float(loss_q.abs().sum())
    assert name != "zero_labels" or (loss_q[1] == 0 and torch.all(grad[1] == 0))


@pytest.mark.parametrize("name", ["ragged", "ragged_cut+1", "ties"])
def test_two_calls_and_a_query_alone_give_the_same_bits(name):
    import ptranking_amd.functional as F
    _, q1, g1 = run(name)
    _, q2, g2 = run(name)
    assert torch.equal(q1, q2) and torch.equal(g1, g2)
    preds, labels, lens, kw = make(name)
    for q in range(preds.shape[0]):
        x = preds[q:q + 1].cuda().requires_grad_(True)
        loss = F.neuralndcg_loss(x, labels[q:q + 1].cuda(), temperature=kw["tau"], iters=kw["iters"], lens=None if lens is None else lens[q:q + 1].cuda())
        loss.backward()
        assert torch.equal(loss.detach().cpu().reshape(()), q1[q]) and torch.equal(x.grad.cpu()[0], g1[q]), (name, q)


def test_ranker_step_on_the_point_scorer():
    """The loss is the functional's on the scorer's scores, the parameters move; use_direct_step changes no bit (no direct C step of its own)."""
    import ptranking_amd as pa
    SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
          "pointsf": dict(num_features=24, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False, dropout=0.0)}
    g = torch.Generator().manual_seed(5)
    X, Y = torch.randn(6, 40, 24, generator=g).cuda(), torch.randint(0, 5, (6, 40), generator=g).float().cuda()

    def make_ranker(direct):
        torch.manual_seed(11)
        r = pa.NeuralNDCG(sf_para_dict={**SF, "pointsf": dict(SF["pointsf"])}, model_para_dict=dict(temperature=0.5, iters=10, top_k=10), gpu=True, device="cuda:0")
        r.init(); r.train_mode(); r.use_direct_step = direct
        return r

    a, b = make_ranker(True), make_ranker(False)
    before = a.point_sf.flat.detach().clone()
    want = pa.functional.neuralndcg_loss(a.predict(X).detach(), Y, temperature=0.5, iters=10, top_k=10)
    (la, _), (lb, _) = (r.train_op(X, Y, epoch_k=1, presort=True, label_type=pa.LABEL_TYPE.MultiLabel) for r in (a, b))
    assert torch.equal(la.reshape(()), lb.reshape(())) and torch.equal(a.point_sf.flat, b.point_sf.flat)
    assert torch.allclose(la.detach().reshape(()), want.reshape(()), rtol=1e-4) and not torch.equal(a.point_sf.flat, before)
