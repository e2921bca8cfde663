"""GPU: what sits between a public loss of ptranking_amd.functional and the C ABI — the sequence of entry points and their scalar arguments
(a literal table, recorded before the launch path was unified), the handling of non-contiguous inputs, and the extra outputs.

Shapes: B = 3, L = 6, T = 2 — B is no multiple of the four queries per workgroup and L % 4 != 0.  Every hyper-parameter is exactly
representable in fp32, so the table holds the values as written.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

B, L, T = 3, 6, 2
P = "ptr"            # a non-NULL pointer argument (a NULL one is recorded as None)


def inputs():
    g = torch.Generator().manual_seed(7)
    d = dict(preds=torch.randn(B, L, generator=g),
             labels=torch.tensor([[3., 2., 1., 1., 0., 0.], [4., 2., 2., 1., 0., 0.], [2., 1., 1., 0., 0., 0.]]),
             perm=torch.stack([torch.randperm(L, generator=g) for _ in range(B)]),
             unif=torch.rand(B, L, generator=g) * 0.98 + 0.01,
             rele=(torch.rand(B, T, L, generator=g) < 0.5).float(),
             vars=torch.rand(B, L, generator=g) + 0.5)
    return {k: v.cuda() for k, v in d.items()}


def losses(F, d):
    """name -> loss as a function of the first differentiable input."""
    y, perm, rele = d["labels"], d["perm"], d["rele"]
    div = lambda obj, **kw: (lambda p: F.divprob_loss(p, d["vars"], rele, obj, **kw))
    return {
        "ranknet": lambda p: F.ranknet_loss(p, y, sigma=2.0),
        "lambdarank": lambda p: F.lambdarank_loss(p, y, sigma=0.5),
        "lambdaloss": lambda p: F.lambdaloss_loss(p, y, k=3, sigma=1.5, mu=4.0, loss_type="NDCG_Loss2++", presort=False),
        "softrank": lambda p: F.softrank_loss(p, y, delta=2.0, top_k=4),
        "listnet": lambda p: F.listnet_loss(p, y),
        "rankmse": lambda p: F.rankmse_loss(p, y),
        "wassrank": lambda p: F.wassrank_loss(p, y, cost_type="dg", lam=0.5, sh_itr=5, gain_base=4.0, non_rele_gap=100.0, var_penalty=2.0,
                                              scale_by_max_label=True),
        "rankcosine": lambda p: F.rankcosine_loss(p, y),
        "stlistnet": lambda p: F.stlistnet_loss(p, y, temperature=0.5, unif=d["unif"]),
        "listmle": lambda p: F.listmle_loss(p, perm),
        "mdprank": lambda p: F.mdprank_loss(p, y, perm, top_k=4, gamma=0.5),
        "approxndcg": lambda p: F.approxndcg_loss(p, y, alpha=8.0, presort=True, couple_batch=False, grad_scale_override=0.25),
        "alphadcg": lambda p: F.alphadcg_loss(p, rele, rt=8.0, alpha=0.25, top_k=4, top_k_axis="documents"),
        "divprob_andcg": div("aNDCG", beta=0.25, top_k=1, top_k_axis="reference"),
        "divprob_nerria": div("nERR-IA", beta=0.5, top_k=4, max_label=2.0),
        "divprob_paircls": div("PairCLS"),
        "divprob_lambdapaircls": div("LambdaPairCLS", norm=False),
    }


SUM = ("ptr_sum_f32", (P, B, 1.0, P, P))
EXPECTED = {
    "ranknet": [("ptr_ranknet_fwd_bwd", (P, P, None, B, L, 2.0, None, P, P, P)), SUM],
    "lambdarank": [("ptr_lambdarank_fwd_bwd", (P, P, None, B, L, 0.5, None, P, P, P)), SUM],
    "lambdaloss": [("ptr_lambdaloss_fwd_bwd", (P, P, None, B, L, 3, 1.5, 4.0, 2, 0, None, P, P, P)), SUM],
    "softrank": [("ptr_softrank_fwd_bwd", (P, P, None, B, L, 2.0, 4, None, P, P, P)), SUM],
    "listnet": [("ptr_listnet_fwd_bwd", (P, P, None, B, L, None, P, P, P)), SUM],
    "rankmse": [("ptr_rankmse_fwd_bwd", (P, P, None, B, L, P, P, P, P))],
    "wassrank": [("ptr_wassrank_fwd_bwd", (P, P, None, B, L, 3, 4.0, 100.0, 2.0, 0.5, 5, 1, P, P, P, P))],
    "rankcosine": [("ptr_rankcosine_fwd_bwd", (P, P, None, B, L, None, P, P, P)), SUM],
    "stlistnet": [("ptr_stlistnet_fwd_bwd", (P, P, P, None, B, L, 0.5, None, P, P, P)), SUM],
    "listmle": [("ptr_listmle_fwd_bwd", (P, P, None, B, L, None, P, P, P)), SUM],
    "mdprank": [("ptr_mdprank_fwd_bwd", (P, P, P, None, B, L, 4, 0.5, None, P, P, P)), SUM],
    "approxndcg": [("ptr_approxndcg_fwd_bwd", (P, P, None, B, L, 8.0, 1, 0, 0.25, P, P, P, P, P, P))],
    "alphadcg": [("ptr_alphadcg_fwd_bwd", (P, P, None, None, B, T, L, 8.0, 0.25, 4, 1, None, P, P, P)), SUM],
    "divprob_andcg": [("ptr_divprob_fwd_bwd", (P, P, P, None, None, B, T, L, 0, 0.25, 1, 0, 1.0, 1, None, P, P, P, P)), SUM],
    "divprob_nerria": [("ptr_divprob_fwd_bwd", (P, P, P, None, None, B, T, L, 1, 0.5, 4, 0, 2.0, 1, None, P, P, P, P)), SUM],
    "divprob_paircls": [("ptr_divprob_fwd_bwd", (P, P, P, None, None, B, T, L, 2, 0.5, 0, 0, 1.0, 1, None, P, P, P, P)), SUM],
    "divprob_lambdapaircls": [("ptr_divprob_fwd_bwd", (P, P, P, None, None, B, T, L, 3, 0.5, 0, 0, 1.0, 0, None, P, P, P, P)), SUM],
}
NAMES = sorted(EXPECTED)


def plain(a):
    if a is None:
        return None
    if isinstance(a, C.c_void_p):
        return P
    return a.value if hasattr(a, "value") else a


def record(monkeypatch, fn):
    """Run fn() with _lib.call wrapped -> [(entry name, arguments with pointers reduced to P / None)]."""
    from ptranking_amd import _lib
    calls, real = [], _lib.call

    def spy(name, *args):
        calls.append((name, tuple(plain(a) for a in args)))
        return real(name, *args)

    with monkeypatch.context() as m:
        m.setattr(_lib, "call", spy)
        out = fn()
    return calls, out


@pytest.fixture(scope="module")
def data():
    return inputs()


def test_the_table_names_every_public_loss():
    import ptranking_amd.functional as F
    public = {n[:-len("_loss")] for n in F.__all__ if n.endswith("_loss")}
    assert public == {n.split("_")[0] for n in NAMES}


@pytest.mark.parametrize("grad", [True, False], ids=["grad", "nograd"])
@pytest.mark.parametrize("name", NAMES)
def test_calls_and_scalar_arguments(name, grad, data, monkeypatch):
    import ptranking_amd.functional as F
    x = data["preds"].clone().requires_grad_(grad)
    calls, loss = record(monkeypatch, lambda: losses(F, data)[name](x))
    print(name, calls)
    assert calls == EXPECTED[name]
    assert loss.shape == () and loss.requires_grad == grad and torch.isfinite(loss)


def grad_of(fn, x):
    x = x.detach().clone().requires_grad_(True)
    fn(x).backward()
    return x.grad


@pytest.mark.parametrize("name", NAMES)
def test_transposed_preds_get_the_gradient_of_a_contiguous_clone(name, data):
    import ptranking_amd.functional as F
    fn = losses(F, data)[name]
    base = data["preds"].t().contiguous().requires_grad_(True)        # [L, B] leaf
    preds = base.t()
    assert not preds.is_contiguous()
    fn(preds).backward()
    assert torch.equal(base.grad.t(), grad_of(fn, preds.contiguous()))


@pytest.mark.parametrize("objective", ["aNDCG", "nERR-IA", "PairCLS", "LambdaPairCLS"])
@pytest.mark.parametrize("which", ["mus", "vars", "vars_only"])
def test_divprob_transposed_mus_and_vars(objective, which, data):
    import ptranking_amd.functional as F
    mus, vars_, rele = data["preds"], data["vars"], data["rele"]
    m = mus.clone().requires_grad_(True)
    v = vars_.clone().requires_grad_(True)
    F.divprob_loss(m, v, rele, objective).backward()
    if which == "mus":
        base = mus.t().contiguous().requires_grad_(True)
        v2 = vars_.clone().requires_grad_(True)
        F.divprob_loss(base.t(), v2, rele, objective).backward()
        assert torch.equal(base.grad.t(), m.grad) and torch.equal(v2.grad, v.grad)
    else:
        base = vars_.t().contiguous().requires_grad_(True)
        m2 = mus.clone().requires_grad_(which == "vars")
        loss = F.divprob_loss(m2, base.t(), rele, objective)
        assert loss.requires_grad
        loss.backward()
        assert torch.equal(base.grad.t(), v.grad)
        assert torch.equal(m2.grad, m.grad) if which == "vars" else m2.grad is None


@pytest.mark.parametrize("grad", [True, False], ids=["grad", "nograd"])
def test_approxndcg_parts(grad, data):
    import ptranking_amd.functional as F
    loss, parts = F.approxndcg_loss(data["preds"].clone().requires_grad_(grad), data["labels"], return_parts=True)
    assert loss.shape == () and sorted(parts) == ["dcg_q", "inv_idcg_q", "scale"]
    assert parts["dcg_q"].shape == (B,) and parts["inv_idcg_q"].shape == (B,) and parts["scale"].shape == (2,)
    assert all(t.dtype == torch.float32 and torch.isfinite(t).all() for t in parts.values())


@pytest.mark.parametrize("grad", [True, False], ids=["grad", "nograd"])
@pytest.mark.parametrize("name", ["alphadcg", "divprob_andcg", "divprob_nerria", "divprob_paircls", "divprob_lambdapaircls"])
def test_loss_q_sums_to_the_loss(name, grad, data):
    """fp32 summation of three numbers, in any order and at any intermediate precision, rounds at most twice: |error| <= 2 u sum|x|, u = 2^-24."""
    import ptranking_amd.functional as F
    x = data["preds"].clone().requires_grad_(grad)
    if name == "alphadcg":
        loss, loss_q = F.alphadcg_loss(x, data["rele"], return_loss_q=True)
    else:
        objective = {"andcg": "aNDCG", "nerria": "nERR-IA", "paircls": "PairCLS", "lambdapaircls": "LambdaPairCLS"}[name.split("_")[1]]
        loss, loss_q = F.divprob_loss(x, data["vars"], data["rele"], objective, return_loss_q=True)
    assert loss_q.shape == (B,) and loss_q.dtype == torch.float32 and not loss_q.requires_grad
    q = loss_q.double().cpu()
    assert abs(float(q.sum()) - float(loss.detach().double())) <= 2.0 ** -23 * float(q.abs().sum())
