"""GPU: attention heads wider than 128 on the wide forms of the listsf kernels (csrc/listsf_wide.hip; 128 < dh <= 352).

(a) the element-wise float64 gate of tests/test_listsf_bounds_gpu.py (f64_bounds.mhsa_fwd / mhsa_bwd, C_ATTN unchanged) through the C ABI
    on a case list that reaches every wide form (tests/test_listsf_wide_cpu.py restates the dispatch and checks that it does);
(b) the reference's own MultiheadAttention / ListNeuralRanker at one head of 136 and 176 (tests/golden/make_golden_listsf_wide.py);
(c) the module at the Yahoo! width (700 features, 2 heads: dh 350) against a float64 restatement of list_ranker.py:209-247;
(d) bit-identical repeats, packed == separate, stored dS == recomputing, empty queries, scores of +-60;
(e) rankers that train on it; (f) the narrow forms next to it.
Each gate prints its worst err/E as a MEASURED line (run with -s)."""
import copy
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import f64_bounds as B
import golden_util as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, L, F, heads, mode, dS scratch, packed [B, L, 3F] projection); dh = F / heads; DT = 2 ceil(dh / 32) column tiles
WIDE_CASES = [
    (2, 7, 258, 2, "eval", False, False),               # dh 129: DT 10, the tail of one column, scalar loads
    (3, 33, 264, 2, "lens", False, False),              # dh 132
    (2, 65, 136, 1, "dropout", False, False),           # dh 136 (MSLR-WEB30K, one head)
    (3, 128, 136, 1, "lens", True, False),              # dh 136, stored dS
    (2, 129, 300, 2, "dropout+lens", True, False),      # dh 150, scalar loads
    (2, 32, 300, 2, "dropout+lens", False, True),       # dh 150 packed: row stride 900
    (2, 64, 176, 1, "eval", False, False),              # dh 176: DT 12
    (2, 257, 384, 2, "lens", True, False),              # dh 192
    (2, 33, 220, 1, "lens", False, False),              # dh 220 (Istella, one head): DT 14
    (2, 128, 220, 1, "dropout", True, False),           # dh 220, stored dS
    (2, 64, 256, 1, "eval", False, False),              # dh 256: DT 16
    (2, 130, 512, 2, "dropout+lens", True, True),       # dh 256 packed
    (2, 40, 272, 1, "eval", False, False),              # dh 272: DT 18
    (2, 129, 544, 2, "dropout+lens", True, False),      # dh 272, stored dS
    (2, 31, 300, 1, "dropout", False, False),           # dh 300: DT 20
    (2, 128, 300, 1, "lens", True, False),              # dh 300, stored dS
    (2, 129, 700, 2, "eval", False, False),             # dh 350 (Yahoo!, the reference's 2 heads): DT 22, scalar loads
    (3, 257, 700, 2, "dropout+lens", True, False),      # dh 350, stored dS
    (2, 513, 700, 2, "dropout", False, False),          # dh 350, recomputing dQ
    (1, 64, 352, 1, "eval", False, False),              # dh 352: the limit
    (2, 1031, 352, 1, "dropout+lens", True, False),     # dh 352, a long list
]


def _id(c):
    Bn, L, F, H, mode, ds, packed = c
    return f"{Bn}x{L}x{F}-h{H}-{mode}" + ("-ds" if ds else "") + ("-packed" if packed else "")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def LS():
    from ptranking_amd import listsf
    return listsf


@pytest.fixture(scope="module")
def wide_golden():
    spec = importlib.util.spec_from_file_location("make_golden_listsf_wide", os.path.join(G.GOLDEN_DIR, "make_golden_listsf_wide.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load()


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("case", WIDE_CASES, ids=[_id(c) for c in WIDE_CASES])
def test_wide_attention_within_f64_bounds(LS, case):
    from ptranking_amd import _lib
    Bn, L, F, H, mode, use_ds, packed = case
    Q, K, V, dO, lens = B.attn_inputs(Bn, L, F, H, seed=L + F)
    p = 0.1 if "dropout" in mode else 0.0
    lens = lens if "lens" in mode else None
    seed, site = 1000 + L, 2
    keep = LS.mhsa_dropout_mask(Bn, L, H, p, seed, site, DEV).cpu() if p else None
    st = _lib.current_stream(torch.device(DEV))
    if packed:
        qkv = torch.cat([Q, K, V], -1).to(DEV)
        ld, ptrs = 3 * F, [LS._voff(qkv, i * F) for i in range(3)]
        dqkv = torch.full_like(qkv, float("nan"))
        gptrs = [LS._voff(dqkv, i * F) for i in range(3)]
    else:
        dev = [t.to(DEV) for t in (Q, K, V)]
        ld, ptrs = F, [_lib.ptr(t) for t in dev]
        grads = [torch.full_like(dev[0], float("nan")) for _ in range(3)]
        gptrs = [_lib.ptr(t) for t in grads]
    lens_d = lens.to(DEV) if lens is not None else None
    O = torch.full((Bn, L, F), float("nan"), device=DEV)
    lse = torch.full((Bn * H * L,), float("nan"), device=DEV)
    _lib.call("ptr_mhsa_forward", *ptrs, ld, _lib.ptr(lens_d), Bn, L, F, H, C.c_float(p), C.c_uint64(seed), site, _lib.ptr(O), _lib.ptr(lse), st)
    dO_d = dO.to(DEV)
    dvec = torch.empty(Bn * H * L, device=DEV)
    ds_ws = torch.full((Bn * H * L * L,), float("nan"), device=DEV) if use_ds else None
    _lib.call("ptr_mhsa_backward", *ptrs, ld, _lib.ptr(O), _lib.ptr(dO_d), _lib.ptr(lse), _lib.ptr(lens_d), Bn, L, F, H, C.c_float(p),
              C.c_uint64(seed), site, _lib.ptr(dvec), *gptrs, _lib.ptr(ds_ws), st)
    torch.cuda.synchronize()
    if packed:
        dQ, dK, dV = (dqkv[..., i * F:(i + 1) * F].cpu() for i in range(3))
    else:
        dQ, dK, dV = (t.cpu() for t in grads)
    O, lse = O.cpu(), lse.cpu()
    what = f"wide attention {_id(case)}"
    c = B.C_ATTN
    rO, EO, rL, EL = B.mhsa_fwd(Q, K, V, H, keep, p, lens, c)
    B.gate(O, rO, EO, what + " O", c)
    B.gate(lse.reshape(Bn, H, L), rL, EL, what + " LSE", c)
    ref = B.mhsa_bwd(Q, K, V, O, dO, lse, H, keep, p, lens, c)
    B.gate(dV, ref["dV"], ref["E_dV"], what + " dV", c)
    B.gate(dK, ref["dK"], ref["E_dK"], what + " dK", c)
    B.gate(dQ, ref["dQ"], ref["E_dQ"], what + " dQ", c)
    if lens is not None:
        for b in range(Bn):
            n = int(lens[b])
            assert bool((dK[b, n:] == 0).all()) and bool((dV[b, n:] == 0).all()), f"{what}: dK / dV of padded keys of query {b} not 0"


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("name", ["c0_d136", "c1_d176"])
def test_golden_wide_mhsa(LS, wide_golden, name):
    c = wide_golden["mhsa"][name]
    Fd = c["x"].shape[-1]
    m = LS.MultiheadAttention(hid_dim=Fd, n_heads=int(c["n_heads"]), dropout=0.1).to(DEV)
    m.load_state_dict({k: _t(v) for k, v in G.sub(c, "sd").items()})
    m.eval()
    x = _t(c["x"]).to(DEV).requires_grad_(True)
    y = m(x)
    (y * _t(c["R"]).to(DEV)).sum().backward()
    G.assert_close(y.detach().cpu().numpy(), c["y"], "y"); G.assert_close(x.grad.cpu().numpy(), c["dx"], "dx")
    for k, p in m.named_parameters():
        G.assert_close(p.grad.cpu().numpy(), c[f"grad/{k}"], k)


def test_golden_wide_listsf_scorer(LS, wide_golden):
    c = wide_golden["listsf"]["AttnDIN_d136"]
    mods = LS.build_listsf(num_features=136, ff_dims=[16], AF='R', TL_AF='GE', apply_tl_af=False, BN=False, bn_type='BN2', bn_affine=False,
                           n_heads=1, encoder_layers=1, encoder_type='AttnDIN')
    for part, m in mods.items():
        m.load_state_dict({k: _t(v) for k, v in G.sub(G.sub(c, "sd"), part).items()})
        m.to(DEV).eval()
    preds = LS.listsf_forward(mods, 'AttnDIN', _t(c["x"]).to(DEV))
    (preds * _t(c["R"]).to(DEV)).sum().backward()
    G.assert_close(preds.detach().cpu().numpy(), c["preds"], "preds")
    for part, m in mods.items():
        for k, p in m.named_parameters():
            got = p.grad.cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
            G.assert_close(got, c[f"grad/{part}/{k}"], f"{part}/{k}")


# ------------------------------------------------------------------------------------------------ (c)
def _mha_f64(x, sd, H):
    """ptranking/base/list_ranker.py:209-247 in float64, on one unpadded batch."""
    Bn, L, Fd = x.shape
    dh = Fd // H
    q, k, v = (x @ sd[f"w_{n}.weight"].T + sd[f"w_{n}.bias"] for n in "qkv")
    q, k, v = (t.view(Bn, L, H, dh).permute(0, 2, 1, 3) for t in (q, k, v))
    att = torch.softmax(q @ k.permute(0, 1, 3, 2) / torch.sqrt(torch.tensor(float(dh), dtype=torch.float64)), dim=-1)
    o = (att @ v).permute(0, 2, 1, 3).contiguous().view(Bn, L, Fd)
    return o @ sd["fc.weight"].T + sd["fc.bias"]


@pytest.fixture(scope="module")
def yahoo_module(LS):
    """MultiheadAttention(700, 2) with seeded weights, its input and cotangent, and the float64 restatement's output and gradients."""
    torch.manual_seed(700)
    m = LS.MultiheadAttention(hid_dim=700, n_heads=2, dropout=0.1).to(DEV).eval()
    x, R = torch.randn(2, 9, 700), torch.randn(2, 9, 700)
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
    x64 = x.double().requires_grad_(True)
    y64 = _mha_f64(x64, sd, 2)
    (y64 * R.double()).sum().backward()
    return m, x, R, sd, x64, y64


def test_yahoo_width_module_against_float64(yahoo_module):
    m, x, R, sd, x64, y64 = yahoo_module
    m.zero_grad()
    xd = x.to(DEV).requires_grad_(True)
    y = m(xd)
    (y * R.to(DEV)).sum().backward()
    G.assert_close(y.detach().cpu().numpy(), y64.detach().numpy(), "y")
    G.assert_close(xd.grad.cpu().numpy(), x64.grad.numpy(), "dx")
    for k, p in m.named_parameters():
        G.assert_close(p.grad.cpu().numpy(), sd[k].grad.numpy(), k)


def test_yahoo_width_module_padded_rows_do_not_leak(yahoo_module):
    """lens = [9, 4]: the real rows of the padded query equal the restatement on the list of 4 alone, whatever the padding holds; with a
    cotangent that is zero on the padded rows so do their input gradients, and the padded rows' are exactly 0."""
    m, x, R, sd, _, _ = yahoo_module
    lens = [9, 4]
    x = x.clone()
    x[1, 4:] = 1e3 * torch.randn(5, 700)
    R = R.clone()
    R[1, 4:] = 0.0
    sd = {k: v.detach() for k, v in sd.items()}
    xd = x.to(DEV).requires_grad_(True)
    y = m(xd, lens=torch.tensor(lens, dtype=torch.int32, device=DEV))
    (y * R.to(DEV)).sum().backward()
    for b, n in enumerate(lens):
        xb = x[b:b + 1, :n].double().requires_grad_(True)
        yb = _mha_f64(xb, sd, 2)
        (yb * R[b:b + 1, :n].double()).sum().backward()
        G.assert_close(y[b, :n].detach().cpu().numpy(), yb[0].detach().numpy(), f"y[{b}]")
        G.assert_close(xd.grad[b, :n].cpu().numpy(), xb.grad[0].numpy(), f"dx[{b}]")
        assert float(xd.grad[b, n:].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ (d)
def _run_core(LS, Q, K, V, dO, H, lens, p=0.1):
    q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
    O = LS.mhsa_core(q, k, v, H, p_drop=p, seed=77, site=3, lens=lens)
    (O * dO).sum().backward()
    return O.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("B_,L,Fd,H,spill", [(2, 129, 700, 2, "1"), (2, 129, 700, 2, "0"), (2, 70, 176, 1, "1")])
def test_wide_repeats_are_bit_identical(LS, B_, L, Fd, H, spill, monkeypatch):
    monkeypatch.setenv("PTR_ATTN_DS_SPILL", spill)
    torch.manual_seed(L + Fd)
    Q, K, V, dO = (torch.randn(B_, L, Fd, device=DEV) for _ in range(4))
    lens = torch.tensor([L, L // 3], dtype=torch.int32, device=DEV)
    a, b = _run_core(LS, Q, K, V, dO, H, lens), _run_core(LS, Q, K, V, dO, H, lens)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    assert all(bool(torch.isfinite(t).all()) for t in a)


@pytest.mark.parametrize("B_,L,Fd,H", [(2, 70, 300, 2), (2, 130, 512, 2), (2, 40, 700, 2)])
def test_wide_packed_projection_equals_separate_tensors(LS, B_, L, Fd, H):
    torch.manual_seed(L)
    qkv = torch.randn(B_, L, 3 * Fd, device=DEV)
    g = torch.randn(B_, L, Fd, device=DEV)
    lens = torch.randint(1, L + 1, (B_,), device=DEV, dtype=torch.int32)
    qp = qkv.clone().requires_grad_(True)
    o1 = LS.mhsa_core_packed(qp, H, p_drop=0.1, seed=5, site=1, lens=lens)
    o1.backward(g)
    q, k, v = (qkv[..., i * Fd:(i + 1) * Fd].contiguous().requires_grad_(True) for i in range(3))
    o2 = LS.mhsa_core(q, k, v, H, p_drop=0.1, seed=5, site=1, lens=lens)
    o2.backward(g)
    assert torch.equal(o1, o2)
    assert torch.equal(qp.grad, torch.cat([q.grad, k.grad, v.grad], dim=-1))


@pytest.mark.parametrize("B_,L,Fd,H,use_lens", [(2, 256, 700, 2, False), (2, 130, 300, 2, True), (1, 200, 136, 1, True)])
def test_wide_backward_from_stored_dS_equals_the_recomputing_kernels(LS, B_, L, Fd, H, use_lens, monkeypatch):
    """As test_attention_backward_from_stored_dS_equals_the_recomputing_kernels holds the narrow forms: dK / dV bit-identical, dQ to fp32
    summation order (1e-5 of its scale)."""
    torch.manual_seed(L)
    Q, K, V, dO = (torch.randn(B_, L, Fd, device=DEV) for _ in range(4))
    lens = torch.tensor([L, max(1, L // 3)][:B_], dtype=torch.int32, device=DEV) if use_lens else None
    grads = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("PTR_ATTN_DS_SPILL", mode)
        grads[mode] = _run_core(LS, Q, K, V, dO, H, lens)[1:]
    assert torch.equal(grads["1"][1], grads["0"][1]) and torch.equal(grads["1"][2], grads["0"][2])
    d = (grads["1"][0] - grads["0"][0]).abs().max().item()
    scale = max(1.0, grads["0"][0].abs().max().item())
    assert d <= 1e-5 * scale, (d, scale)
    assert torch.isfinite(grads["1"][0]).all()


def test_wide_empty_query_and_scores_of_sixty(LS):
    """lens = 0 gives O = 0, LSE = 0 and zero gradients, never NaN; scores of about +-60 (3 sigma of N(0, 20^2)) stay finite."""
    from ptranking_amd import _lib
    torch.manual_seed(9)
    B_, L, Fd, H = 3, 70, 700, 2
    s = 20.0 ** 0.5
    q, k, v = (torch.randn(B_, L, Fd, device=DEV).requires_grad_(True) for _ in range(3))
    lens = torch.tensor([70, 0, 5], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        smax = float(((q * s) @ (k * s).transpose(1, 2)).abs().max()) / (Fd // H) ** 0.5
    assert smax > 60.0, smax
    o = LS.mhsa_core(q * s, k * s, v, H, p_drop=0.1, seed=3, site=0, lens=lens)
    o.sum().backward()
    assert torch.isfinite(o).all() and all(torch.isfinite(t.grad).all() for t in (q, k, v))
    assert float(o.detach()[1].abs().max()) == 0.0
    assert float(k.grad[1].abs().max()) == 0.0 and float(v.grad[1].abs().max()) == 0.0 and float(q.grad[1].abs().max()) == 0.0
    assert float(k.grad[2, 5:].abs().max()) == 0.0 and float(v.grad[2, 5:].abs().max()) == 0.0
    # the log-sum-exp of the empty query, through the C ABI
    Q = (q.detach() * s).contiguous()
    O = torch.full_like(Q, float("nan"))
    lse = torch.full((B_ * H * L,), float("nan"), device=DEV)
    _lib.call("ptr_mhsa_forward", _lib.ptr(Q), _lib.ptr((k.detach() * s).contiguous()), _lib.ptr(v.detach().contiguous()), Fd, _lib.ptr(lens),
              B_, L, Fd, H, C.c_float(0.0), C.c_uint64(0), 0, _lib.ptr(O), _lib.ptr(lse), _lib.current_stream(torch.device(DEV)))
    torch.cuda.synchronize()
    assert float(lse.view(B_, H, L)[1].abs().max()) == 0.0 and float(O[1].abs().max()) == 0.0 and bool(torch.isfinite(lse).all())


# ------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("ranker,F,H,enc", [("ListNet", 700, 2, "DASALC"), ("LambdaRank", 136, 1, "DASALC")])
def test_rankers_train_on_wide_heads(ranker, F, H, enc):
    """Five steps on a padded batch (B = 3, L = 9): the loss stays finite and ends below where it began, every gradient is finite.
    The same batch every step and dropout 0, so the objective is one deterministic function and "decreasing" is defined; Adagrad's first
    step moves EVERY coordinate by lr, and a 700-wide Linear sums 700 of them (0.01 moved the ListNet loss from 5.6 to 10.7 in two
    steps), so lr = 1e-4 keeps a step inside the first-order range.  Training-mode dropout on wide heads is pinned by the gates above."""
    import ptranking_amd as pa
    listsf = dict(num_features=F, ff_dims=[32], AF='R', TL_AF='GE', apply_tl_af=False, BN=False, bn_type='BN2', bn_affine=False, n_heads=H,
                  encoder_layers=1, encoder_type=enc, dropout=0.0)
    sf = dict(sf_id='listsf', opt='Adagrad', lr=1e-4, listsf=listsf)
    torch.manual_seed(4)
    kw = dict(model_para_dict={"sigma": 1.0}) if ranker == "LambdaRank" else {}
    r = getattr(pa, ranker)(sf_para_dict=copy.deepcopy(sf), gpu=True, device=DEV, **kw)
    r.init(); r.train_mode()
    lens = [9, 4, 6]
    X = torch.randn(3, 9, F, device=DEV)
    Y = torch.sort(torch.randint(0, 5, (3, 9), device=DEV).float(), dim=1, descending=True)[0].contiguous()
    for b, n in enumerate(lens):
        X[b, n:] = 0.0; Y[b, n:] = 0.0
        Y[b, 0] = max(float(Y[b, 0]), 1.0)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    losses = []
    for _ in range(5):
        loss, stop = r.train_op(X, Y, epoch_k=1, presort=True, label_type=pa.LABEL_TYPE.MultiLabel, lens=lens_t)
        assert torch.isfinite(loss) and not stop
        losses.append(float(loss.detach()))
        grads = [p.grad for p in r.get_parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    print(f"MEASURED {ranker} F={F} heads={H} losses {losses}")
    assert losses[-1] < losses[0], losses


# ------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("B_,L,Fd,H", [(2, 129, 136, 2), (2, 64, 256, 2)])
def test_narrow_heads_beside_the_wide_ones_are_bit_stable(LS, B_, L, Fd, H):
    torch.manual_seed(L + Fd)
    Q, K, V, dO = (torch.randn(B_, L, Fd, device=DEV) for _ in range(4))
    a, b = _run_core(LS, Q, K, V, dO, H, None), _run_core(LS, Q, K, V, dO, H, None)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
