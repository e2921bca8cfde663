"""CPU self-test of tests/f64_bounds.py: fp32 restatements of each dense primitive pass the element-wise float64 gate, and planted faults
— the kind a bf16x6 or a chunked-reduction kernel can make — fail it while the max-norm `close` the dense-layer GPU tests used before
passes them (the gap the element-wise gate closes)."""
import math

import pytest
import torch

import f64_bounds as B
import golden_util as G


def _bf16_planes(x):
    """x = p0 + p1 + p2 with bf16-representable planes (the operand split of the bf16x6 kernels)."""
    p0 = x.bfloat16().float()
    r = x - p0
    p1 = r.bfloat16().float()
    p2 = (r - p1).bfloat16().float()
    return p0, p1, p2


def _x6_matmul(a, b, drop_low_a=False):
    """a @ b in six bf16-plane products (i + j <= 2), fp32 accumulation; drop_low_a: the a2 * b0 product is missing."""
    A, Bp = _bf16_planes(a), _bf16_planes(b)
    pairs = [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1)] + ([] if drop_low_a else [(2, 0)])
    out = torch.zeros(a.shape[0], b.shape[1])
    for i, j in sorted(pairs, key=lambda t: -(t[0] + t[1])):        # small products first, as the kernels add them
        out += A[i] @ Bp[j]
    return out


@pytest.fixture(scope="module")
def data():
    X, info = B.structured_inputs(3000, 136, seed=3)
    W = B.weights(100, 136, seed=4)
    b = torch.randn(100)
    dY, zero_rows = B.structured_grads(3000, 100, seed=5)
    return X, W, b, dY, info, zero_rows


def test_structured_data_has_the_stated_features(data):
    X, W, b, dY, info, zero_rows = data
    assert bool((X[:, info["zero_col"]] == 0).all())
    assert X[:, info["const_col"]].unique().numel() == 1
    assert torch.equal(X[-375:], X[:375])
    for j in info["offset_cols"]:
        col = X[:, j].double()
        assert float(col.mean().abs()) > 500 * float(col.std())
    sc = X.abs().amax(0)
    assert float(sc.max() / sc[sc > 0].min()) > 2 ** 12                # column scales over many orders of magnitude
    assert bool((dY[zero_rows] == 0).all()) and int(zero_rows.sum()) >= 3000 // 16
    rs = dY.abs().amax(1)
    assert float(rs.max() / rs[rs > 0].min()) > 2 ** 8


def test_fp32_gemms_pass_the_gate(data):
    X, W, b, dY, info, zero_rows = data
    Z, E = B.gemm_fwd(X, W, b, B.C_FP32)
    B.gate(X @ W.t() + b, Z, E, "cpu fp32 fwd", B.C_FP32)
    B.gate(_x6_matmul(X, W.t()) + b, Z, B.gemm_fwd(X, W, b, B.C_X6)[1], "cpu bf16x6 fwd", B.C_X6)
    gt = torch.randn(3000, 136)
    G, EG = B.gemm_bwd_input(dY, W, B.C_FP32, gate=gt, p=0.1)
    B.gate((dY @ W) * (gt > 0).float() / 0.9, G, EG, "cpu fp32 bwd-input", B.C_FP32)
    dW, EdW, db, Edb = B.gemm_bwd_weight(X, dY, B.C_FP32)
    B.gate(dY.t() @ X, dW, EdW, "cpu fp32 dW", B.C_FP32)
    B.gate(dY.sum(0), db, Edb, "cpu fp32 db", B.C_FP32)
    B.gate(_x6_matmul(dY.t(), X), dW, B.gemm_bwd_weight(X, dY, B.C_X6)[1], "cpu bf16x6 dW", B.C_X6)


def test_dropped_bf16_plane_fails_the_gate_and_passes_close(data):
    X, W, b, dY, info, zero_rows = data
    Z, E = B.gemm_fwd(X, W, b, B.C_X6)
    bad = _x6_matmul(X, W.t(), drop_low_a=True) + b
    assert B.maxnorm_close(bad, Z, 2e-5)
    with pytest.raises(AssertionError, match="element-wise f64 bound failed"):
        B.gate(bad, Z, E, "planted: dropped plane fwd", B.C_X6)
    dW, EdW, _, _ = B.gemm_bwd_weight(X, dY, B.C_X6)
    badw = _x6_matmul(dY.t(), X, drop_low_a=True)
    assert B.maxnorm_close(badw, dW, 5e-5)
    with pytest.raises(AssertionError, match="element-wise f64 bound failed"):
        B.gate(badw, dW, EdW, "planted: dropped plane dW", B.C_X6)


def test_one_perturbed_small_column_fails_the_gate_and_passes_close(data):
    X, W, b, dY, info, zero_rows = data
    dW, EdW, _, _ = B.gemm_bwd_weight(X, dY, B.C_FP32)
    got = dY.t() @ X
    j = int(X.abs().amax(0).masked_fill(X.abs().amax(0) == 0, float("inf")).argmin())     # the smallest non-zero feature column
    got[:, j] *= 1.0 + 1e-3
    assert B.maxnorm_close(got, dW, 5e-5)
    with pytest.raises(AssertionError, match="element-wise f64 bound failed"):
        B.gate(got, dW, EdW, "planted: small column", B.C_FP32)


def test_exact_invariants_of_the_structured_data(data):
    X, W, b, dY, info, zero_rows = data
    dW = dY.t() @ X
    assert bool((dW[:, info["zero_col"]] == 0).all())                        # all-zero X column -> exactly-zero dW column
    assert bool(((dY @ W)[zero_rows] == 0).all())                            # zero dY row -> exactly-zero dX row


def _chunked_colsum(v, nblk, drop=None):
    """Column sums the way colsum2_kernel<1> + colsum2_reduce_kernel<0> form them: per-chunk partials, lane bl adds partials bl, bl + 32,
    bl + 64, bl + 96 per trip, the 32 lane sums in order.  drop: the partial index that goes missing."""
    R = v.shape[0]
    chunk = -(-R // nblk)
    parts = [v[i * chunk:(i + 1) * chunk].sum(0) if i * chunk < R else torch.zeros(v.shape[1]) for i in range(nblk)]
    if drop is not None:
        parts[drop] = torch.zeros_like(parts[drop])
    lanes = []
    for bl in range(32):
        s = torch.zeros(v.shape[1])
        for b0 in range(bl, nblk, 128):
            q = [parts[b0 + k * 32] if b0 + k * 32 < nblk else torch.zeros(v.shape[1]) for k in range(4)]
            s = s + ((q[0] + q[1]) + (q[2] + q[3]))
        lanes.append(s)
    t = torch.zeros(v.shape[1])
    for s in lanes:
        t = t + s
    return t


def test_dropped_partial_of_a_chunked_sum_fails_the_gate_and_passes_close():
    """Column sums over 32 768 rows in 512 partials (the batch-norm backward's dbeta / dgamma), column scales 2^-12..1: one partial whose
    rows only carry the small columns (sparse features, padded documents) goes missing."""
    R, N, nblk, small = 32768, 100, 512, 500
    g = torch.Generator().manual_seed(7)
    e = torch.randint(-12, 1, (N,), generator=g)
    e[0], e[1] = 0, -12
    dY = torch.randn(R, N, generator=g) * torch.pow(2.0, e.float())
    dY[small * 64:(small + 1) * 64, e > -11] = 0.0
    _, _, db, Edb = B.gemm_bwd_weight(torch.zeros(R, 4), dY, B.C_BNACT)
    B.gate(_chunked_colsum(dY, nblk), db, Edb, "cpu chunked colsum", B.C_BNACT)
    bad = _chunked_colsum(dY, nblk, drop=small)
    assert B.maxnorm_close(bad, db, 5e-5)
    with pytest.raises(AssertionError, match="element-wise f64 bound failed"):
        B.gate(bad, db, Edb, "planted: dropped partial", B.C_BNACT)


def _fp32_bn_stats(z, eps=1e-5, empty_chunk_bug=False):
    """colsum2_kernel<0> + colsum2_reduce_kernel<1> restated in fp32 torch ops (pivoted chunk sums, parallel-variance combination).
    empty_chunk_bug: a chunk that starts past R counts min(R, end) - start (negative) rows in the variance."""
    R, N = z.shape
    nb = B.bn_blocks(R)
    chunk = -(-R // nb)
    means, m2s, ns = [], [], []
    for i in range(nb):
        s = z[i * chunk:(i + 1) * chunk]
        if s.shape[0] == 0:
            means.append(torch.zeros(N)); m2s.append(torch.zeros(N)); ns.append(float(min(R, (i + 1) * chunk) - i * chunk) if empty_chunk_bug else 0.0)
            continue
        k = s[0]
        d = s - k
        s1, s2 = d.sum(0), (d * d).sum(0)
        m1 = s1 / s.shape[0]
        m2s.append((s2 - s1 * m1).clamp(min=0)); means.append(k + m1); ns.append(float(s.shape[0]))
    mean = torch.stack([n * m for n, m in zip(ns, means)]).sum(0) / R          # a tree over the chunks, as the finishing kernel's lanes
    m2 = torch.stack([q + n * (m - mean) ** 2 for n, m, q in zip(ns, means, m2s)]).sum(0)
    return mean, 1.0 / torch.sqrt(m2 / R + eps)


def test_fp32_bn_statistics_pass_and_an_empty_chunk_with_negative_rows_fails():
    """512 chunks of 257 rows over 131 073 rows: the last chunk starts past R.  Counting min(R, end) - start = -254 rows for it subtracts
    254 mean^2 from M2 — at a mean of 3 standard deviations a finite rstd about 1 % too large, which the bound catches."""
    torch.manual_seed(11)
    R, N = 131073, 8
    z = (3.0 + torch.randn(R, N)) * torch.pow(2.0, torch.arange(N) - 4.0)
    mean, rstd, Em, Er = B.bn_stats(z, B.C_BNACT)
    m32, r32 = _fp32_bn_stats(z)
    B.gate(m32, mean[0], Em[0], "cpu fp32 bn mean", B.C_BNACT)
    B.gate(r32, rstd[0], Er[0], "cpu fp32 bn rstd", B.C_BNACT)
    _, rbad = _fp32_bn_stats(z, empty_chunk_bug=True)
    assert bool(torch.isfinite(rbad).all())
    assert float((rbad.double() / rstd[0] - 1).abs().min()) > 5e-3
    with pytest.raises(AssertionError, match="element-wise f64 bound failed"):
        B.gate(rbad, rstd[0], Er[0], "planted: empty chunk", B.C_BNACT)


@pytest.mark.parametrize("af", [B.AF_NONE, B.AF_RELU, B.AF_LEAKY, B.AF_ELU, B.AF_SELU, B.AF_GELU, B.AF_SIGMOID, B.AF_TANH], ids=B.AF_NAMES.get)
def test_fp32_bnact_forward_and_backward_pass_the_gate(af):
    torch.manual_seed(af)
    R, N = 4000, 24
    z = (torch.randn(1, N) * 50 + torch.randn(R, N) * torch.rand(1, N) * 3).float()
    mean, rstd = z.double().mean(0).float(), (1.0 / torch.sqrt(z.double().var(0, unbiased=False) + 1e-5)).float()
    gamma, beta = torch.randn(N), torch.randn(N)
    acts = {B.AF_NONE: lambda y: y, B.AF_RELU: torch.relu, B.AF_LEAKY: lambda y: torch.nn.functional.leaky_relu(y, 0.01),
            B.AF_ELU: torch.nn.functional.elu, B.AF_SELU: torch.selu, B.AF_GELU: torch.nn.functional.gelu, B.AF_SIGMOID: torch.sigmoid,
            B.AF_TANH: torch.tanh}
    y32 = ((z - mean) * rstd * gamma + beta).requires_grad_(True)
    a32 = acts[af](y32)
    a, Ea, acc = B.bnact_fwd(z, mean, rstd, gamma, beta, af, B.C_BNACT)
    B.gate(a32, a, Ea, f"cpu fp32 bnact fwd {B.AF_NAMES[af]}", B.C_BNACT, accept=B.accept_from(a32, acc))
    da = torch.randn(R, N)
    ref = B.bnact_bwd(z, da, mean, rstd, gamma, beta, af, B.C_BNACT)
    da = da.masked_fill(ref["amb"], 0.0)
    ref = B.bnact_bwd(z, da, mean, rstd, gamma, beta, af, B.C_BNACT)
    a32.backward(da)
    dy = y32.grad
    xh = (z - mean) * rstd
    sdy, sdyx = dy.sum(0), (dy * xh).sum(0)
    dz = gamma * rstd * (dy - sdy / R - xh * (sdyx / R))
    B.gate(dz, ref["dz"], ref["E_dz"], f"cpu fp32 bnact bwd dz {B.AF_NAMES[af]}", B.C_BNACT)
    B.gate(sdyx, ref["dgamma"], ref["E_dgamma"], f"cpu fp32 bnact bwd dgamma {B.AF_NAMES[af]}", B.C_BNACT)
    B.gate(sdy, ref["dbeta"], ref["E_dbeta"], f"cpu fp32 bnact bwd dbeta {B.AF_NAMES[af]}", B.C_BNACT)


def test_bn_as_z_times_r_minus_mu_times_r_fails_the_gate_and_passes_close():
    torch.manual_seed(12)
    R, N = 4000, 24
    z = (300.0 + torch.randn(R, N)).float()                    # mean ~300 standard deviations
    mean, rstd = z.double().mean(0).float(), (1.0 / torch.sqrt(z.double().var(0, unbiased=False) + 1e-5)).float()
    a, Ea, _ = B.bnact_fwd(z, mean, rstd, None, None, B.AF_NONE, B.C_BNACT)
    B.gate((z - mean) * rstd, a, Ea, "cpu fp32 bn (z - mu) r", B.C_BNACT)
    bad = z * rstd - mean * rstd
    assert B.maxnorm_close(bad, a, 2e-5)
    with pytest.raises(AssertionError, match="element-wise f64 bound failed"):
        B.gate(bad, a, Ea, "planted: z r - mu r", B.C_BNACT)


def test_relu_chain_bounds_pass_an_fp32_mlp_with_dropout():
    torch.manual_seed(13)
    R, F, NL = 2000, 136, 3
    X, _ = B.structured_inputs(R, F, seed=14)
    Ws = [B.weights(100, F, seed=15)] + [B.weights(100, 100, seed=16 + l) for l in range(NL - 1)] + [B.weights(1, 100, seed=20)]
    bs = [torch.randn(w.shape[0]) * 0.1 for w in Ws]
    masks = [(torch.rand(R, F) > 0.1).float()] + [(torch.rand(R, 100) > 0.1).float() for _ in range(NL - 1)]
    p = 0.1
    fwd = B.relu_mlp(X, Ws, bs, B.C_FP32, masks=masks, p=p)
    assert fwd["amb_frac"] <= B.MAX_AMBIGUOUS
    dout = torch.randn(R).masked_fill(fwd["amb_rows"], 0.0)
    ref = B.relu_mlp(X, Ws, bs, B.C_FP32, masks=masks, p=p, dout=dout)
    Wp = [w.clone().requires_grad_(True) for w in Ws]
    bp = [b.clone().requires_grad_(True) for b in bs]

    def run():
        h = X * masks[0] / (1 - p)
        for l in range(NL):
            h = torch.relu(h @ Wp[l].t() + bp[l])
            if l < NL - 1:
                h = h * masks[l + 1] / (1 - p)
        return (h @ Wp[NL].t() + bp[NL])[:, 0]

    out = run()
    B.gate(out, ref["out"], ref["E_out"], "cpu fp32 mlp out", B.C_FP32)
    out.backward(dout)
    for l in range(NL + 1):
        B.gate(Wp[l].grad, ref["dW"][l], ref["E_dW"][l], f"cpu fp32 mlp dW{l}", B.C_FP32)
        B.gate(bp[l].grad, ref["db"][l], ref["E_db"][l], f"cpu fp32 mlp db{l}", B.C_FP32)


# ---------------------------------------------------------------------------------------------------------------------------- attention
def _fp32_mhsa_fwd(Q, K, V, H, keep, p, lens, KC=32, lens_off=0):
    """mhsa_fwd_kernel restated in fp32 torch ops: online softmax over KC-key chunks (running max, rescaled sum and accumulator),
    O = acc (1 / (1-p)) / l, LSE = m + log l.  lens_off: the key mask reaches lens + lens_off keys (planted fault).  Returns (O, LSE)."""
    Bn, L, F = Q.shape
    dh = F // H
    s = torch.tensor(1.0 / math.sqrt(dh), dtype=torch.float32)
    hv = lambda T: T.reshape(Bn, L, H, dh).permute(0, 2, 1, 3)
    q, k, v = hv(Q), hv(K), hv(V)
    kinv = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32) if keep is not None else torch.tensor(1.0)
    O, LSE = torch.zeros(Bn, H, L, dh), torch.zeros(Bn, H, L)
    for b in range(Bn):
        n = min(L, int(lens[b]) + lens_off) if lens is not None else L
        m, l, acc = torch.full((H, L, 1), -math.inf), torch.zeros(H, L, 1), torch.zeros(H, L, dh)
        for kc in range(0, n, KC):
            ke = min(n, kc + KC)
            S = (q[b] @ k[b, :, kc:ke].transpose(-1, -2)) * s
            m_new = torch.maximum(m, S.amax(-1, keepdim=True))
            corr = torch.exp(m - m_new)
            e = torch.exp(S - m_new)
            rs = e.sum(-1, keepdim=True)
            if keep is not None:
                e = e * keep[b, :, :, kc:ke]
            l, m = l * corr + rs, m_new
            acc = acc * corr + e @ v[b, :, kc:ke]
        if n > 0:
            O[b] = acc * (kinv / l)
            LSE[b] = (m + torch.log(l))[..., 0]
    return O.permute(0, 2, 1, 3).reshape(Bn, L, F), LSE


def _fp32_mhsa_bwd(Q, K, V, O, dO, lse, H, keep, p, lens, lens_off=0, ds_twice_tail=False, d_bf16=False):
    """The backward kernels restated in fp32: P = exp(S - lse), D = rowsum(O dO), dS = P (dP keep' - D) s, dQ = dS K, dK = dS^T Q,
    dV = P'^T dO.  Planted faults: lens_off (key mask off by lens_off keys), ds_twice_tail (the last head's dS scaled by s twice),
    d_bf16 (D from a bf16-rounded O).  Returns (dQ, dK, dV)."""
    Bn, L, F = Q.shape
    dh = F // H
    s = torch.tensor(1.0 / math.sqrt(dh), dtype=torch.float32)
    hv = lambda T: T.reshape(Bn, L, H, dh).permute(0, 2, 1, 3)
    mg = lambda T: T.permute(0, 2, 1, 3).reshape(Bn, L, F)
    q, k, v, o, g = hv(Q), hv(K), hv(V), hv(O.bfloat16().float() if d_bf16 else O), hv(dO)
    n = (lens.long() + lens_off).clamp(max=L) if lens is not None else torch.full((Bn,), L)
    ok = (torch.arange(L)[None, :] < n[:, None]).reshape(Bn, 1, 1, L)
    S = (q @ k.transpose(-1, -2)) * s
    P = torch.where(ok, torch.exp(S - lse.reshape(Bn, H, L, 1)), torch.zeros(1))
    D = (o * g).sum(-1, keepdim=True)
    dP = g @ v.transpose(-1, -2)
    kp = keep * torch.tensor(1.0 / (1.0 - p), dtype=torch.float32) if keep is not None else torch.ones(1)
    dS = P * (dP * kp - D) * s
    if ds_twice_tail:
        dS[:, H - 1] = dS[:, H - 1] * s
    return mg(dS @ k), mg(dS.transpose(-1, -2) @ q), mg((P * kp).transpose(-1, -2) @ g)


def _keep_mask(Bn, H, L, p, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(Bn, H, L, L, generator=g) >= p).float()


def _attn_gate(Q, K, V, dO, H, keep, p, lens, what, **faults):
    """fp32 forward + backward (with faults) through the f64 gates of mhsa_fwd and mhsa_bwd (given the fp32 O and LSE)."""
    fwd_faults = {k: v for k, v in faults.items() if k == "lens_off"}
    O, LSE = _fp32_mhsa_fwd(Q, K, V, H, keep, p, lens, **fwd_faults)
    rO, EO, rL, EL = B.mhsa_fwd(Q, K, V, H, keep, p, lens, B.C_ATTN)
    B.gate(O, rO, EO, f"{what} O", B.C_ATTN)
    B.gate(LSE, rL, EL, f"{what} LSE", B.C_ATTN)
    dQ, dK, dV = _fp32_mhsa_bwd(Q, K, V, O, dO, LSE, H, keep, p, lens, **faults)
    ref = B.mhsa_bwd(Q, K, V, O, dO, LSE, H, keep, p, lens, B.C_ATTN)
    B.gate(dV, ref["dV"], ref["E_dV"], f"{what} dV", B.C_ATTN)
    B.gate(dK, ref["dK"], ref["E_dK"], f"{what} dK", B.C_ATTN)
    B.gate(dQ, ref["dQ"], ref["E_dQ"], f"{what} dQ", B.C_ATTN)
    return O, dQ, dK, dV


@pytest.mark.parametrize("Bn,L,F,H,mode", [(3, 200, 136, 2, "lens"), (2, 97, 200, 2, "dropout"), (3, 70, 17, 1, "dropout+lens"),
                                           (1, 33, 64, 4, "eval")])
def test_fp32_attention_passes_the_gate(Bn, L, F, H, mode):
    Q, K, V, dO, lens = B.attn_inputs(Bn, L, F, H, seed=L)
    p = 0.1 if "dropout" in mode else 0.0
    keep = _keep_mask(Bn, H, L, p, L) if p else None
    _attn_gate(Q, K, V, dO, H, keep, p, lens if "lens" in mode else None, f"cpu fp32 attention {mode}")


def _torch_ref_attention(Q, K, V, dO, H, lens):
    """The fp32 reference the existing oracle tests compare with (oracle/torch_ref.py, autograd)."""
    from oracle import torch_ref as T
    qc, kc, vc = (t.clone().requires_grad_(True) for t in (Q, K, V))
    out = T.mhsa_core_ref(qc, kc, vc, H, lens=lens)
    (out * dO).sum().backward()
    return out.detach(), qc.grad, kc.grad, vc.grad


def test_attention_lens_off_by_one_fails_the_gate_and_passes_close():
    """The key mask admits key lens[b] too, a key with small K and V: in a peaked head (|S| up to ~50) its probability is ~e^-20 or
    less, so O and the gradients of the real keys move far below 1e-5; but the padded key's dK / dV rows are no longer exactly 0."""
    Bn, L, F, H = 3, 100, 40, 1
    Q, K, V, dO, _ = B.attn_inputs(Bn, L, F, H, seed=4)
    Q *= 0.8
    lens = torch.tensor([L, L, 60], dtype=torch.int32)
    K[2, 60] *= 1e-3
    V[2, 60] *= 1e-3
    ref = _torch_ref_attention(Q, K, V, dO, H, lens)
    with pytest.raises(AssertionError, match="element-wise f64 bound failed"):
        _attn_gate(Q, K, V, dO, H, None, 0.0, lens, "planted: lens off by one", lens_off=1)
    O, LSE = _fp32_mhsa_fwd(Q, K, V, H, None, 0.0, lens, lens_off=1)
    dQ, dK, dV = _fp32_mhsa_bwd(Q, K, V, O, dO, LSE, H, None, 0.0, lens, lens_off=1)
    assert float(dV[2, 60].abs().max()) > 0
    for name, a, r in zip(("O", "dQ", "dK", "dV"), (O, dQ, dK, dV), ref):
        G.assert_close(a.numpy(), r.numpy(), f"planted: lens off by one {name}")


def test_attention_ds_scaled_twice_on_a_tail_head_fails_the_gate_and_passes_close():
    """dS of the last head multiplied by 1/sqrt(dh) once more: the tail head's dQ / dK are 10x too small, but its V is 2^-18 of the
    other head's, so they sit under the old gate's floor of 1e-6 x max."""
    Bn, L, F, H = 2, 130, 200, 2
    Q, K, V, dO, lens = B.attn_inputs(Bn, L, F, H, seed=3)
    V[..., 100:] *= 2.0 ** -18
    ref = _torch_ref_attention(Q, K, V, dO, H, None)
    with pytest.raises(AssertionError, match="element-wise f64 bound failed"):
        _attn_gate(Q, K, V, dO, H, None, 0.0, None, "planted: dS scaled twice", ds_twice_tail=True)
    O, LSE = _fp32_mhsa_fwd(Q, K, V, H, None, 0.0, None)
    dQ, dK, dV = _fp32_mhsa_bwd(Q, K, V, O, dO, LSE, H, None, 0.0, None, ds_twice_tail=True)
    for name, a, r in zip(("O", "dQ", "dK", "dV"), (O, dQ, dK, dV), ref):
        G.assert_close(a.numpy(), r.numpy(), f"planted: dS scaled twice {name}")


def test_attention_d_from_bf16_output_fails_the_gate():
    Bn, L, F, H = 2, 130, 136, 2
    Q, K, V, dO, lens = B.attn_inputs(Bn, L, F, H, seed=4)
    with pytest.raises(AssertionError, match="element-wise f64 bound failed"):
        _attn_gate(Q, K, V, dO, H, None, 0.0, lens, "planted: D from bf16 O", d_bf16=True)


# ---------------------------------------------------------------------------------------------------------------------------- LayerNorm
def _fp32_ln_fwd(x, a2, b2, eps=1e-6, one_pass=False):
    """layernorm_fwd_kernel restated in fp32: two-pass mean and unbiased variance (one_pass: (sum x^2 - mean sum x) / (F - 1), planted),
    eps added to sd.  Returns (y, stats [R, 3] = {mean, 1 / (sd + eps), sd})."""
    F = x.shape[1]
    mean = x.sum(1, keepdim=True) / F
    if one_pass:
        var = ((x * x).sum(1, keepdim=True) - mean * x.sum(1, keepdim=True)).clamp(min=0) / (F - 1)
    else:
        c = x - mean
        var = (c * c).sum(1, keepdim=True) / (F - 1)
    sd = torch.sqrt(var)
    rinv = 1.0 / (sd + eps)
    return a2 * (x - mean) * rinv + b2, torch.cat([mean, rinv, sd], 1)


def _ln_reduce(part):
    """layernorm_reduce_kernel's order: lane sl (16 of them) adds partials sl, sl + 16, sl + 32, sl + 48 per trip of 64; then the 16
    lane sums in lane order."""
    nblk = part.shape[0]
    at = lambda k: part[k] if k < nblk else torch.zeros(part.shape[1])
    t = torch.zeros(part.shape[1])
    for sl in range(16):
        s = torch.zeros(part.shape[1])
        for k in range(sl, nblk, 64):
            s = s + ((at(k) + at(k + 16)) + (at(k + 32) + at(k + 48)))
        t = t + s
    return t


def _fp32_ln_bwd(x, a2, dy, stats, drop_part=None):
    """layernorm_bwd_kernel + layernorm_reduce_kernel restated in fp32 (per-block partials of da / db over rows r with
    (r / 4) % blocks == block, blocks = min(ceil(R / 4), 1024)).  drop_part: that block's partial goes missing (planted).
    Returns (dx, da, db)."""
    R, F = x.shape
    mean, rinv, sd = stats[:, 0:1], stats[:, 1:2], stats[:, 2:3]
    c = x - mean
    gg = dy * a2
    gbar = gg.sum(1, keepdim=True) / F
    k2 = torch.where(sd > 0, rinv * rinv * (gg * c).sum(1, keepdim=True) / (sd * (F - 1)), torch.zeros(1))
    dx = rinv * (gg - gbar) - c * k2
    nblk = min(-(-R // 4), 1024)
    blk = (torch.arange(R) // 4) % nblk
    pa = torch.zeros(nblk, F).index_add_(0, blk, dy * c * rinv)
    pb = torch.zeros(nblk, F).index_add_(0, blk, dy)
    if drop_part is not None:
        pa[drop_part] = 0.0
        pb[drop_part] = 0.0
    return dx, _ln_reduce(pa), _ln_reduce(pb)


def _ln_gate(x, a2, b2, dy, what, eps=1e-6, **faults):
    y, st = _fp32_ln_fwd(x, a2, b2, eps, one_pass=faults.get("one_pass", False))
    ry, Ey, rst = B.layernorm_fwd(x, a2, b2, eps, B.C_LN)
    B.gate(st[:, 0], rst["mean"], rst["E_mean"], f"{what} mean", B.C_LN)
    B.gate(st[:, 2], rst["sd"], rst["E_sd"], f"{what} sd", B.C_LN)
    B.gate(st[:, 1], rst["rinv"], rst["E_rinv"], f"{what} rinv", B.C_LN)
    B.gate(y, ry, Ey, f"{what} y", B.C_LN)
    dx, da, db = _fp32_ln_bwd(x, a2, dy, st, drop_part=faults.get("drop_part"))
    ref = B.layernorm_bwd(x, a2, dy, st, B.C_LN)
    B.gate(dx, ref["dx"], ref["E_dx"], f"{what} dx", B.C_LN)
    B.gate(da, ref["da"], ref["E_da"], f"{what} da", B.C_LN)
    B.gate(db, ref["db"], ref["E_db"], f"{what} db", B.C_LN)
    return y, dx, da, db


def test_layernorm_inputs_have_the_stated_rows():
    x, a2, b2, dy, kinds = B.ln_inputs(5000, 136, seed=1)
    xd = x.double()
    sd, mean = xd.std(1), xd.mean(1)
    assert bool((mean[kinds == 1].abs() > 50 * sd[kinds == 1]).all())
    assert bool((sd[kinds == 2] < 1e-5 * mean[kinds == 2].abs()).all())
    assert bool((sd[kinds >= 3] == 0).all()) and bool((x[kinds == 5] == 0).all())
    assert all(int((kinds == k).sum()) > 10 for k in range(6))


@pytest.mark.parametrize("R,F", [(3000, 136), (700, 24), (300, 700), (64, 2), (4101, 65)])
def test_fp32_layernorm_passes_the_gate(R, F):
    x, a2, b2, dy, _ = B.ln_inputs(R, F, seed=R + F)
    _ln_gate(x, a2, b2, dy, f"cpu fp32 layernorm R={R} F={F}")


def _torch_ref_layernorm(x, a2, b2, dy):
    from oracle import torch_ref as T
    xc, ac, bc = (t.clone().requires_grad_(True) for t in (x, a2, b2))
    y = T.layer_norm_ref(xc, ac, bc)
    (y * dy).sum().backward()
    return y.detach(), xc.grad, ac.grad, bc.grad


def test_one_pass_layernorm_variance_fails_the_gate_and_passes_close():
    """var = (sum x^2 - mean sum x) / (F - 1) on rows whose mean is 5 standard deviations: the roundings of sum x^2 ~ 26 F var move
    the variance by a few 1e-6 relative — under the 1e-5 of the fp32 comparison, over the two-pass bound."""
    g = torch.Generator().manual_seed(21)
    R, F = 2000, 136
    x = 5.0 + torch.randn(R, F, generator=g)
    a2, b2, dy = torch.randn(F, generator=g), torch.randn(F, generator=g), torch.randn(R, F, generator=g)
    _ln_gate(x, a2, b2, dy, "cpu fp32 layernorm offset 5 sd")
    y, st = _fp32_ln_fwd(x, a2, b2, one_pass=True)
    dx, da, db = _fp32_ln_bwd(x, a2, dy, st)
    for name, got, r in zip(("y", "dx", "da", "db"), (y, dx, da, db), _torch_ref_layernorm(x, a2, b2, dy)):
        G.assert_close(got.numpy(), r.numpy(), f"planted: one-pass variance {name}")
    with pytest.raises(AssertionError, match="element-wise f64 bound failed"):
        _ln_gate(x, a2, b2, dy, "planted: one-pass variance", one_pass=True)


def test_dropped_layernorm_partial_fails_the_gate_and_passes_close():
    """32 768 rows in 1024 partials of 32 rows, dy columns scaled 2^-20..1: one partial whose rows carry only the columns below 2^-17 goes
    missing from da / db."""
    g = torch.Generator().manual_seed(22)
    R, F, drop = 32768, 100, 500
    x = torch.randn(R, F, generator=g)
    a2, b2 = torch.randn(F, generator=g), torch.randn(F, generator=g)
    e = torch.randint(-20, 1, (F,), generator=g)
    e[0], e[1] = 0, -20
    dy = torch.randn(R, F, generator=g) * torch.pow(2.0, e.float())
    rows = ((torch.arange(R) // 4) % 1024) == drop
    dy[rows.nonzero()[:, 0][:, None], (e > -18).nonzero()[:, 0][None, :]] = 0.0
    _ln_gate(x, a2, b2, dy, "cpu fp32 layernorm 1024 partials")
    y, st = _fp32_ln_fwd(x, a2, b2)
    dx, da, db = _fp32_ln_bwd(x, a2, dy, st, drop_part=drop)
    for name, got, r in zip(("y", "dx", "da", "db"), (y, dx, da, db), _torch_ref_layernorm(x, a2, b2, dy)):
        G.assert_close(got.numpy(), r.numpy(), f"planted: dropped partial {name}")
    with pytest.raises(AssertionError, match="element-wise f64 bound failed"):
        _ln_gate(x, a2, b2, dy, "planted: dropped partial", drop_part=drop)


# ---------------------------------------------------------------------------------------------------------------------------- losses
# tests/f64_loss_bounds.py: the C oracle (the reference's arithmetic in fp32, oracle/ltr_oracle.c) passes every loss gate on the
# generated inputs; planted faults pass the rule the loss tests use (golden_util.assert_close on the batch total and the gradient,
# tests/test_parity_gpu.py loss_and_grad) and fail the new gates.
import numpy as np  # noqa: E402

import f64_loss_bounds as FL  # noqa: E402


def _oracle():
    from oracle import c_oracle
    return c_oracle


def _old_rule_passes(total, total_ref, grad, grad_ref):
    try:
        G.assert_close(np.array(total), np.array(total_ref), "loss")
        G.assert_close(grad, grad_ref, "grad")
        return True
    except AssertionError:
        return False


@pytest.mark.parametrize("L,kw", [(16, {}), (100, dict(quantise=True, offset=1000.0)), (40, dict(mix="yahoo", lens="full"))],
                         ids=["L16", "L100-quant-offset", "L40-yahoo-full"])
def test_oracle_pair_losses_pass_the_gate(L, kw):
    O = _oracle()
    p, y, n, screened = FL.pair_inputs(48, L, seed=L, **kw)
    assert screened <= FL.MAX_SCREENED
    for name, fn, ref in (("ranknet", O.ranknet, FL.ranknet), ("lambdarank", O.lambdarank, FL.lambdarank)):
        lq, g = fn(p, y, 1.0, n)
        r = ref(p, y, n, 1.0, FL.C_PAIR)
        FL.gate_losses(lq, g, r, f"oracle {name} L{L}", FL.C_PAIR, float(lq.astype(np.float64).sum()), FL.batch_total(r, FL.C_PAIR))
    assert np.isnan(FL.lambdarank(p, y, n, 1.0)["loss_q"][2])              # query 2 has no relevant document


@pytest.mark.parametrize("presort,couple", [(1, 1), (0, 1), (1, 0), (0, 0)])
def test_oracle_approxndcg_passes_the_gate(presort, couple):
    O = _oracle()
    p, y, n, _ = FL.pair_inputs(40, 60, sigma=10.0, seed=5, quantise=bool(presort), offset=1000.0 * presort, every_relevant=bool(couple))
    if not couple:              # a one-document query without a relevant one: the oracle gives 0 * 1 / 0 = 0 there, the kernel NaN
        n[5:] = np.maximum(n[5:], 2)
    lo, dcg, inv, g = O.approxndcg(p, y, 10.0, bool(presort), bool(couple), n)
    r = FL.approxndcg(p, y, n, 10.0, bool(presort), bool(couple), 0.0, FL.C_APPROX)
    c = FL.C_APPROX
    FL.gate_nan(dcg, r["dcg_q"], r["E_dcg_q"], "oracle approxndcg dcg_q", c)
    FL.gate_nan(inv, r["inv_idcg_q"], r["E_inv_idcg_q"], "oracle approxndcg inv_idcg_q", c)
    FL.gate_nan(g, r["grad"], r["E_grad"], "oracle approxndcg grad", c)
    FL.gate_nan([lo], [r["loss"]], [r["E_loss"]], "oracle approxndcg loss", c)


@pytest.mark.parametrize("L,offset", [(20, 0.0), (64, 1000.0), (130, 0.0)])
def test_oracle_listwise_losses_pass_the_gate(L, offset):
    O = _oracle()
    p, y, n = FL.listwise_inputs(40, L, seed=L, offset=offset)
    perm = FL.listmle_perm(y, n)
    c = FL.C_LIST
    for name, got, ref in (("listnet", O.listnet(p, y, n), FL.listnet(p, y, n, c)),
                           ("listmle", O.listmle(p, perm, n), FL.listmle(p, perm, n, c)),
                           ("rankmse", O.rankmse(p, y, n), FL.rankmse(p, y, n, c)),
                           ("rankcosine", O.rankcosine(p, y, n), FL.rankcosine(p, y, n, c))):
        FL.gate_losses(got[0], got[1], ref, f"oracle {name} L{L}", c)
    assert FL.rankcosine(p, y, n, c)["loss_q"][4] == 2.0                    # zero-length query: (1 - 0) / 0.5


def test_lambdarank_loss_with_a_slightly_wrong_ln2_fails_the_gate_and_passes_the_old_rule():
    """The ring kernel scales its log2-domain loss by ln2 / sigma once per query: a ln2 3e-6 off is a relative bias below the old 1e-5."""
    O = _oracle()
    p, y, n, _ = FL.pair_inputs(64, 128, seed=3, specials=False)
    lq, g = O.lambdarank(p, y, 1.0, n)
    bad = (lq.astype(np.float64) * (1.0 + 3e-6)).astype(np.float32)
    assert _old_rule_passes(bad.astype(np.float64).sum(), lq.astype(np.float64).sum(), g, g)
    r = FL.lambdarank(p, y, n, 1.0, FL.C_PAIR)
    FL.gate_losses(lq, g, r, "lambdarank oracle", FL.C_PAIR)
    with pytest.raises(AssertionError, match="loss_q"):
        FL.gate_losses(bad, g, r, "lambdarank ln2 off", FL.C_PAIR)


def test_one_wrong_query_loss_in_a_bench_sized_batch_fails_the_gate_and_passes_the_old_rule():
    """RankNet, B = 4096: one query's loss_q 2 % off (the first query of a slot past a workgroup boundary) moves the batch total by ~5e-6."""
    O = _oracle()
    p, y, n, _ = FL.pair_inputs(4096, 8, seed=12, specials=False)
    lq, g = O.ranknet(p, y, 1.0, n)
    bad = lq.copy()
    bad[17 * 16] *= np.float32(1.02)
    assert _old_rule_passes(bad.astype(np.float64).sum(), lq.astype(np.float64).sum(), g, g)
    r = FL.ranknet(p, y, n, 1.0, FL.C_PAIR)
    FL.gate_losses(lq, g, r, "ranknet oracle", FL.C_PAIR)
    with pytest.raises(AssertionError, match="loss_q"):
        FL.gate_losses(bad, g, r, "ranknet one query off", FL.C_PAIR)


def test_approxndcg_inv_idcg_in_the_neighbours_slot_fails_the_gate():
    """inv_idcg_q of a workgroup's last query (4 per workgroup) written to its neighbour's slot: no test read these slots before, so the
    loss and the gradients — all the old rule saw — are the oracle's own."""
    O = _oracle()
    p, y, n, _ = FL.pair_inputs(24, 40, sigma=10.0, seed=13, every_relevant=True)
    lo, dcg, inv, g = O.approxndcg(p, y, 10.0, True, True, n)
    bad = inv.copy()
    bad[8] = inv[7]                 # no test read inv_idcg_q before: the loss and the gradients, all the old rule saw, are untouched
    r = FL.approxndcg(p, y, n, 10.0, True, True, 0.0, FL.C_APPROX)
    FL.gate_nan(inv, r["inv_idcg_q"], r["E_inv_idcg_q"], "inv_idcg_q oracle", FL.C_APPROX)
    with pytest.raises(AssertionError):
        FL.gate_nan(bad, r["inv_idcg_q"], r["E_inv_idcg_q"], "inv_idcg_q in the neighbour's slot", FL.C_APPROX)


def test_listnet_normaliser_with_a_low_precision_log_fails_the_gate_and_passes_the_old_rule():
    """ListNet with log Z carrying 2^-16 relative error (a short log approximation): every query's loss moves by ~1.5e-5 absolute."""
    O = _oracle()
    p, y, n = FL.listwise_inputs(64, 64, seed=14)
    lq, g = O.listnet(p, y, n)
    zs = np.array([np.exp(p[q, :n[q]].astype(np.float64) - p[q, :n[q]].max()).sum() if n[q] else 1.0 for q in range(len(n))])
    bad = (lq + np.where(n > 0, np.log(zs) * 2.0 ** -16, 0.0)).astype(np.float32)
    assert _old_rule_passes(bad.astype(np.float64).sum(), lq.astype(np.float64).sum(), g, g)
    r = FL.listnet(p, y, n, FL.C_LIST)
    FL.gate_losses(lq, g, r, "listnet oracle", FL.C_LIST)
    with pytest.raises(AssertionError, match="loss_q"):
        FL.gate_losses(bad, g, r, "listnet low-precision log", FL.C_LIST)


def _fixture_cases():
    """(name, family, case) of the reference's own fp32 outputs that the loss gates cover (losses_knife.npz, the threshold band, is not
    among them)."""
    out = []
    for f in ("losses.npz", "losses_big.npz", "losses_long.npz", "siblings.npz"):
        for fam, cases in G._load(f).items():
            if fam in ("ranknet", "lambdarank", "approxndcg", "listnet", "listmle", "rankmse", "rankcosine"):
                out += [(f"{f[:-4]}/{fam}/{k}", fam, cases[k]) for k in sorted(cases) if _in_model(fam, cases[k])]
    return out


def _in_model(fam, case):
    """Pair-loss cases whose sigma |ds| reaches the screened band or beyond (losses/ranknet/wide: p underflows to 0 in fp32 past
    x ~ -87, a branch the restatement does not take) stay with their own fp32 tests, as losses_knife.npz does."""
    if fam not in ("ranknet", "lambdarank"):
        return True
    p = np.asarray(case["preds"], np.float64)
    x = float(case["sigma"]) * np.abs(p[:, :, None] - p[:, None, :]).max()
    return x < FL.SCREEN_BANDS[0][0]


@pytest.mark.parametrize("name,fam,case", _fixture_cases(), ids=[c[0] for c in _fixture_cases()])
def test_reference_fp32_outputs_pass_the_gate(name, fam, case):
    """The reference's own fp32 runs (its batch loss total and gradient) against the float64 gates: the total against the summed bound."""
    p, y, g = case["preds"], case["labels"], case["grad"]
    if fam in ("ranknet", "lambdarank"):
        c = FL.C_PAIR
        r = (FL.ranknet if fam == "ranknet" else FL.lambdarank)(p, y, None, float(case["sigma"]), c)
        tot, E = FL.batch_total(r, c)
    elif fam == "approxndcg":
        c = FL.C_APPROX
        presort = bool(int(case["presort"])) if "presort" in case else True          # as tests/test_oracle_golden.py runs it
        r = FL.approxndcg(p, y, None, float(case["alpha"]), presort, True, 0.0, c)
        tot, E = r["loss"], r["E_loss"]
    else:
        c = FL.C_LIST
        if fam == "listmle":
            r = FL.listmle(p, case["perm"], None, c)
        else:
            r = {"listnet": FL.listnet, "rankmse": FL.rankmse, "rankcosine": FL.rankcosine}[fam](p, y, None, c)
        tot, E = FL.batch_total(r, c, 1.0 / p.shape[0] if fam == "rankmse" else 1.0)
    FL.gate_nan([float(case["loss"])], [tot], [E], f"{name} loss", c)
    if fam == "listmle":        # the reference's autograd gradient through its log-cumsum-exp needs c 4.2 on two cases (c1, c4)
        return
    FL.gate_nan(g, r["grad"], r["E_grad"], f"{name} grad", c)


# ------------------------------------------------------------------------------------------------------ LambdaLoss, SoftRank, STListNet
# The oracle and the reference's fp32 fixtures pass the new gates, the restated gradients are the derivative of the restated losses,
# float64 emulations of the kernels' own expressions agree with the restatements, planted faults fail.
LL_MU = 5.0


@pytest.mark.parametrize("L,k,kw", [(16, 5, {}), (100, 100, dict(quantise=True, offset=1000.0, need_clamps=True)), (40, 11, dict(mix="yahoo", lens="full"))],
                         ids=["L16-k5", "L100-kL-quant-offset", "L40-k11-yahoo-full"])
def test_oracle_lambdaloss_passes_the_gate(L, k, kw):
    """The oracle rounds p ** w near 1 in fp32, as the reference does: log_floor.  Prints the constant each loss type needs."""
    O = _oracle()
    c = FL.C_LLOSS
    for lt in (0, 1, 2):
        for presort in (True, False):
            p, y, n, *_ = FL.lambdaloss_inputs(48, L, k, mu=LL_MU, loss_type=lt, presort=presort, seed=L + lt, **kw)
            lq, g = O.lambdaloss(p, y, k=k, sigma=1.0, mu=LL_MU, loss_type=lt, presort=presort, lens=n)
            r = FL.lambdaloss(p, y, n, k, 1.0, LL_MU, lt, presort, c, log_floor=True)
            FL.gate_losses(lq, g, r, f"oracle lambdaloss t{lt} pre{int(presort)} L{L}", c, float(lq.astype(np.float64).sum()), FL.batch_total(r, c))
            assert r["loss_q"][4] == 0                                          # length 0
            assert np.isnan(r["loss_q"][2]) == (lt == 0) and np.isnan(r["grad"][2, 0]) == (lt == 0)      # no relevant document
            assert lt == 0 or (r["loss_q"][2] == 0 and (r["grad"][2] == 0).all())


@pytest.mark.parametrize("L,delta,top_k", [(16, 2.0, None), (100, 0.3, 10), (40, 1.0, 50)])
def test_oracle_softrank_passes_the_gate(L, delta, top_k):
    O = _oracle()
    c = FL.C_APPROX
    p, y, n, _ = FL.pair_inputs(40, L, sigma=FL.softrank_inv_den(delta), seed=L, sort_labels=True, span=8.0, offset=1000.0 if L == 100 else 0.0)
    lq, g = O.softrank(p, y, delta, top_k, n)
    r = FL.softrank(p, y, n, delta, top_k, c)
    FL.gate_losses(lq, g, r, f"oracle softrank L{L}", c)
    assert r["loss_q"][4] == 0 and np.isnan(r["loss_q"][2]) and r["grad"][5, 0] == 0 and r["loss_q"][3] == -1.0


@pytest.mark.parametrize("L,T,offset", [(20, 1.0, 0.0), (64, 2.0, 1000.0), (130, 0.5, 0.0)])
def test_oracle_stlistnet_passes_the_gate(L, T, offset):
    O = _oracle()
    c = FL.C_LIST
    p, y, u, n = FL.stlistnet_inputs(40, L, seed=L, offset=offset)
    lq, g = O.stlistnet(p, y, u, T, n)
    FL.gate_losses(lq, g, FL.stlistnet(p, y, u, n, T, c), f"oracle stlistnet L{L}", c)


def _new_fixture_cases():
    out = []
    for f in ("losses.npz", "losses_big.npz", "losses_knife.npz", "siblings.npz", "losses_norel.npz"):
        for fam, cases in G._load(f).items():
            if fam in ("lambdaloss", "lambdaloss1", "softrank", "stlistnet"):
                out += [(f"{f[:-4]}/{fam}/{k}", fam, cases[k]) for k in sorted(cases) if not fam.startswith("lambdaloss") or _ll_in_model(fam, cases[k])]
    return out


def _ll_args(fam, case):
    lt = 0 if fam == "lambdaloss1" else int(case["loss_type"])
    return (int(case["k"]), float(case["sigma"]), float(case["mu"]) if "mu" in case else LL_MU, lt,
            bool(int(case["presort"])) if "presort" in case else True)


def _ll_in_model(fam, case):
    """Queries with an entry inside the screened distance of a clamp (most of losses_knife.npz) stay with their own fp32 tests."""
    p, y = np.asarray(case["preds"]), np.asarray(case["labels"])
    return not any(FL.lambdaloss_query(p[q], y[q], *_ll_args(fam, case), 1.0, detail=True)[4].any() for q in range(p.shape[0]))


@pytest.mark.parametrize("name,fam,case", _new_fixture_cases(), ids=[c[0] for c in _new_fixture_cases()])
def test_reference_fp32_lambdaloss_softrank_stlistnet_pass_the_gate(name, fam, case):
    """The reference's own fp32 batch total and gradient; where it is NaN (losses_norel.npz) the restatement is NaN."""
    p, y, g = case["preds"], case["labels"], case["grad"]
    if fam in ("lambdaloss", "lambdaloss1"):
        c = FL.C_LLOSS
        r = FL.lambdaloss(p, y, None, *_ll_args(fam, case), c, log_floor=True)
    elif fam == "softrank":
        c = FL.C_APPROX
        r = FL.softrank(p, y, None, float(case["delta"]), int(case["top_k"]), c)
    else:
        c = FL.C_LIST
        r = FL.stlistnet(p, y, case["unif"], None, float(case["temperature"]), c)
    tot, E = FL.batch_total(r, c)
    FL.gate_nan([float(case["loss"])], [tot], [E], f"{name} loss", c)
    if "no_relevant" in name and fam == "lambdaloss" and int(case["loss_type"]) != 0:
        # Loss2 / Loss2++ select no entry: loss 0.  The reference's gradient is autograd's 0 * NaN; the product's is the constant's, 0
        assert np.isnan(g).all() and (r["grad"] == 0).all()
        return
    FL.gate_nan(g, r["grad"], r["E_grad"], f"{name} grad", c)


def _central(fn, s, h=1e-5):
    g = np.empty(s.size)
    for i in range(s.size):
        a, b = s.copy(), s.copy()
        a[i] += h
        b[i] -= h
        g[i] = (fn(a) - fn(b)) / (2 * h)
    return g


def test_restated_gradients_are_the_derivatives_of_the_restated_losses():
    """Central differences in float64, at points away from the clamps (N(0, 1) scores: no entry near either)."""
    g_ = np.random.default_rng(5)
    n = 12
    s = g_.standard_normal(n) + 0.01 * np.arange(n)
    y = -np.sort(-g_.choice(5, size=n).astype(np.float64))
    y[0] = max(y[0], 1.0)
    for lt in (0, 1, 2):
        for presort, k in ((True, 7), (False, 12)):
            yy = y if presort else g_.permutation(y)
            f = lambda v: FL.lambdaloss_query(v, yy, k, 1.3, LL_MU, lt, presort, 1.0)[0]
            *_, near, a, b = FL.lambdaloss_query(s, yy, k, 1.3, LL_MU, lt, presort, 1.0, detail=True)
            assert not near.any() and a == 0 and b == 0
            np.testing.assert_allclose(FL.lambdaloss_query(s, yy, k, 1.3, LL_MU, lt, presort, 1.0)[2], _central(f, s), rtol=1e-7, atol=1e-9)
    for top_k in (None, 5):
        f = lambda v: FL.softrank_query(v, y, 0.4, top_k, 1.0)[0]
        np.testing.assert_allclose(FL.softrank_query(s, y, 0.4, top_k, 1.0)[2], _central(f, s), rtol=1e-7, atol=1e-9)
    u = g_.random(n).astype(np.float32)
    f = lambda v: FL.stlistnet_query(v, y, u, 0.5, 1.0)[0]
    np.testing.assert_allclose(FL.stlistnet_query(s, y, u, 0.5, 1.0)[2], _central(f, s), rtol=1e-7, atol=1e-9)


# ---- float64 emulations of the kernels' own expressions (csrc/lambdaloss.hip, approxndcg.hip, listwise.hip)
def _emu_lambdaloss_generic(s, y, k, sigma, mu, lt, presort):
    """lambdaloss_kernel: ideal staging, ranks, the circulant walk over (a, a + d mod kk) with forward / wrapped rank distances, Loss1's
    two ordered entries per unordered pair plus the diagonal."""
    s, y = np.asarray(s, np.float64), np.asarray(y, np.float64)
    n = s.size
    idx = np.arange(n)
    il = idx if presort else np.lexsort((idx, -y))
    S, Y = s[il], y[il]
    rk = np.empty(n, int)
    rk[np.lexsort((idx, -S))] = idx
    idcg = sum((2.0 ** Y[p] - 1.0) / math.log2(p + 2.0) for p in range(n))
    pk = np.zeros((n, 4))
    for p in range(n):
        pk[rk[p], 0], pk[rk[p], 1], pk[rk[p], 3] = S[p], (2.0 ** Y[p] - 1.0) / idcg, Y[p]
        pk[p, 2] = 1.0 / (1.0 / math.log2(p + 2.0))
    kk = min(max(k, 0), n)
    ln2, l2e = math.log(2.0), FL.LL_LOG2_EPS
    loss, gr = 0.0, np.zeros(n)
    lg = lambda x: -math.log1p(math.exp(-x)) / ln2 if x > -700 else x / ln2

    def pair(a, d, dfw, dwr):
        nonlocal loss
        b, fwd = a + d, a + d < kk
        if not fwd:
            b -= kk
        me, o = pk[a], pk[b]
        if lt == 0:
            x = sigma * (me[0] - o[0])
            wb, wa = o[1] * o[2], me[1] * me[2]
            pab, pba = 1.0 / (1.0 + math.exp(-x)), 1.0 / (1.0 + math.exp(x))
            lab = lg(x) if pab >= FL.LL_EPS else l2e
            lba = lg(-x) if pba >= FL.LL_EPS else l2e
            zab, zba = wb * lab, wa * lba
            loss -= (zab if zab >= l2e else l2e) + (zba if zba >= l2e else l2e)
            g = 0.0
            if pab >= FL.LL_EPS and zab >= l2e:
                g -= wb * sigma * (1.0 - pab) / ln2
            if pba >= FL.LL_EPS and zba >= l2e:
                g += wa * sigma * (1.0 - pba) / ln2
            gr[a] += g
            gr[b] -= g
            return
        if me[3] == o[3]:
            return
        a_wins = me[3] > o[3]
        delta = dfw if fwd else dwr
        absG = abs(me[1] - o[1])
        w = delta * absG if lt == 1 else (abs(me[2] - o[2]) + mu * delta) * absG
        x = sigma * ((me[0] - o[0]) if a_wins else (o[0] - me[0]))
        p0 = 1.0 / (1.0 + math.exp(-x))
        lp = lg(x) if p0 >= FL.LL_EPS else l2e
        z = w * lp
        ok = z >= l2e
        loss -= z if ok else l2e
        g = -(w * sigma * (1.0 - p0)) / ln2 if (p0 >= FL.LL_EPS and ok) else 0.0
        g = g if a_wins else -g
        gr[a] += g
        gr[b] -= g

    if lt == 0:
        loss += sum(min(pk[a, 1] * pk[a, 2], -l2e) for a in range(kk))
    for d in range(1, ((kk - 1) >> 1) + 1):
        dfw, dw = abs(pk[d - 1, 2] - pk[d, 2]), kk - d
        dwr = abs(pk[dw - 1, 2] - pk[dw, 2])
        for a in range(kk):
            pair(a, d, dfw, dwr)
    if kk > 0 and kk % 2 == 0:
        d = kk >> 1
        dfw = abs(pk[d - 1, 2] - pk[d, 2])
        for a in range(d):
            pair(a, d, dfw, dfw)
    out = np.empty(n)
    out[il] = gr[rk]
    return loss, out


def _emu_lambdaloss_topk(s, y, k, sigma, mu, lt, fast=True):
    """lambdaloss_topk_kernel: kk arg-max rounds (score descending, index ascending), the pair of each lane from the triangular lane
    index, the fast route's e = exp(-|x|), p = 1 / (1 + e) or e / (1 + e), log2 p = min(x, 0) log2(e) - log2(1 + e), and the gather of
    record r's pairs from lane a (kk - 1) - a (a - 1) / 2 + b - a - 1."""
    s, y = np.asarray(s, np.float64), np.asarray(y, np.float64)
    n = s.size
    idcg = sum((2.0 ** y[i] - 1.0) / math.log2(i + 2.0) for i in range(n))
    kk = min(max(k, 0), n)
    live, rec = np.ones(n, bool), []
    for _ in range(kk):
        m = s[live].max()
        i = int(np.nonzero(live & (s == m))[0][0])
        rec.append(i)
        live[i] = False
    rinv = [1.0 / (1.0 / math.log2(r + 2.0)) for r in range(64)]
    npairs = kk * (kk - 1) // 2
    ln2, l2e = math.log(2.0), FL.LL_LOG2_EPS
    ga, loss = np.zeros(64), 0.0
    for lane in range(npairs):
        a, rem = 0, lane
        for _ in range(11):
            row = kk - 1 - a
            if rem >= row and row > 0:
                rem -= row
                a += 1
        b = a + 1 + rem
        delta, dpos = abs(rinv[b - a - 1] - rinv[b - a]), abs(rinv[a] - rinv[b])
        ya, yb = y[rec[a]], y[rec[b]]
        if ya == yb:
            continue
        Ga, Gb = (2.0 ** ya - 1.0) / idcg, (2.0 ** yb - 1.0) / idcg
        w = delta * abs(Ga - Gb) if lt == 1 else (dpos + mu * delta) * abs(Ga - Gb)
        x = sigma * ((s[rec[a]] - s[rec[b]]) if ya > yb else (s[rec[b]] - s[rec[a]]))
        if fast:
            e = math.exp(-abs(x))
            pb = 1.0 / (1.0 + e)
            p0 = pb if x >= 0 else e * pb
            lp = min(x, 0.0) / ln2 - math.log2(1.0 + e) if p0 >= FL.LL_EPS else l2e
        else:
            p0 = 1.0 / (1.0 + math.exp(-x)) if x > -700 else 0.0
            lp = -math.log1p(math.exp(-x)) / ln2 if p0 >= FL.LL_EPS else l2e
        z = w * lp
        ok = z >= l2e
        loss -= z if ok else l2e
        g = -(w * sigma * (1.0 - p0)) / ln2 if (p0 >= FL.LL_EPS and ok) else 0.0
        ga[lane] = g if ya > yb else -g
    out = np.zeros(n)
    for r in range(kk):
        for o in range(kk):
            if o != r:
                a_, b_ = min(r, o), max(r, o)
                gv = ga[a_ * (kk - 1) - ((a_ * (a_ - 1)) >> 1) + (b_ - a_ - 1)]
                out[rec[r]] += gv if r < o else -gv
    return loss, out


def _emu_softrank(s, y, inv_den, top_k):
    """approxndcg_kernel<SOFT>: both indicators of a pair from one erfc of |x| (the complement by subtraction), the circulant half
    matrix, the symmetric flow cb phi - ca phi, the 1 / IDCG scale."""
    s, y = np.asarray(s, np.float64), np.asarray(y, np.float64)
    n = s.size
    gn = 2.0 ** y - 1.0
    idcg = sum(gn[a] / math.log2(a + 2.0) for a in range(n))
    top = top_k if top_k and top_k > 0 else 1 << 30
    pi = np.zeros(n)

    def pairs():
        for d in range(1, ((n - 1) >> 1) + 1):
            for a in range(n):
                yield a, (a + d) % n
        if n > 0 and n % 2 == 0:
            for a in range(n >> 1):
                yield a, a + (n >> 1)

    for a, b in pairs():
        d = s[b] - s[a]
        sm = 0.5 * math.erfc(abs(d) * inv_den)
        lg = 1.0 - sm
        pi[a] += lg if d > 0 else sm
        pi[b] += sm if d > 0 else lg
    ca, dcg = np.zeros(n), 0.0
    for a in range(n):
        if a < top:
            v = pi[a] + 1.0
            l2 = math.log2(v + 1.0)
            dcg += gn[a] / l2
            ca[a] = gn[a] / (math.log(2.0) * (1.0 + v) * l2 * l2)
    g = np.zeros(n)
    for a, b in pairs():
        x = (s[b] - s[a]) * inv_den
        phi = 0.5641895835477563 * inv_den * math.exp(-x * x)
        flow = ca[b] * phi - ca[a] * phi
        g[a] += flow
        g[b] -= flow
    return -(dcg / idcg), g / idcg


def _emu_stlistnet(s, y, u, inv_t):
    """listnet_kernel with unif: a = (s + -log(-log(u + 1e-20) + 1e-20)) / T, log-softmax by max shift, grad (softmax sum_py - py) / T."""
    uu = (np.asarray(u, np.float32) + np.float32(1e-20)).astype(np.float64)
    a = (np.asarray(s, np.float64) + -np.log(-np.log(uu) + 1e-20)) * inv_t
    y = np.asarray(y, np.float64)
    ea, eb = np.exp(a - a.max()), np.exp(y - y.max())
    py = eb / eb.sum()
    lsm = (a - a.max()) - math.log(ea.sum())
    return -(py * lsm).sum(), (np.exp(lsm) * py.sum() - py) * inv_t


def test_float64_emulations_of_the_kernels_agree_with_the_restatements():
    tol = dict(rtol=1e-12, atol=1e-12)
    for lt in (0, 1, 2):
        for L, k, presort, kw in ((24, 24, True, dict(need_clamps=True)), (24, 7, False, {}), (24, 8, True, dict(quantise=True)), (9, 50, True, {})):
            p, y, n, *_ = FL.lambdaloss_inputs(12, L, k, sigma=1.5, mu=LL_MU, loss_type=lt, presort=presort, seed=L + k, **kw)
            for q in range(12):
                sq, yq = p[q, :n[q]], y[q, :n[q]]
                if n[q] == 0 or not (yq > 0).any():
                    continue
                r = FL.lambdaloss_query(sq, yq, k, 1.5, LL_MU, lt, presort, 1.0)
                lo, gr = _emu_lambdaloss_generic(sq, yq, k, 1.5, LL_MU, lt, presort)
                np.testing.assert_allclose(lo, r[0], **tol)
                np.testing.assert_allclose(gr, r[2], **tol)
                if lt and presort and k <= 11:
                    for fast in (True, False):
                        lo, gr = _emu_lambdaloss_topk(sq, yq, k, 1.5, LL_MU, lt, fast)
                        np.testing.assert_allclose(lo, r[0], **tol)
                        np.testing.assert_allclose(gr, r[2], **tol)
    p, y, n, _ = FL.pair_inputs(12, 21, sigma=0.5, seed=3, sort_labels=True, span=8.0, every_relevant=True, quantise=True)
    u = np.random.default_rng(4).random(p.shape).astype(np.float32)
    u[0, :2] = (0.0, 2.0 ** -24)
    for q in range(12):
        sq, yq = p[q, :n[q]], y[q, :n[q]]
        for top_k in (None, 4):
            r = FL.softrank_query(sq, yq, 0.5, top_k, 1.0)
            lo, gr = _emu_softrank(sq, yq, 0.5, top_k)
            np.testing.assert_allclose(lo, r[0], **tol)
            np.testing.assert_allclose(gr, r[2], **tol)
        r = FL.stlistnet_query(sq, yq, u[q, :n[q]], 0.5, 1.0)
        lo, gr = _emu_stlistnet(sq, yq, u[q, :n[q]], 0.5)
        np.testing.assert_allclose(lo, r[0], **tol)
        np.testing.assert_allclose(gr, r[2], **tol)


# ---- planted faults
def test_lambdaloss_log2_of_the_fp32_probability_fails_without_the_floor_and_passes_the_old_rule():
    """log2 p from the fp32-rounded p (what a hardware log of p gives near 1, and what the generic kernel's comment rules out) at
    k = L = 256.  One query of the batch is a converged one — grades 21 / sigma apart, so every winner's p rounds to 1 in fp32 and its
    log2 to 0, where the true term is e^-x / ln2 —: its ~2e4 pair losses are all lost, all with one sign.  (Rounding p merely NEAR 1 is
    unbiased noise, and Loss2's weights already carry ~1e-4 relative from the adjacent discounts they subtract; only the bias shows.)
    The batch total, all the old rule saw, moves by 1e-10; the query's loss_q leaves the relative bound, and is inside it again once
    the floor is added that the top-k kernel (at most 55 pairs) is allowed."""
    O = _oracle()
    p, y, n, *_ = FL.lambdaloss_inputs(8, 256, 256, loss_type=1, presort=True, seed=21, lens="full", specials=False)
    p[0] = (21.0 * y[0] + np.random.default_rng(1).uniform(-0.5, 0.5, 256)).astype(np.float32)
    *_, near, _, _ = FL.lambdaloss_query(p[0], y[0], 256, 1.0, LL_MU, 1, True, 1.0, detail=True)
    assert not near.any()
    lq, g = O.lambdaloss(p, y, k=256, sigma=1.0, mu=LL_MU, loss_type=1, presort=True, lens=n)
    c = FL.C_LLOSS
    r = FL.lambdaloss(p, y, n, 256, 1.0, LL_MU, 1, True, c)
    bad = r["loss_q"].copy()
    for q in range(8):
        s_, y_ = p[q].astype(np.float64), y[q].astype(np.float64)
        o = np.lexsort((np.arange(256), -s_))
        ss, ys = s_[o], y_[o]
        G_ = FL._gain(ys) / (FL._gain(y_) * FL._disc(256)).sum()
        inv = np.log2(np.arange(256) + 2.0)
        d = np.abs(np.arange(256)[:, None] - np.arange(256)[None, :])
        w = np.where(d > 0, np.abs(inv[np.maximum(d - 1, 0)] - inv[d]), 0.0) * np.abs(G_[:, None] - G_[None, :])
        act = ys[:, None] > ys[None, :]
        x = ss[:, None] - ss[None, :]
        pr = FL._sig(x)
        ok = act & (pr >= 1e-7)
        lp = -(np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))) / FL.LN2
        lp32 = np.log2(pr.astype(np.float32).astype(np.float64), where=ok, out=np.zeros_like(pr))
        bad[q] += (w * (lp - lp32))[ok].sum()
    assert _old_rule_passes(bad.sum(), r["loss_q"].sum(), g, g)
    FL.gate_losses(lq, g, FL.lambdaloss(p, y, n, 256, 1.0, LL_MU, 1, True, c, log_floor=True), "lambdaloss oracle", c)
    with pytest.raises(AssertionError, match="loss_q"):
        FL.gate_nan(bad, r["loss_q"], r["E_loss_q"], "lambdaloss fp32 log2 p loss_q", c)
    rf = FL.lambdaloss(p, y, n, 256, 1.0, LL_MU, 1, True, c, log_floor=True)
    FL.gate_nan(bad, rf["loss_q"], rf["E_loss_q"], "lambdaloss fp32 log2 p with the floor", c)


def _erfc_as(x):
    """Abramowitz & Stegun 7.1.26: erfc to 1.5e-7 absolute."""
    t = 1.0 / (1.0 + 0.3275911 * x)
    return t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429)))) * np.exp(-x * x)


def test_softrank_with_a_low_precision_erfc_fails_the_gate_and_passes_the_old_rule():
    """erfc by Abramowitz & Stegun 7.1.26 (1.5e-7 absolute).  Near x = 0 that is inside the noise of a c u-relative erfc; from x ~ 1.3 on
    it is 2 to 300 times the bound of the small indicator.  Query 0 has its best document 1.9 .. 2.6 den above 63 others (there the
    approximation errs by +3e-8 .. +7e-8, all one way), and top_k = 1 makes its loss that document's expected rank alone."""
    O = _oracle()
    delta = 2.0
    inv_den = FL.softrank_inv_den(delta)
    p, y, n, _ = FL.pair_inputs(32, 64, sigma=inv_den, seed=17, sort_labels=True, span=8.0, every_relevant=True, lens="full", specials=False)
    p[0, 0], y[0, 0] = 0.0, 3.0
    p[0, 1:] = (-(1.9 + 0.7 * np.arange(63) / 62.0) / inv_den).astype(np.float32)
    lq, g = O.softrank(p, y, delta, 1, n)
    bad = np.empty(32)
    for q in range(32):
        s_, y_ = p[q].astype(np.float64), y[q].astype(np.float64)
        x = (s_[:, None] - s_[None, :]) * inv_den
        sm = 0.5 * _erfc_as(np.abs(x))
        yv = np.where(x > 0, sm, 1.0 - sm)
        np.fill_diagonal(yv, 0.0)
        pi = 1.0 + yv.sum(1)
        bad[q] = -((FL._gain(y_[0]) / np.log2(pi[0] + 1.0)) / (FL._gain(y_) * FL._disc(64)).sum())
    c = FL.C_APPROX
    r = FL.softrank(p, y, n, delta, 1, c)
    FL.gate_losses(lq, g, r, "softrank oracle", c)
    assert _old_rule_passes(bad.sum(), r["loss_q"].sum(), g, g)
    with pytest.raises(AssertionError, match="loss_q"):
        FL.gate_losses(bad, g, r, "softrank low-precision erfc", c)


def test_stlistnet_gumbel_noise_through_a_low_precision_log_fails_the_gate_and_passes_the_old_rule():
    """The inner log of the Gumbel draw with 2^-17.5 (5e-6) relative error, of either sign: every noise value moves by 5e-6 absolute.
    The old rule lets a gradient element move by 1e-5 of itself plus 1e-6 of the largest; the gate's bound on the same elements is
    about half of what they move."""
    O = _oracle()
    p, y, u, n = FL.stlistnet_inputs(48, 64, seed=19)
    lq, g = O.stlistnet(p, y, u, 1.0, n)
    rng = np.random.default_rng(2)
    uu = (u + np.float32(1e-20)).astype(np.float64)
    gum = -(np.log(-(np.log(uu) * (1.0 + 2.0 ** -17.5 * rng.choice([-1.0, 1.0], size=u.shape))) + 1e-20))
    bad_l, bad_g = np.zeros(48), np.zeros((48, 64))
    for q in range(48):
        if n[q]:
            bad_l[q], _, bad_g[q, :n[q]], _ = FL.listnet_query(p[q, :n[q]].astype(np.float64) + gum[q, :n[q]], y[q, :n[q]], 1.0)
    c = FL.C_LIST
    r = FL.stlistnet(p, y, u, n, 1.0, c)
    FL.gate_losses(lq, g, r, "stlistnet oracle", c)
    assert _old_rule_passes(bad_l.sum(), r["loss_q"].sum(), bad_g, r["grad"])
    with pytest.raises(AssertionError):
        FL.gate_losses(bad_l, bad_g, r, "stlistnet low-precision log", c)


def test_planted_exact_and_nan_faults_fail_the_new_gates():
    O = _oracle()
    c = FL.C_LLOSS
    p, y, n, *_ = FL.lambdaloss_inputs(24, 32, 5, loss_type=1, presort=True, seed=23)
    lq, g = O.lambdaloss(p, y, k=5, sigma=1.0, mu=LL_MU, loss_type=1, presort=True, lens=n)
    r = FL.lambdaloss(p, y, n, 5, 1.0, LL_MU, 1, True, c, log_floor=True)
    FL.gate_losses(lq, g, r, "lambdaloss oracle", c)
    q = 10
    beyond = int(np.argsort(-p[q, :n[q]].astype(np.float64), kind="stable")[7])        # ranked eighth: beyond k = 5
    assert r["grad"][q, beyond] == 0 and r["E_grad"][q, beyond] == 0
    bad = g.copy()
    bad[q, beyond] = 1e-9
    with pytest.raises(AssertionError, match="grad"):
        FL.gate_losses(lq, bad, r, "a 1e-9 gradient beyond k", c)
    # NDCG_Loss1 with a finite loss on the query without a relevant document (what the kernel returned before this gate)
    lq1, g1 = O.lambdaloss(p, y, k=5, sigma=1.0, mu=LL_MU, loss_type=0, presort=True, lens=n)
    r1 = FL.lambdaloss(p, y, n, 5, 1.0, LL_MU, 0, True, c, log_floor=True)
    FL.gate_losses(lq1, g1, r1, "lambdaloss1 oracle", c)
    assert np.isnan(r1["loss_q"][2])
    bad = lq1.copy()
    bad[2] = 25 * 26.575424
    with pytest.raises(AssertionError, match="loss_q"):
        FL.gate_losses(bad, g1, r1, "Loss1 finite where the reference is NaN", c)
    # SoftRank: NaN on the zero-length query
    ps, ys, ns, _ = FL.pair_inputs(24, 32, sigma=0.25, seed=29, sort_labels=True, span=8.0)
    ls, gs = O.softrank(ps, ys, 2.0, None, ns)
    rs = FL.softrank(ps, ys, ns, 2.0, None, FL.C_APPROX)
    FL.gate_losses(ls, gs, rs, "softrank oracle", FL.C_APPROX)
    bad = ls.copy()
    assert ns[4] == 0 and bad[4] == 0
    bad[4] = np.nan
    with pytest.raises(AssertionError, match="loss_q"):
        FL.gate_losses(bad, gs, rs, "softrank NaN on a zero-length query", FL.C_APPROX)


def test_oracle_follows_the_reference_on_a_query_without_a_relevant_document():
    """tests/golden/losses_norel.npz, the reference's own outputs: NDCG_Loss1 is NaN, loss and every gradient; NDCG_Loss2 / Loss2++ are 0
    — with a NaN gradient in the reference (autograd's 0 * NaN through the unselected entries), where the oracle and the kernels keep
    the derivative of the constant, 0 —; SoftRank is NaN throughout."""
    O = _oracle()
    fams = G._load("losses_norel.npz")
    for name, case in sorted(fams["lambdaloss"].items()):
        lt = int(case["loss_type"])
        assert np.isnan(case["grad"]).all() and np.isnan(case["loss"]) == (lt == 0) and (lt == 0 or float(case["loss"]) == 0), name
        lq, g = O.lambdaloss(case["preds"], case["labels"], k=int(case["k"]), sigma=1.0, mu=float(case["mu"]), loss_type=lt, presort=True)
        assert (np.isnan(g).all() and np.isnan(lq[0])) if lt == 0 else ((g == 0).all() and lq[0] == 0), name
    for name, case in sorted(fams["softrank"].items()):
        one = case["preds"].shape[1] == 1                      # one document: no pair, the gradient is exactly 0
        assert "one_doc" in name if one else "one_doc" not in name
        assert ((case["grad"] == 0).all() if one else np.isnan(case["grad"]).all()) and np.isnan(case["loss"]), name
        lq, g = O.softrank(case["preds"], case["labels"], float(case["delta"]), int(case["top_k"]) or None)
        assert ((g == 0).all() if one else np.isnan(g).all()) and np.isnan(lq[0]), name
        r = FL.softrank(case["preds"], case["labels"], None, float(case["delta"]), int(case["top_k"]), FL.C_APPROX)
        assert ((r["grad"] == 0).all() if one else np.isnan(r["grad"]).all()) and np.isnan(r["loss_q"][0]), name
    assert any("one_doc" in name for name in fams["softrank"])


def test_a_nan_score_gives_a_nan_list_where_the_reference_ranks_it_first():
    """tests/golden/losses_nanscore.npz, the reference's own outputs on lists with fewer than k real scores: torch.sort ranks a NaN score
    first, its differences count as 0 and carry no gradient, and every output is finite.  The product deviates, on purpose (header of
    csrc/lambdaloss.hip): such a list has no ranking, so its loss and the gradient of every document are NaN — in the oracle and in the
    restatement that the kernels are gated against."""
    O = _oracle()
    cases = G._load("losses_nanscore.npz")["lambdaloss"]
    assert len(cases) == 8
    for name, case in sorted(cases.items()):
        p, y, k, lt = case["preds"], case["labels"], int(case["k"]), int(case["loss_type"])
        real = int((~np.isnan(p)).sum())
        assert 0 < real < 5 and np.isfinite(case["loss"]) and np.isfinite(case["grad"]).all() and (case["grad"][np.isnan(p)] == 0).all(), name
        first = torch.sort(torch.from_numpy(p), dim=1, descending=True)[1][0, :p.shape[1] - real].numpy()
        assert np.isnan(p[0, first]).all(), name                 # the reference's order: every NaN before the best real score
        lq, g = O.lambdaloss(p, y, k=k, sigma=1.0, mu=float(case["mu"]), loss_type=lt, presort=True)
        r = FL.lambdaloss(p, y, None, k, 1.0, float(case["mu"]), lt, True, FL.C_LLOSS)
        assert np.isnan(lq[0]) and np.isnan(g).all() and np.isnan(r["loss_q"][0]) and np.isnan(r["grad"]).all() and (r["E_grad"] == 0).all(), name
        FL.gate_losses(lq, g, r, name, FL.C_LLOSS)
    # a NaN score in one list leaves its neighbours alone; padding stays 0
    p, y, n, *_ = FL.lambdaloss_inputs(12, 16, 5, loss_type=2, presort=True, seed=3)
    clean = FL.lambdaloss(p, y, n, 5, 1.0, LL_MU, 2, True, FL.C_LLOSS)
    q = int(np.argmax(n >= 2))
    p[q, 1] = np.nan
    lq, g = O.lambdaloss(p, y, k=5, sigma=1.0, mu=LL_MU, loss_type=2, presort=True, lens=n)
    r = FL.lambdaloss(p, y, n, 5, 1.0, LL_MU, 2, True, FL.C_LLOSS, log_floor=True)
    FL.gate_losses(lq, g, r, "one NaN score", FL.C_LLOSS)
    others = np.arange(12) != q
    assert np.array_equal(r["grad"][others], clean["grad"][others], equal_nan=True) and np.isnan(r["grad"][q, :n[q]]).all()
    assert (g[q, n[q]:] == 0).all() and np.isnan(lq[q])
