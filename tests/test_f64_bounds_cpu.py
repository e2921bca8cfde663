"""CPU self-test of tests/f64_bounds.py: fp32 restatements of each dense primitive pass the element-wise float64 gate, and planted faults
— the kind a bf16x6 or a chunked-reduction kernel can make — fail it while the max-norm `close` the dense-layer GPU tests used before
passes them (the gap the element-wise gate closes)."""
import pytest
import torch

import f64_bounds as B


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
