"""Float64 references and ELEMENT-WISE error bounds for the dense-layer kernels (Linear GEMMs, the fused pointsf scorer, batch norm +
activation), and the structured data that makes those bounds bite.

Why: a max-norm gate `|got - ref|.max() <= tol * max(1, |ref|.max())` only sees the largest column.  On LETOR-like data — feature
scales over many orders of magnitude, sparse and constant features, padded (zero-gradient) rows — a wrong SMALL column of an output,
of dW or of a batch-norm gradient passes it (tests/test_f64_bounds_cpu.py plants such faults and shows it).  Here each element gets
its own bound.

The gate is  |got - ref| <= E  element by element, with ref computed in float64 from the very fp32 inputs the kernel saw, and

    E = c * u * (float64 sum of |terms| that form the element) [+ what earlier layers carried in],       u = 2^-24

which is the standard first-order bound of a k-ordered fp32 dot product (each rounding is at most u times the partial sum, and every
partial sum is at most the sum of |terms|).  `c` is one constant per kernel family, set from GPU measurement (see the constants below).

GEMM (`gemm_fwd`, `gemm_bwd_input`, `gemm_bwd_weight`):
    Y  = X W^T + b            E_Y  = c u (|X| |W|^T + |b|)
    dX = (dY W) * g / (1-p)   E_dX = (c u |dY| |W|) * g / (1-p) + u |dX|         (g = [gate > 0]; the scale is one more rounding)
    dW = dY^T X,  db = sum dY E_dW = c u |dY|^T |X|,  E_db = c u sum |dY|
Layer chains (`relu_mlp`), first order: an input error E_in reaches the output through |W|:
    forward   E_l = c u (|W_l| |H_{l-1}| + |b_l|) + |W_l| E_{l-1}  (E_{l-1} of H = relu(Z) * mask / (1-p): the Z bound times the mask scale)
    backward  E_dH = c u |dZ| |W| + E_dZ |W|,     E_dZ = E_dH * gate
              E_dW = c u |dZ|^T |H| + E_dZ^T |H| + |dZ|^T E_H
ReLU at a kink: where |z| <= E_z the sign of the kernel's z cannot be decided.  The forward gate accepts either branch there (h = 0, or
h within E of z); `relu_mlp` reports the rows holding such a unit, the tests give those rows zero output gradient (so a flipped gate
cannot move a gradient: the row's dZ is exactly 0 either way) and assert that such units are rare (`MAX_AMBIGUOUS`).

Batch norm + activation (the arithmetic of csrc/bnact.hip):
  statistics (`bn_stats`): per chunk b of rows (pivot k_b = the chunk's first row, as colsum2_kernel<0> uses) the kernel sums
    d = z - k_b and d^2, then combines chunk means and M2 by the parallel-variance formula.  Every rounding is relative to one of
    |mu| (the chunk mean k_b + m_b and the weighted mean of the chunk means), |z - k_b| or (z - k_b)^2, and |mean_b - mu| (mu + ..):
        E_mu  = c u (|mu| + A),   A  = mean |z - k|
        E_var = c u (S2 + D (|mu| + A)),   S2 = mean (z - k)^2,  D = mean over rows of |mean_b - mu|
        E_rstd = rstd (E_var / (2 (var + eps)) + c u)
  forward (`bnact_fwd`), given the kernel's own mean / rstd (they are its inputs, exact in float64):
        xh = (z - mu) rstd, y = gamma xh + beta:   E_xh = c u |xh|,  E_y = |gamma| E_xh + c u |y|
        a  = f(y) keep / (1-p):   E_a = (|f'(y)| E_y + E_f(y)) keep / (1-p) + u |a|
    E_f: the evaluation error of the activation, c u |f| plus, for GELU, 0.5 |y| * 6.8e-8 — erf_fast's stated maximum absolute
    error (csrc/bnact.hip) — and the rounding of 0.5 y (1 + erf): c u 0.5 |y| (1 + |erf|).
  backward (`bnact_bwd`):  dy = da keep/(1-p) f'(y),  sdy = sum dy,  sdyx = sum dy xh  (over the real rows of the group)
        dz = gamma rstd (dy - sdy/n - xh sdyx/n),  dgamma = sdyx,  dbeta = sdy
        E_dy   = |da| keep/(1-p) (|f''(y)| E_y + E_f'(y)) + c u |dy|
        E_sdy  = c u sum|dy| + sum E_dy,     E_sdyx = c u sum|dy xh| + sum (E_dy |xh| + |dy| E_xh)
        E_dz   = |gamma| rstd (E_dy + E_sdy/n + E_xh |sdyx|/n + |xh| E_sdyx/n) + c u |gamma| rstd (|dy| + |sdy|/n + |xh| |sdyx|/n)
    (E_f' likewise: erf_fast's 0.5 * 6.8e-8 in GELU', and y pdf(y) (1 + y^2) u for the exp2 of -y^2/2 on a rounded argument.)
  The mean offset |mu| enters the statistics bound only: given mu, (z - mu) is one rounding of |z - mu|.  A kernel that computes
  z * rstd - mu * rstd instead rounds |z| rstd and |mu| rstd — far above E_xh on a column whose mean is many standard deviations.

Multi-head attention core (the arithmetic of csrc/listsf.hip), per (query, head), s = 1/sqrt(dh), keys >= lens excluded (P = 0 there,
so the dK / dV rows of padded keys are exactly 0: E = 0 demands equality), keep' = keep / (1 - p) from the kernel's exported mask:
  forward (`mhsa_fwd`):
        S = s q.k                   E_S = c u s |q|.|k|
        P = exp(S - m) / l          E_P = P (e_j + sum_k P_k e_k),   e_j = E_S_j + c u (1 + |S_j - m|)
    (|S - m| u: the rounding of the exponent's argument, relative to the argument; the online softmax's rescaling factors
    exp(m_old - m_new) of a key add up to at most |S_j - m| more of it; sum_k P_k e_k is the error of the normaliser l)
        O = (P keep') V             E_O = c u |P'| |V| + E_P' |V|
        LSE = m + log l             E_LSE = sum P e + c u (|LSE| + 1)
  backward (`mhsa_bwd`), given the kernel's own O and LSE (inputs of ptr_mhsa_backward: exact in float64, as bnact_fwd takes the
  kernel's mean / rstd — the forward's error stays out of the backward's gate):
        P = exp(S - lse)            E_P = P (E_S + c u (1 + |S - lse|))
        D = sum O dO                E_D = c u sum |O| |dO|
        dP = dO V^T                 E_dP = c u |dO| |V|^T
        dS = P (dP keep' - D) s     E_dS = s (P (E_dP keep' + E_D + c u (|dP keep'| + |D|)) + E_P |dP keep' - D|)
    (the roundings of dP keep' and of the difference are relative to |dP keep'| + |D|, not to |dS|: they matter where dP keep' ~ D)
        dQ = dS K                   E_dQ = c u |dS| |K| + E_dS |K|
        dK = dS^T Q                 E_dK = c u |dS|^T |Q| + E_dS^T |Q|
        dV = P'^T dO                E_dV = c u |P'|^T |dO| + E_P'^T |dO|

LayerNorm (list_ranker.py:152-174; csrc/listsf.hip layernorm_*_kernel): two-pass mean / UNBIASED variance over the F features of a
row, eps added to the standard deviation:
  forward (`layernorm_fwd`):
        mean = sum x / F            E_mean = c u mean |x|
        c_i = x_i - mean            E_c = E_mean + u |c|
        var = sum c^2 / (F - 1)     E_var = (c u sum c^2 + F E_mean^2 + 2 u E_mean sum |c|) / (F - 1)
    (sum_i (c_i + d)^2 = sum c^2 + F d^2: a shared error d of the mean enters the two-pass variance at second order only.  A one-pass
    E[x^2] - mean^2 rounds mean^2, and fails this bound on rows whose mean is a few standard deviations)
        sd = sqrt(var)              E_sd = min(E_var / (2 sd), sqrt(E_var)) + c u sd        (sqrt(E_var): the bound at sd = 0)
        rinv = 1 / (sd + eps)       E_rinv = rinv^2 (E_sd + c u (sd + eps)) + c u rinv
        y = a c rinv + b            E_y = |a| (E_c rinv + |c| E_rinv) + c u (|a c rinv| + |y|)
    A near-constant row (sd ~ u |mean|) gets a bound of the order of |a| c u |mean| / (sd + eps): the kernel's own c_i there are all
    rounding, and so is y.  (sqrt and the reciprocal count c u, not u: the device's are 1-ulp approximations.)
  backward (`layernorm_bwd`), given the kernel's stats {mean, rinv, sd}; g = dy a, c = x - mean:
        dx = rinv (g - mean g) - c k2,   k2 = rinv^2 sum(g c) / (sd (F - 1)),   k2 = 0 on a row with sd = 0 (the kernel's rule: the
    derivative of 1/(std + eps) is undefined there; autograd gives NaN)
        E_dx = rinv c u sum|g| / F + |c| rinv^2 c u sum|g c| / (sd (F - 1)) + c u (rinv (|g| + |mean g|) + |c k2|)
        da = sum_rows dy c rinv     E_da = c u sum |dy c rinv|;      db = sum_rows dy    E_db = c u sum |dy|
"""
import math

import numpy as np
import torch

U = 2.0 ** -24

# ---- one constant per kernel family (c above), set from GPU measurement on an MI355X: each gated test prints `MEASURED <what>: worst err/E
# (c C: needs c >= k)`; k is the constant that data needs.  Worst k over tests/test_dense_bounds_gpu.py:
C_FP32 = 32.0     # fp32-MFMA GEMMs (linear.hip, scorer.hip / scorer_bwd.hip): worst 20.7 (linear forward 2049 x 136 -> 408, structured data); 1.5x
                  # headroom.  Above the guide's 1.3-2.5 for random data because a dominant column (2^10 scale, mean 1000x its spread) makes
                  # every k-ordered partial sum as large as the whole |terms| sum: ~sqrt(K) roundings of that size (fp32 torch on the CPU: 15).
C_X6 = 32.0       # bf16x6 GEMMs (linear_x6.hip, linear_bw_x6.hip, scorer_x6.hip, scorer_bwd_x6.hip, scorer_dw_x6.hip): worst 16.3 (same shape); 2x.
                  # Scorer chains, either forward: worst 4.4.  A dropped bf16 plane product of the linear forward needs 69.
C_BNACT = 16.0    # batch-norm statistics / bnact forward / backward (bnact.hip): worst 10.5 (rstd of per-query groups of 128 rows: the one-pass
                  # M2 = sum d^2 - sum d * mean_d cancels against the pivot's offset); everything else <= 2.3; 1.5x headroom
C_ATTN = 8.0      # attention core forward / backward (listsf.hip mhsa_*_kernel, tests/test_listsf_bounds_gpu.py): worst 4.94 (dK, 3 x 128 keys,
                  # dh 17, stored dS); dV at 513 and 1031 keys 4.4; O and LSE <= 3.3; 1.6x headroom.  fp32 torch on the CPU: 3.4
C_LN = 6.0        # LayerNorm forward / backward (listsf.hip layernorm_*_kernel): worst 3.35 (row mean, 32773 x 700); y, dx 3.2 up to
                  # 262144 x 136; 1.8x headroom.  fp32 torch on the CPU: 3.2

MAX_AMBIGUOUS = 0.01     # at most this fraction of ReLU units (elements) may lie within their bound of the kink (else the bound says little)
ERF_FAST_ABS = 6.8e-8    # erf_fast's stated maximum absolute error (csrc/bnact.hip)
FLT_MIN = 2.0 ** -126    # an fp32 activation (or derivative) below the normal range may flush to 0: its absolute error floor

AF_NONE, AF_RELU, AF_LEAKY, AF_ELU, AF_SELU, AF_GELU, AF_SIGMOID, AF_TANH = range(8)     # PTR_AF_* (include/ptranking_amd.h)
AF_NAMES = {AF_NONE: "none", AF_RELU: "relu", AF_LEAKY: "leaky", AF_ELU: "elu", AF_SELU: "selu", AF_GELU: "gelu", AF_SIGMOID: "sigmoid",
            AF_TANH: "tanh"}


def d64(t):
    """float64 CPU copy (numpy arrays and tensors alike)."""
    if isinstance(t, np.ndarray):
        return torch.from_numpy(t).double()
    return t.detach().double().cpu()


# ---------------------------------------------------------------------------------------------------------------------------- the gate
def gate(got, ref, E, what, c=None, accept=None):
    """|got - ref| <= E element-wise (E == 0: exact equality).  accept: boolean mask of elements an alternative rule already accepted
    (a ReLU kink taken the other way).  Prints the worst err/E as a MEASURED line (times c: the constant this data would need), raises
    with the first failing index, got, ref, E and the number of failing elements.  Returns the worst err/E."""
    __tracebackhide__ = True
    got, ref = d64(got), d64(ref)
    E = d64(E).expand_as(ref) if torch.is_tensor(E) else torch.full_like(ref, float(E))
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs()
    ok = err <= E
    ok &= torch.isfinite(got)
    if accept is not None:
        ok |= accept.to(torch.bool) & torch.isfinite(got)
    judged = (E > 0) if accept is None else ((E > 0) & ~accept.to(torch.bool))
    worst = float((err[judged] / E[judged]).max()) if bool(judged.any()) else 0.0
    print(f"MEASURED {what}: worst err/E {worst:.3f}" + (f" (c {c:g}: needs c >= {worst * c:.2f})" if c else "") + f" over {ref.numel()} elements")
    if not bool(ok.all()):
        bad = ~ok
        i = int(torch.nonzero(bad.reshape(-1))[0])
        idx = np.unravel_index(i, tuple(ref.shape)) if ref.dim() else ()
        raise AssertionError(f"{what}: element-wise f64 bound failed at {tuple(int(j) for j in idx)}: got {float(got.reshape(-1)[i])!r} "
                             f"ref {float(ref.reshape(-1)[i])!r} |diff| {float(err.reshape(-1)[i]):.3e} > E {float(E.reshape(-1)[i]):.3e}; "
                             f"{int(bad.sum())} of {ref.numel()} elements fail (worst err/E {worst:.2f})")
    return worst


def maxnorm_close(got, ref, tol):
    """The max-norm rule the dense-layer tests used before (tests/test_linear_gpu.py `close`): True when it would pass."""
    got, ref = d64(got), d64(ref)
    return float((got - ref).abs().max()) <= tol * max(1.0, float(ref.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------- data
def structured_inputs(R, K, seed=0, scale_exp=(-10, 10), sparse_frac=0.2):
    """fp32 [R, K] features shaped like LETOR data: log-uniform column scales 2^-10..2^10, ~20 % sparse columns (90 % zeros), one
    all-zero column, one constant column (a value whose multiples are exact in fp32), duplicated rows and two columns whose mean is
    ~1000x their spread.  Returns (X, info) with info = {'zero_col', 'const_col', 'offset_cols'}."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(scale_exp[0], scale_exp[1] + 1, (K,), generator=g).double()
    X = torch.randn(R, K, generator=g, dtype=torch.float64) * torch.pow(2.0, e)
    perm = torch.randperm(K, generator=g)
    nsp = max(1, int(sparse_frac * K))
    for j in perm[:nsp].tolist():
        X[torch.rand(R, generator=g) < 0.9, j] = 0.0
    zero_col, const_col = int(perm[nsp % K]), int(perm[(nsp + 1) % K])
    offset_cols = [int(perm[(nsp + 2 + i) % K]) for i in range(2)] if K >= nsp + 4 else []
    X[:, zero_col] = 0.0
    X[:, const_col] = 1.5 * 2.0 ** float(e[const_col])
    for j in offset_cols:
        X[:, j] = 2.0 ** float(e[j]) * (1000.0 + torch.randn(R, generator=g, dtype=torch.float64))
    if R >= 8:
        nd = R // 8
        X[R - nd:] = X[:nd]                                   # duplicated rows
    return X.float().contiguous(), dict(zero_col=zero_col, const_col=const_col, offset_cols=offset_cols)


def structured_grads(R, N, seed=1, zero_frac=0.1, scale_exp=(-12, 0)):
    """fp32 [R, N] output gradients: rows scaled 2^-12..1, ~10 % zero (padded) rows and a zero block at the end.  Returns (dY, zero_rows)."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(scale_exp[0], scale_exp[1] + 1, (R, 1), generator=g).double()
    dY = torch.randn(R, N, generator=g, dtype=torch.float64) * torch.pow(2.0, e)
    zero = torch.rand(R, generator=g) < zero_frac
    zero[R - max(1, R // 16):] = True if R > 1 else zero[R - 1:]
    dY[zero] = 0.0
    return dY.float().contiguous(), zero


def weights(N, K, seed=2):
    """fp32 [N, K] weights ~ N(0, 1/K) with per-output-row scales 2^-4..2^4 (a small row makes a small output column)."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(-4, 5, (N, 1), generator=g).double()
    return (torch.randn(N, K, generator=g, dtype=torch.float64) * torch.pow(2.0, e) / math.sqrt(K)).float().contiguous()


# ---------------------------------------------------------------------------------------------------------------------------- GEMM
def _mm(a, b, chunk=65536):
    if a.shape[0] <= chunk:
        return a @ b
    return torch.cat([a[i:i + chunk] @ b for i in range(0, a.shape[0], chunk)])


def gemm_fwd(X, W, b, c):
    """Z = X W^T + b and its bound."""
    X, W = d64(X), d64(W)
    Z = _mm(X, W.t())
    S = _mm(X.abs(), W.abs().t())
    if b is not None:
        Z = Z + d64(b)
        S = S + d64(b).abs()
    return Z, c * U * S


def relu_fwd_accept(got, Z, EZ):
    """Elements a ReLU kernel may legitimately have taken either way: |z| <= E_z and got is 0 or within E_z of z."""
    got = d64(got)
    amb = Z.abs() <= EZ
    return amb & ((got == 0) | ((got - Z).abs() <= EZ))


def gemm_bwd_input(dY, W, c, gate=None, p=0.0):
    """dX = (dY W) * [gate > 0] / (1 - p) and its bound."""
    dY, W = d64(dY), d64(W)
    G = _mm(dY, W)
    S = _mm(dY.abs(), W.abs())
    if gate is not None:
        m = (d64(gate) > 0).double() / (1.0 - p)
        G, S = G * m, S * m
    return G, c * U * S + U * G.abs()


def gemm_bwd_weight(X, dY, c):
    """dW = dY^T X, db = sum_rows dY, and their bounds."""
    X, dY = d64(X), d64(dY)
    return dY.t() @ X, c * U * (dY.abs().t() @ X.abs()), dY.sum(0), c * U * dY.abs().sum(0)


# ---------------------------------------------------------------------------------------------------------------------------- ReLU MLP
def relu_mlp(X, Ws, bs, c, masks=None, p=0.0, dout=None, chunk=65536):
    """(Dropout -> Linear -> ReLU) x NL -> Linear (the fused pointsf scorer) in float64 with first-order chain bounds.  masks: keep masks
    [R, width] per dropout site (0 = input) or None.  dout [R]: weights of the output (d loss / d pred); rows holding an ambiguous ReLU
    unit should get 0 there (see the module docstring).  Returns dict(out, E_out, amb_rows, amb_frac (ambiguous hidden units / all), and with dout: dW, E_dW, db, E_db lists)."""
    NL = len(Ws) - 1
    Ws, bs = [d64(w) for w in Ws], [d64(b) for b in bs]
    R = X.shape[0]
    want_bwd = dout is not None
    dW = [torch.zeros_like(w) for w in Ws]; EdW = [torch.zeros_like(w) for w in Ws]
    db = [torch.zeros_like(b) for b in bs]; Edb = [torch.zeros_like(b) for b in bs]
    outs, Eouts, amb_rows = [], [], []
    n_amb = n_units = 0
    for r0 in range(0, R, chunk):
        h = d64(X[r0:r0 + chunk])
        if masks is not None:
            h = h * d64(masks[0][r0:r0 + chunk]) / (1 - p)
        Eh = torch.zeros_like(h)
        hs, Ehs, gates = [h], [Eh], []
        amb = torch.zeros(h.shape[0], dtype=torch.bool)
        for l in range(NL + 1):
            W, b = Ws[l], bs[l]
            z = h @ W.t() + b
            Ez = c * U * (h.abs() @ W.abs().t() + b.abs()) + Eh @ W.abs().t()
            if l == NL:
                outs.append(z[:, 0]); Eouts.append(Ez[:, 0])
                break
            kink = z.abs() <= Ez
            amb |= kink.any(dim=1)
            n_amb += int(kink.sum()); n_units += kink.numel()
            msk = d64(masks[l + 1][r0:r0 + chunk]) / (1 - p) if (masks is not None and l < NL - 1) else torch.ones_like(z)
            gt = (z > 0).double() * msk
            h = z.clamp(min=0) * msk
            Eh = (Ez + U * z.abs()) * msk * ((z > 0) | kink).double()      # a unit below its kink is exactly 0
            hs.append(h); Ehs.append(Eh); gates.append(gt)
        amb_rows.append(amb)
        if not want_bwd:
            continue
        dz = d64(dout[r0:r0 + chunk]).reshape(-1, 1)
        Edz = torch.zeros_like(dz)
        for l in range(NL, -1, -1):
            h, Eh = hs[l], Ehs[l]
            dW[l] += dz.t() @ h
            EdW[l] += c * U * (dz.abs().t() @ h.abs()) + Edz.t() @ h.abs() + dz.abs().t() @ Eh
            db[l] += dz.sum(0)
            Edb[l] += c * U * dz.abs().sum(0) + Edz.sum(0)
            if l == 0:
                break
            dh = dz @ Ws[l]
            Edh = c * U * (dz.abs() @ Ws[l].abs()) + Edz @ Ws[l].abs()
            dz, Edz = dh * gates[l - 1], (Edh + U * dh.abs()) * gates[l - 1]
    res = dict(out=torch.cat(outs), E_out=torch.cat(Eouts), amb_rows=torch.cat(amb_rows), amb_frac=n_amb / max(n_units, 1))
    if want_bwd:
        res.update(dW=dW, E_dW=EdW, db=db, E_db=Edb)
    return res


# ---------------------------------------------------------------------------------------------------------------------------- BN + AF
def bn_blocks(R):
    """Chunks of the whole-batch statistics (csrc/bnact.hip bn_blocks): one per 256 rows, at most 512."""
    return max(1, min(512, (R + 255) // 256))


def real_rows_mask(R, lens=None, L=0):
    if lens is None:
        return torch.ones(R, dtype=torch.bool)
    r = torch.arange(R)
    return (r % L) < d64(lens).long()[r // L]


def bn_stats(z, c, group=0, lens=None, L=0, eps=1e-5):
    """Float64 mean / rstd of the columns of z (whole batch, or per group of `group` rows; real rows only) and their bounds, with the
    kernel's chunk pivots.  Returns (mean, rstd, E_mean, E_rstd) as [G, N]."""
    z = d64(z)
    R, N = z.shape
    real = real_rows_mask(R, lens, L).double().reshape(-1, 1)
    chunk = group if group else -(-R // bn_blocks(R))
    starts = (torch.arange(R) // chunk) * chunk
    dk = (z - z[starts]) * real                               # d = z - k (pivot: the chunk's first row, padded or not)
    G = R // group if group else 1
    zg, dg, rg = z.view(G, -1, N), dk.view(G, -1, N), real.view(G, -1, 1)
    n = rg.sum(1).clamp(min=1)
    mean = (zg * rg).sum(1) / n
    var = (((zg - mean[:, None]) ** 2) * rg).sum(1) / n
    A, S2 = dg.abs().sum(1) / n, (dg ** 2).sum(1) / n
    # |chunk mean - mean| per row (whole batch: chunks of `chunk` rows; grouped: the group is the chunk)
    cid = torch.arange(R) // chunk
    nc = int(cid.max()) + 1
    csum = torch.zeros(nc, N, dtype=torch.float64).index_add_(0, cid, z * real)
    ccnt = torch.zeros(nc, dtype=torch.float64).index_add_(0, cid, real[:, 0]).clamp(min=1)
    cmean = csum / ccnt[:, None]
    D = ((cmean[cid] - mean.repeat_interleave(R // G, 0)).abs() * real).view(G, -1, N).sum(1) / n
    rstd = 1.0 / torch.sqrt(var + eps)
    E_mean = c * U * (mean.abs() + A)
    E_var = c * U * (S2 + D * (mean.abs() + A))
    E_rstd = rstd * (E_var / (2 * (var + eps)) + c * U)
    return mean, rstd, E_mean, E_rstd


def af_f(af, y):
    """Activation, derivative, second derivative and the evaluation bounds of the first two (without c u), float64."""
    one = torch.ones_like(y)
    if af == AF_NONE:
        return y, one, torch.zeros_like(y), torch.zeros_like(y), torch.zeros_like(y)
    if af == AF_RELU:
        return y.clamp(min=0), (y > 0).double(), torch.zeros_like(y), y.clamp(min=0), torch.zeros_like(y)
    if af == AF_LEAKY:
        f = torch.where(y > 0, y, 0.01 * y)
        return f, torch.where(y > 0, one, 0.01 * one), torch.zeros_like(y), f.abs(), torch.zeros_like(y)
    if af in (AF_ELU, AF_SELU):
        s, a = (1.0507009873554805, 1.6732632423543772) if af == AF_SELU else (1.0, 1.0)
        ey = torch.exp(y.clamp(max=0))
        f = s * torch.where(y > 0, y, a * torch.expm1(y.clamp(max=0)))
        fp = s * torch.where(y > 0, one, a * ey)
        fpp = s * torch.where(y > 0, torch.zeros_like(y), a * ey)
        return f, fp, fpp, f.abs() + s * a * ey * (y <= 0).double(), fp.abs()
    if af == AF_GELU:
        erf = torch.erf(y / math.sqrt(2.0))
        pdf = torch.exp(-0.5 * y * y) / math.sqrt(2 * math.pi)
        f = 0.5 * y * (1 + erf)
        fp = 0.5 * (1 + erf) + y * pdf
        fpp = pdf * (2 - y * y)
        Ef = 0.5 * y.abs() * (1 + erf.abs()) + f.abs()            # times c u; plus 0.5 |y| ERF_FAST_ABS (added in bnact_*)
        Efp = 0.5 * (1 + erf.abs()) + y.abs() * pdf * (2 + y * y) + fp.abs()
        return f, fp, fpp, Ef, Efp
    if af == AF_SIGMOID:
        s = torch.sigmoid(y)
        return s, s * (1 - s), s * (1 - s) * (1 - 2 * s), s, s
    if af == AF_TANH:
        t = torch.tanh(y)
        return t, 1 - t * t, -2 * t * (1 - t * t), t.abs(), t * t + (1 - t * t)
    raise ValueError(af)


def _erf_terms(af, y):
    """The erf_fast absolute-error terms (not scaled by c) of f and f'."""
    if af != AF_GELU:
        return 0.0, 0.0
    return 0.5 * y.abs() * ERF_FAST_ABS, 0.5 * ERF_FAST_ABS * (1 + y.abs())


def _bn_setup(z, mean, rstd, gamma, beta, group, c):
    z = d64(z)
    R, N = z.shape
    G = R // group if group else 1
    mu = d64(mean).reshape(G, N).repeat_interleave(R // G, 0)
    rs = d64(rstd).reshape(G, N).repeat_interleave(R // G, 0)
    ga = d64(gamma).reshape(1, N) if gamma is not None else torch.ones(1, N, dtype=torch.float64)
    be = d64(beta).reshape(1, N) if beta is not None else torch.zeros(1, N, dtype=torch.float64)
    xh = (z - mu) * rs
    y = ga * xh + be
    E_xh = c * U * xh.abs()
    E_y = ga.abs() * E_xh + c * U * y.abs()
    return z, xh, y, ga, rs, E_xh, E_y


def bnact_fwd(z, mean, rstd, gamma, beta, af, c, group=0, keep=None, p=0.0):
    """a = f(gamma (z - mean) rstd + beta) keep / (1 - p) with the kernel's own mean / rstd (None: no batch norm).  Returns (a, E_a,
    accept) — accept: elements at a ReLU / leaky kink (|y| <= E_y) where the kernel may take either branch (within E_a of it)."""
    if mean is None:
        y = d64(z); E_y = torch.zeros_like(y)
    else:
        _, _, y, _, _, _, E_y = _bn_setup(z, mean, rstd, gamma, beta, group, c)
    f, fp, _, Ef, _ = af_f(af, y)
    e1, _ = _erf_terms(af, y)
    scale = d64(keep) / (1 - p) if keep is not None else torch.ones_like(y)
    a = f * scale
    E = (fp.abs() * E_y + c * U * Ef + e1 + FLT_MIN) * scale + U * a.abs()
    accept = None
    if af in (AF_RELU, AF_LEAKY):
        amb = y.abs() <= E_y
        alt = torch.where(y > 0, (0.01 if af == AF_LEAKY else 0.0) * y, y) * scale      # the other branch
        accept = amb, alt, (E_y + U * y.abs()) * scale
    return a, E, accept


def accept_from(got, accept):
    if accept is None:
        return None
    amb, alt, Ealt = accept
    return amb & ((d64(got) - alt).abs() <= Ealt)


def bnact_bwd(z, da, mean, rstd, gamma, beta, af, c, group=0, keep=None, p=0.0, lens=None, L=0):
    """dz, dgamma (= sum dy xh), dbeta (= sum dy) and their bounds, with the kernel's own mean / rstd.  Grouped (group > 0): dgamma /
    dbeta summed over every group.  Returns dict(dz, E_dz, dgamma, E_dgamma, dbeta, E_dbeta, amb) — amb: elements at a ReLU / leaky kink
    (the derivative itself undecidable; keep their da 0)."""
    z, xh, y, ga, rs, E_xh, E_y = _bn_setup(z, mean, rstd, gamma, beta, group, c)
    R, N = z.shape
    real = real_rows_mask(R, lens, L).double().reshape(-1, 1)
    scale = d64(keep) / (1 - p) if keep is not None else torch.ones_like(z)
    f, fp, fpp, _, Efp = af_f(af, y)
    _, e2 = _erf_terms(af, y)
    da = d64(da) * real
    dy = da * scale * fp
    E_dy = da.abs() * scale * (fpp.abs() * E_y + c * U * Efp + e2 + FLT_MIN) + c * U * dy.abs()
    amb = (y.abs() <= E_y) & (da != 0) if af in (AF_RELU, AF_LEAKY) else torch.zeros_like(z, dtype=torch.bool)
    G = R // group if group else 1
    v = lambda t: t.view(G, -1, N)
    n = v(real.expand(R, N)).sum(1).clamp(min=1)
    sdy, sdyx = v(dy).sum(1), v(dy * xh).sum(1)
    E_sdy = c * U * v(dy.abs()).sum(1) + v(E_dy).sum(1)
    E_sdyx = c * U * v((dy * xh).abs()).sum(1) + v(E_dy * xh.abs() + dy.abs() * E_xh).sum(1)
    rep = lambda t: t.repeat_interleave(R // G, 0)
    s1, s2, n_, e1_, e2_ = rep(sdy), rep(sdyx), rep(n), rep(E_sdy), rep(E_sdyx)
    gr = ga.abs() * rs
    dz = ga * rs * (dy - s1 / n_ - xh * s2 / n_) * real
    E_dz = (gr * (E_dy + e1_ / n_ + E_xh * s2.abs() / n_ + xh.abs() * e2_ / n_)
            + c * U * gr * (dy.abs() + s1.abs() / n_ + xh.abs() * s2.abs() / n_)) * real
    return dict(dz=dz, E_dz=E_dz, dgamma=sdyx.sum(0), E_dgamma=E_sdyx.sum(0) + c * U * sdyx.abs().sum(0),
                dbeta=sdy.sum(0), E_dbeta=E_sdy.sum(0) + c * U * sdy.abs().sum(0), amb=amb)


# ---------------------------------------------------------------------------------------------------------------------------- attention
def attn_inputs(B, L, F, H, seed=0):
    """fp32 Q, K, V, dO [B, L, F] shaped to make the attention bounds bite: per-head scales of Q, K and V spread over ~2^10; every
    other head (head 0 of a one-head call with an even seed) peaked, |S| up to ~60; dO columns scaled 2^-10..1 and ~10 % zero rows.
    Returns (Q, K, V, dO, lens) with lens [B] int32 = L, 1, then random (B >= 2), or all L (B == 1)."""
    g = torch.Generator().manual_seed(seed)
    dh = F // H
    r = lambda: torch.randn(B, L, H, dh, generator=g, dtype=torch.float64)
    e = lambda lo, hi: torch.pow(2.0, torch.randint(lo, hi + 1, (1, 1, H, 1), generator=g).double())
    peaked = ((torch.arange(H) + seed) % 2 == 0).double().reshape(1, 1, H, 1)
    sq, sk = e(-5, 3), e(-5, 3)
    sq = peaked * 6.0 + (1 - peaked) * sq                      # S = q.k / sqrt(dh) ~ N(0, sq sk): 6 x 2.5 -> |S| up to ~60
    sk = peaked * 2.5 + (1 - peaked) * sk
    Q, K, V = r() * sq, r() * sk, r() * e(-5, 5)
    dO = torch.randn(B, L, F, generator=g, dtype=torch.float64) * torch.pow(2.0, torch.randint(-10, 1, (1, 1, F), generator=g).double())
    dO[torch.rand(B, L, generator=g) < 0.1] = 0.0
    lens = torch.randint(1, L + 1, (B,), generator=g, dtype=torch.int32)
    lens[0] = L
    if B >= 2:
        lens[1] = 1
    f = lambda t: t.reshape(B, L, F).float().contiguous()
    return f(Q), f(K), f(V), dO.float().contiguous(), lens


def _heads(T, H):
    """[B, L, F] -> float64 [B, H, L, dh] (heads are column blocks)."""
    B, L, F = T.shape
    return d64(T).reshape(B, L, H, F // H).permute(0, 2, 1, 3)


def _merge(T):
    """float64 [B, H, L, dh] -> [B, L, H * dh]."""
    B, H, L, dh = T.shape
    return T.permute(0, 2, 1, 3).reshape(B, L, H * dh)


def _attn_setup(Q, K, H, lens, keep, p, c):
    q, k = _heads(Q, H), _heads(K, H)
    B, _, L, dh = q.shape
    s = 1.0 / math.sqrt(dh)
    S = s * (q @ k.transpose(-1, -2))
    E_S = c * U * s * (q.abs() @ k.abs().transpose(-1, -2))
    n = d64(lens).long() if lens is not None else torch.full((B,), L, dtype=torch.long)
    ok = (torch.arange(L)[None, :] < n[:, None]).reshape(B, 1, 1, L)
    kp = d64(keep) / (1.0 - p) if keep is not None else torch.ones(1, dtype=torch.float64)
    return q, k, s, S, E_S, ok, kp


def mhsa_fwd(Q, K, V, H, keep, p, lens, c):
    """O = softmax(s Q_h K_h^T, keys < lens) keep' V_h and LSE [B, H, L] with their bounds (module docstring).  keep: the kernel's
    [B, H, L, L] 1/0 keep mask (ptr_mhsa_dropout_mask) or None.  A query with no key (lens 0) has O = 0, LSE = 0 exactly.
    Returns (O, E_O, LSE, E_LSE)."""
    q, k, s, S, E_S, ok, kp = _attn_setup(Q, K, H, lens, keep, p, c)
    v = _heads(V, H)
    has = ok.any(-1, keepdim=True)
    Sm = S.masked_fill(~ok, -math.inf)
    m = torch.where(has, Sm.amax(-1, keepdim=True), torch.zeros(1, dtype=torch.float64))
    lse = torch.where(has, torch.logsumexp(Sm, -1, keepdim=True), torch.zeros(1, dtype=torch.float64))
    P = torch.exp(Sm - torch.where(has, lse, torch.zeros(1, dtype=torch.float64)))
    e = torch.where(ok, E_S + c * U * (1.0 + (S - m).abs()), torch.zeros(1, dtype=torch.float64))
    Pe = (P * e).sum(-1, keepdim=True)
    E_P = P * (e + Pe) + FLT_MIN * ok
    Pd, E_Pd = P * kp, E_P * kp
    O = Pd @ v
    E_O = c * U * (Pd.abs() @ v.abs()) + E_Pd @ v.abs()
    E_lse = torch.where(has, Pe + c * U * (lse.abs() + 1.0), torch.zeros(1, dtype=torch.float64))
    return _merge(O), _merge(E_O), lse[..., 0], E_lse[..., 0]


def mhsa_bwd(Q, K, V, O_k, dO, lse_k, H, keep, p, lens, c):
    """dQ, dK, dV of the attention core for output gradient dO, given the kernel's own O and LSE ([B, L, F] and B*H*L), with their
    bounds (module docstring).  Returns dict(dQ, E_dQ, dK, E_dK, dV, E_dV) as [B, L, F]."""
    q, k, s, S, E_S, ok, kp = _attn_setup(Q, K, H, lens, keep, p, c)
    v, o, g = _heads(V, H), _heads(O_k, H), _heads(dO, H)
    B, _, L, _ = q.shape
    lse = d64(lse_k).reshape(B, H, L, 1)
    P = torch.where(ok, torch.exp(S - lse), torch.zeros(1, dtype=torch.float64))
    E_P = P * (E_S + c * U * (1.0 + (S - lse).abs())) + FLT_MIN * ok
    D = (o * g).sum(-1, keepdim=True)
    E_D = c * U * (o.abs() * g.abs()).sum(-1, keepdim=True)
    dP = g @ v.transpose(-1, -2)
    E_dP = c * U * (g.abs() @ v.abs().transpose(-1, -2))
    dPk = dP * kp
    t = dPk - D
    dS = P * t * s
    E_dS = s * (P * (E_dP * kp + E_D + c * U * (dPk.abs() + D.abs())) + E_P * t.abs())
    Pd, E_Pd = P * kp, E_P * kp
    aS, tS = dS.abs(), lambda x: x.transpose(-1, -2)
    res = dict(dQ=dS @ k, E_dQ=c * U * (aS @ k.abs()) + E_dS @ k.abs(),
               dK=tS(dS) @ q, E_dK=c * U * (tS(aS) @ q.abs()) + tS(E_dS) @ q.abs(),
               dV=tS(Pd) @ g, E_dV=c * U * (tS(Pd.abs()) @ g.abs()) + tS(E_Pd) @ g.abs())
    return {key: _merge(val) for key, val in res.items()}


# ---------------------------------------------------------------------------------------------------------------------------- LayerNorm
def layernorm_fwd(x, a2, b2, eps, c):
    """y = a2 (x - mean) / (sd + eps) + b2 per row (sd unbiased) with its bound, and the statistics the kernel exports.  Returns
    (y, E_y, stats) with stats = dict(mean, rinv, sd, E_mean, E_rinv, E_sd), each [R]."""
    x = d64(x)
    F = x.shape[1]
    a, b = d64(a2).reshape(1, F), d64(b2).reshape(1, F)
    mean = x.mean(1, keepdim=True)
    cc = x - mean
    var = (cc * cc).sum(1, keepdim=True) / (F - 1)
    sd = var.sqrt()
    rinv = 1.0 / (sd + eps)
    y = a * cc * rinv + b
    E_mean = c * U * x.abs().mean(1, keepdim=True)
    E_c = E_mean + U * cc.abs()
    E_var = (c * U * (cc * cc).sum(1, keepdim=True) + F * E_mean ** 2 + 2 * U * E_mean * cc.abs().sum(1, keepdim=True)) / (F - 1)
    E_sd = torch.where(sd > 0, torch.minimum(E_var / (2 * sd), E_var.sqrt()), E_var.sqrt()) + c * U * sd
    E_rinv = rinv ** 2 * (E_sd + c * U * (sd + eps)) + c * U * rinv
    E_y = a.abs() * (E_c * rinv + cc.abs() * E_rinv) + c * U * ((a * cc * rinv).abs() + y.abs())
    st = dict(mean=mean[:, 0], rinv=rinv[:, 0], sd=sd[:, 0], E_mean=E_mean[:, 0], E_rinv=E_rinv[:, 0], E_sd=E_sd[:, 0])
    return y, E_y, st


def layernorm_bwd(x, a2, dy, stats_k, c):
    """dx, da2, db2 of the LayerNorm for output gradient dy, given the kernel's stats [R, 3] = {mean, rinv, sd} (exact inputs), with
    their bounds.  Rows with sd = 0 drop the second term, as the kernel does.  Returns dict(dx, E_dx, da, E_da, db, E_db)."""
    x, dy, st = d64(x), d64(dy), d64(stats_k).reshape(-1, 3)
    F = x.shape[1]
    a = d64(a2).reshape(1, F)
    mean, rinv, sd = st[:, 0:1], st[:, 1:2], st[:, 2:3]
    cc = x - mean
    gg = dy * a
    gbar = gg.sum(1, keepdim=True) / F
    pos = sd > 0
    den = torch.where(pos, sd * (F - 1), torch.ones(1, dtype=torch.float64))
    k2 = torch.where(pos, rinv ** 2 * (gg * cc).sum(1, keepdim=True) / den, torch.zeros(1, dtype=torch.float64))
    E_k2 = torch.where(pos, rinv ** 2 * c * U * (gg * cc).abs().sum(1, keepdim=True) / den, torch.zeros(1, dtype=torch.float64))
    dx = rinv * (gg - gbar) - cc * k2
    E_dx = (rinv * c * U * gg.abs().sum(1, keepdim=True) / F + cc.abs() * E_k2
            + c * U * (rinv * (gg.abs() + gbar.abs()) + (cc * k2).abs()))
    t = dy * cc * rinv
    return dict(dx=dx, E_dx=E_dx, da=t.sum(0), E_da=c * U * t.abs().sum(0), db=dy.sum(0), E_db=c * U * dy.abs().sum(0))


def ln_inputs(R, F, seed=0):
    """fp32 [R, F] LayerNorm inputs, a2, b2 and dy: rows of scale 2^-8..2^8, a quarter of them offset by 100..1000x their spread,
    near-constant rows (spread 2^-20 of the value), exactly constant rows (1.5 x 2^k: sums exact in fp32; and 0.1: not), ~5 % all-zero
    rows (padded documents); dy rows scaled 2^-12..1 with columns scaled 2^-6..1.  Returns (x, a2, b2, dy, kinds) with kinds [R]:
    0 plain, 1 offset, 2 near-constant, 3 constant exact, 4 constant inexact, 5 zero."""
    g = torch.Generator().manual_seed(seed)
    sc = torch.pow(2.0, torch.randint(-8, 9, (R, 1), generator=g).double())
    x = torch.randn(R, F, generator=g, dtype=torch.float64) * sc
    u = torch.rand(R, generator=g)
    kinds = torch.zeros(R, dtype=torch.long)
    kinds[u < 0.25] = 1
    kinds[(u >= 0.25) & (u < 0.3)] = 2
    kinds[(u >= 0.3) & (u < 0.33)] = 3
    kinds[(u >= 0.33) & (u < 0.36)] = 4
    kinds[u >= 0.95] = 5
    if R >= 6:
        kinds[:6] = torch.arange(6)                      # every kind at least once
    off = sc * (100.0 + 900.0 * torch.rand(R, 1, generator=g, dtype=torch.float64))
    x = torch.where((kinds == 1)[:, None], x + off, x)
    x = torch.where((kinds == 2)[:, None], off * (1.0 + 2.0 ** -20 * torch.randn(R, F, generator=g, dtype=torch.float64)), x)
    x = torch.where((kinds == 3)[:, None], 1.5 * sc, x)
    x = torch.where((kinds == 4)[:, None], 0.1 * torch.ones_like(x), x)
    x = torch.where((kinds == 5)[:, None], torch.zeros_like(x), x)
    a2 = 1.0 + 0.5 * torch.randn(F, generator=g, dtype=torch.float64)
    b2 = 0.1 * torch.randn(F, generator=g, dtype=torch.float64)
    dy = (torch.randn(R, F, generator=g, dtype=torch.float64) * torch.pow(2.0, torch.randint(-12, 1, (R, 1), generator=g).double())
          * torch.pow(2.0, torch.randint(-6, 1, (1, F), generator=g).double()))
    return x.float().contiguous(), a2.float(), b2.float(), dy.float().contiguous(), kinds
