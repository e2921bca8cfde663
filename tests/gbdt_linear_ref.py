"""Float64 numpy restatement of linear trees (rules 1 to 7 of include/ptranking_amd.h; ptranking_amd/csrc/gbdt_linear.hip): the leaf fit and the
leaf output only; the grower is tests/gbdt_ref.py's.  Test infrastructure, never imported by the package.  Nothing here is LightGBM's."""
import numpy as np

import gbdt_ref as R

K = 30
FLOOR = 2.0 ** -40
GAMMA_NUMPY = 0.30           # measured (test_gbdt_linear_cpu.py): the worst residual factor of numpy's own float64 Cholesky solve on SOLVE_CASES
GAMMA = 4.0 * GAMMA_NUMPY    # what the kernel gets: it eliminates in another order, without pivoting
SOLVE_CASES = [(k, lam) for k in (1, 16, 30) for lam in (0.0, 1.0)]


def path_features(tree):
    """Rule 1 -> per leaf the list of distinct features on its path, in order of first appearance from the root."""
    out = [None] * (tree["feature"].size + 1)

    def down(at, path):
        if at < 0:
            out[~at] = path
            return
        f = int(tree["feature"][at])
        here = path if f in path else path + [f]
        down(int(tree["left"][at]), here)
        down(int(tree["right"][at]), here)
    down(0 if tree["feature"].size else ~0, [])
    return out


def moments(X, rows, P, g, h, dtype=np.float64):
    """Rules 2 and 3 over the rows of a leaf -> (A [k+1, k+1], b [k+1], m_u, sum |h z z^T|, sum |g z|)."""
    X, rows = np.asarray(X, np.float32), np.asarray(rows, np.int64)
    z = np.concatenate([X[rows][:, P].astype(dtype), np.ones((rows.size, 1), dtype)], axis=1)
    ok = ~np.isnan(z).any(axis=1)
    z, gg, hh = z[ok], np.asarray(g, np.float32)[rows][ok].astype(dtype), np.asarray(h, np.float32)[rows][ok].astype(dtype)
    T = hh[:, None, None] * (z[:, :, None] * z[:, None, :])
    return T.sum(0), (gg[:, None] * z).sum(0), int(ok.sum()), np.abs(T).sum(0), np.abs(gg[:, None] * z).sum(0)


def solve(A, b, k, m_u, lam):
    """Rules 4 and 5 -> (c float64 [k + 1] or None, status, the smallest pivot ratio p_j / (A + L)_jj seen)."""
    if k == 0:
        return None, 1, np.inf
    if k > K:
        return None, 2, np.inf
    if m_u < k + 1:
        return None, 3, np.inf
    M = np.array(A, np.float64) + np.diag([lam] * k + [0.0])
    d0, L, worst = np.diag(M).copy(), np.zeros_like(M), np.inf
    for j in range(k + 1):
        p = M[j, j] - L[j, :j] @ L[j, :j]
        with np.errstate(all="ignore"):
            worst = min(worst, p / d0[j] if np.isfinite(p) and d0[j] > 0 else 0.0)
        if not (np.isfinite(p) and p > FLOOR * d0[j]):
            return None, 4, worst
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    c = -np.linalg.solve(L.T, np.linalg.solve(L, np.asarray(b, np.float64)))
    return (c, 0, worst) if np.isfinite(c).all() else (None, 5, worst)


def residual_factor(A, b, k, lam, c):
    """|| (A + L) c + b ||_inf / ((k + 1) 2^-52 ||A + L||_inf ||c||_inf): what test 2 bounds by GAMMA."""
    M = np.array(A, np.float64) + np.diag([lam] * k + [0.0])
    return np.abs(M @ c + b).max() / ((k + 1) * 2.0 ** -52 * np.abs(M).sum(1).max() * np.abs(c).max())


def solve_case(k, lam, m=200, seed=0):
    """The well-conditioned system of a SOLVE_CASES entry from random fp32 data -> (A, b, m_u)."""
    rng = np.random.default_rng(100 * k + seed)
    X = rng.standard_normal((m, k)).astype(np.float32)
    g, h = rng.standard_normal(m).astype(np.float32), (0.5 + rng.random(m)).astype(np.float32)
    return moments(X, np.arange(m), list(range(k)), g, h)[:3]


def workspace(systems):
    """One partial per leaf in ptr_gbdt_linear_moments' layout: (ws [leaves, 32, 32], usable, item_offsets, nfeat) from [(A, b, m_u, k)]."""
    ws = np.zeros((len(systems), 32, 32))
    for l, (A, b, _, k) in enumerate(systems):
        ws[l, :k + 1, :k + 1], ws[l, :k + 1, k + 1] = A, b
    return ws, np.array([s[2] for s in systems], np.int32), np.arange(len(systems) + 1, dtype=np.int32), np.array([s[3] for s in systems], np.int32)


def leaf_output(x, value, feats, coeff, const):
    """Rule 7 for one row, float64 (the kernel rounds it to fp32)."""
    if feats[0] < 0:
        return np.float64(value)
    acc = np.float64(const)
    for f, cj in zip(feats, coeff):
        if f < 0:
            break
        if np.isnan(x[f]):
            return np.float64(value)
        acc = acc + np.float64(cj) * np.float64(x[f])
    return acc


def assign(X, tree):
    """The leaf of every row under the raw predictor's predicate: left on x <= threshold, a NaN along default_left."""
    leaf = np.zeros(len(X), np.int64)
    for i, x in enumerate(np.asarray(X, np.float32)):
        node = 0 if tree["feature"].size else ~0
        while node >= 0:
            xv = x[tree["feature"][node]]
            go = bool(tree["default_left"][node]) if np.isnan(xv) and "default_left" in tree else xv <= tree["threshold"][node]
            node = tree["left"][node] if go else tree["right"][node]
        leaf[i] = ~node
    return leaf


def tree_outputs(X, tree):
    """One tree's float64 outputs for every row."""
    leaf = assign(X, tree)
    return np.array([leaf_output(x, tree["value"][l], tree["leaf_features"][l], tree["leaf_coeff"][l], tree["leaf_const"][l])
                     for x, l in zip(np.asarray(X, np.float32), leaf)])


def flat(trees):
    """GBDT.flat()'s layout for hand-made trees."""
    cat = lambda k: np.concatenate([t[k] for t in trees])
    out = {k: cat(k) for k in trees[0]}
    out["tree_offsets"] = np.concatenate([[0], np.cumsum([t["feature"].size for t in trees])]).astype(np.int32)
    return out


def fit_squared_error(X, y, rounds, linear, num_leaves=6, lr=0.5, max_bin=63, min_data=5, lam=0.0):
    """A whole fit under squared error on the restatement alone (tests/gbdt_ref.py grows, this file fits the leaves) -> (trees, float64
    scores as the fp32 sums predict makes).  What the `plain` case of the GPU fits trains, so its loss gap is known before a GPU runs."""
    X, y = np.asarray(X, np.float32), np.asarray(y, np.float32)
    edges, nbins = R.bin_edges(X, max_bin)
    bins = R.bin_matrix(X, edges, nbins)
    scores, trees = np.zeros(len(X), np.float32), []
    for _ in range(rounds):
        g, h = (scores - y).astype(np.float32), np.ones(len(X), np.float32)
        qg, qh, expo, _ = R.quantize(g, h)
        t, leaf_rows, _ = R.grow_tree(bins, qg, qh, expo, edges, nbins, max_bin, num_leaves, lr=lr, min_data=min_data)
        nl = t["value"].size
        t["leaf_features"], t["leaf_coeff"], t["leaf_const"] = np.full((nl, K), -1, np.int32), np.zeros((nl, K)), np.zeros(nl)
        for l, P in enumerate(path_features(t) if linear else []):
            A, b, m_u = moments(X, leaf_rows[l], P, g, h)[:3]
            c, status, _ = solve(A, b, len(P), m_u, lam)
            if status == 0:
                t["leaf_features"][l, :len(P)], t["leaf_coeff"][l, :len(P)], t["leaf_const"][l] = P, c[:-1] * lr, c[-1] * lr
        scores = (scores + tree_outputs(X, t).astype(np.float32)).astype(np.float32)
        trees.append(t)
    return trees, scores
