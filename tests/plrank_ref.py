"""PL-Rank, the rule of include/ptranking_amd.h in plain torch on GIVEN rankings `perm`.  float64 is the reference of the GPU tests; at float32 it
is the eager evaluation whose error sets the gate's constant.  Also returns the element-wise rounding bound: 2^-24 times the sum of the
absolute values of the terms each output is built from.  Shares nothing with the kernel."""
import itertools

import torch

EPS32 = 2.0 ** -24


def plrank(preds, labels, perm, lens=None, top_k=10, normalize=True, dtype=torch.float64):
    """preds, labels [B, L], perm int64 [B, S, L], lens [B] or None -> value_q [B], grad [B, L] (of the loss -reward), and their bounds."""
    B, S, L = perm.shape
    pos = torch.arange(L)
    n = torch.full((B,), L) if lens is None else lens.long()
    real = pos[None, :] < n[:, None]                                            # by document and by position alike
    s = torch.where(real, preds, torch.tensor(float("-inf"))).to(dtype)
    nanq = (torch.isnan(s) & real).any(1)
    rho = torch.where(real, torch.pow(2.0, labels.to(dtype)) - 1.0, torch.zeros((), dtype=dtype))
    top_k = int(top_k or 0)
    K = n if top_k <= 0 else torch.where(n < top_k, n, torch.tensor(top_k))
    placed = pos[None, :] < K[:, None]
    theta = torch.where(placed, 1.0 / torch.log2(pos.to(dtype) + 2.0), torch.zeros((), dtype=dtype))
    if normalize:
        idcg = (torch.sort(rho, dim=1, descending=True).values * theta).sum(1, keepdim=True)
        theta = torch.where(idcg > 0, theta / idcg, torch.zeros((), dtype=dtype))
    e = torch.where(real, torch.exp(s - s.max(1, keepdim=True).values.clamp(min=-1e30)), torch.zeros((), dtype=dtype))
    ey, ry = (torch.gather(x[:, None, :].expand(B, S, L), 2, perm) for x in (e, rho))
    suffix = lambda x: torch.flip(torch.cumsum(torch.flip(x, (2,)), 2), (2,))
    D, a = suffix(ey), theta[:, None, :] * ry
    PR = suffix(a)
    PRn = torch.cat((PR[:, :, 1:], torch.zeros(B, S, 1, dtype=dtype)), 2)        # PR at position p + 1
    inv = torch.where(placed[:, None, :], 1.0 / D, torch.zeros((), dtype=dtype))
    RI, DR = torch.cumsum(PR * inv, 2), torch.cumsum(theta[:, None, :] * inv, 2)  # their terms end at K - 1: position p holds c(p)
    out = []
    for sign in (-1.0, 1.0):                                                    # the gradient's terms, then their absolute values
        g = torch.where(real[:, None, :], PRn + ey * (ry.abs() if sign > 0 else ry) * DR + sign * ey * RI, torch.zeros((), dtype=dtype))
        out.append(torch.zeros(B, L, dtype=dtype).scatter_add_(1, perm.reshape(B, S * L), g.reshape(B, S * L)) / S)
    value, grad = a.sum((1, 2)) / S, -out[0]
    value[nanq] = float("nan")
    grad[nanq[:, None] & real] = float("nan")
    return value, grad, EPS32 * a.abs().sum((1, 2)) / S, EPS32 * out[1]


def exact_gradient(s, rho, K):
    """One query, by enumerating the top-K rankings in float64: the exact gradient of the expected DCG@K, and the standard deviation of the
    per-sample estimate g (whose mean over the rankings is asserted to be that gradient)."""
    n, theta = s.numel(), 1.0 / torch.log2(torch.arange(K, dtype=torch.float64) + 2.0)
    x = s.double().clone().requires_grad_(True)
    e = torch.exp(x - x.max())
    expected, mean, second = 0.0, torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for head in itertools.permutations(range(n), K):
        y = list(head) + [i for i in range(n) if i not in head]                # the unplaced tail's order does not enter g
        prob = torch.stack([e[y[p]] / e[y[p:]].sum() for p in range(K)]).prod()
        expected = expected + prob * (theta * rho.double()[list(head)]).sum()
        _, g, _, _ = plrank(s[None], torch.log2(rho + 1.0)[None], torch.tensor(y)[None, None], top_k=K, normalize=False)
        mean += prob.detach() * -g[0]
        second += prob.detach() * g[0] ** 2
    expected.backward()
    assert (mean - x.grad).abs().max() <= 1e-9
    return x.grad, (second - mean ** 2).clamp(min=0).sqrt()
