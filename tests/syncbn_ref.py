"""Test-side float64 restatement of the synchronised 'BN' statistics (include/ptranking_amd.h, "synchronised 'BN' statistics across
data-parallel ranks"): W ranks hold uneven pieces of one batch, exchange one slot (mean, M2, count) each in the forward and one pair of
column sums each in the backward, and must end with what ONE rank computes on the whole batch.  Not product code: it is the executable
specification the GPU tests compare the kernels' data flow against, and tests/test_syncbn_cpu.py checks it against whole-batch
statistics and against autograd of the whole batch.

The activation is left out (dy is taken as given): the split concerns the batch-norm part of the backward only."""
import torch

EPS = 1e-5


def partial(z, real=None):
    """One rank's slot: (mean [N], M2 [N], count) over its real rows.  z [R, N] float64, real [R] bool or None.  count 0: mean 0, M2 0."""
    z = z.double()
    r = torch.ones(z.shape[0], dtype=torch.float64) if real is None else real.double()
    n = float(r.sum())
    if n == 0:
        return torch.zeros(z.shape[1], dtype=torch.float64), torch.zeros(z.shape[1], dtype=torch.float64), 0.0
    mean = (z * r[:, None]).sum(0) / n
    m2 = (((z - mean) ** 2) * r[:, None]).sum(0)
    return mean, m2, n


def combine(slots, eps=EPS):
    """Rank-order parallel-variance combination of the slots [(mean, M2, count)] -> mean, rstd, total count (>= 1).  A slot with count 0
    is skipped.  Biased variance, as BatchNorm normalises."""
    n = sum(c for _, _, c in slots)
    n = max(n, 1.0)
    N = slots[0][0].numel()
    mean = torch.zeros(N, dtype=torch.float64)
    for m, _, c in slots:                       # rank order 0 .. W-1
        if c > 0:
            mean = mean + c * m
    mean = mean / n
    m2 = torch.zeros(N, dtype=torch.float64)
    for m, q, c in slots:
        if c > 0:
            m2 = m2 + (q + c * (m - mean) ** 2)
    return mean, 1.0 / torch.sqrt(m2 / n + eps), n


def backward_sums(z, dy, mean, rstd, real=None):
    """One rank's [sum dy | sum dy xhat] over its real rows with the GLOBAL mean / rstd: its dbeta | dgamma."""
    r = torch.ones(z.shape[0], dtype=torch.float64) if real is None else real.double()
    xh = (z.double() - mean) * rstd
    d = dy.double() * r[:, None]
    return d.sum(0), (d * xh).sum(0)


def backward_apply(z, dy, mean, rstd, gamma, sums, n, real=None):
    """dz of one rank's rows from every rank's sums (added in rank order) and the global count n; a padded row's dz is 0."""
    r = torch.ones(z.shape[0], dtype=torch.float64) if real is None else real.double()
    s1 = sum(s[0] for s in sums)
    s2 = sum(s[1] for s in sums)
    xh = (z.double() - mean) * rstd
    return (gamma * rstd) * (dy.double() - s1 / n - xh * (s2 / n)) * r[:, None]


def split_rows(R, W, empty=None, seed=0):
    """Cut [0, R) into W uneven consecutive pieces [(lo, hi)]; piece `empty` (if any) gets no rows of its own — the tests give it rows
    that are all padding instead."""
    g = torch.Generator().manual_seed(seed)
    live = [w for w in range(W) if w != empty]
    cuts = sorted(int(c) for c in (torch.randperm(R - 1, generator=g)[:len(live) - 1] + 1)) if len(live) > 1 else []
    edges = [0] + cuts + [R]
    out, k = [], 0
    for w in range(W):
        if w == empty:
            out.append((edges[k], edges[k]))
        else:
            out.append((edges[k], edges[k + 1]))
            k += 1
    return out
