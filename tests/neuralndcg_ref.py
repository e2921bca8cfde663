"""NeuralNDCG, the rule of include/ptranking_amd.h in plain torch: the explicit [n, n] matrix, a loop of T iterations, autograd.  float64 is the
reference of the GPU tests; at float32 it is the eager evaluation whose error sets the gate's constant C.  Shares nothing with the kernel."""
import torch

EPS = 1e-10


def ndcg_query(s, y, tau=1.0, iters=50, top_k=None, powered=True, return_matrix=False):
    """One query of n real documents (1-d tensors, any float dtype; s may require grad) -> ndcg_q as a 0-d tensor (or the matrix P)."""
    n, dt = s.numel(), s.dtype
    g = (torch.pow(torch.tensor(2.0, dtype=dt), y.to(dt)) - 1.0) if powered else y.to(dt)
    k = n if not top_k else min(int(top_k), n)
    d = 1.0 / torch.log2(torch.arange(n, dtype=dt) + 2.0)
    idcg = (torch.sort(g, descending=True).values[:k] * d[:k]).sum()
    if n == 0 or not idcg > 0:
        return s.sum() * 0.0
    B = (s[:, None] - s[None, :]).abs().sum(dim=1)                       # B_j
    c = (n + 1 - 2 * (torch.arange(n, dtype=dt) + 1.0))                  # c_i
    logits = (c[:, None] * s[None, :] - B[None, :]) / tau                # row i a position, column j a document
    P = torch.softmax(logits, dim=1)
    for _ in range(int(iters)):
        P = P / P.sum(dim=0, keepdim=True).clamp(min=EPS)
        P = P / P.sum(dim=1, keepdim=True).clamp(min=EPS)
    if return_matrix:
        return P
    return (d[:k] * (P[:k] * g[None, :]).sum(dim=1)).sum() / idcg


def loss_and_grad(preds, labels, lens=None, dtype=torch.float64, **kw):
    """[B, L] batch -> (loss_q [B], grad [B, L]) at `dtype`, padded slots 0; loss_q = -ndcg_q."""
    Bq, L = preds.shape
    loss_q = torch.zeros(Bq, dtype=dtype)
    grad = torch.zeros(Bq, L, dtype=dtype)
    for q in range(Bq):
        n = L if lens is None else int(lens[q])
        s = preds[q, :n].to(dtype).clone().requires_grad_(True)
        loss = -ndcg_query(s, labels[q, :n], **kw)
        loss.backward()
        loss_q[q], grad[q, :n] = loss.detach(), s.grad
    return loss_q, grad
