"""SetRank-style induced self-attention on the rectangular attention kernels (csrc/xattn.hip).

An induced multi-head self-attention block (IMSAB) replaces the L x L self-attention of a `listsf` encoder layer by two CROSS-attentions
through M learned inducing points: the M points attend to the L documents, then the L documents attend to the M results.  The cost per query
and head is O(L M) instead of O(L^2), and the block stays permutation-equivariant in the documents.

    MAB(X, Y)  = LN(H + Drop(rFF(H))),   H = LN(X + Drop(MHA(X, Y, Y)))
    IMSAB(X)   = MAB(X, MAB(I, X))       I [n_induce, hid_dim] learned
    scorer     = head feed-forward stack -> IMSAB x encoder_layers -> tail feed-forward stack to one score per document

This rule is this project's own, modelled on SetRank (Pang et al., SIGIR 2020) and the Set Transformer's ISAB (Lee et al., ICML 2019).
Nothing here is compared with the authors' code and no parity with it is claimed; SetRank's ordinal embeddings of an initial ranking are
not part of it.  The training loss of the `SetRank` ranker is the softmax cross-entropy of ListNet (SetRank's attention-rank loss).

What runs where: both attentions on ptr_xattn_forward / ptr_xattn_backward (one side of at most 64 rows held in LDS, the other streamed; no
[L, M] tensor is written), LayerNorm on ptr_layernorm_*, the projections on the project's GEMMs.  Padded batches: `lens` (int32 [B]) excludes
padded documents as keys of the first attention and as queries of the second.  There is no CPU / eager fallback: CPU tensors raise.
"""
import copy
import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from .host import build_stacked_ffnet
from .linear import FusedLinear, linear
from .listsf import LayerNorm, PositionwiseFeedForward, _need_gpu, _voff

MAX_SHORT = 64         # the kernels' contract: min(Lq, Lk) <= 64 ...
MAX_HEAD_DIM = 128     # ... and head dimension <= 128


class _XattnFn(torch.autograd.Function):
    """Q [Lq, F] (shared by every query: batch stride 0) or [B, Lq, F]; K, V [B, Lk, F], or V None and K the packed [B, Lk, 2F] K|V."""

    @staticmethod
    def forward(ctx, Q, K, V, lens_q, lens_k, n_heads):
        packed = V is None
        Q, K = Q.contiguous(), K.contiguous()
        V = None if packed else V.contiguous()
        B, Lk = K.shape[0], K.shape[1]
        Lq, Fdim = Q.shape[-2], Q.shape[-1]
        dev = K.device
        qbs = Lq * Fdim if Q.dim() == 3 else 0
        ld_kv = 2 * Fdim if packed else Fdim
        O = torch.empty((B, Lq, Fdim), device=dev, dtype=torch.float32)
        lse = torch.empty(B * n_heads * Lq, device=dev, dtype=torch.float32)
        kp, vp = (_voff(K, 0), _voff(K, Fdim)) if packed else (_lib.ptr(K), _lib.ptr(V))
        with torch.cuda.device(dev):
            _lib.call("ptr_xattn_forward", _lib.ptr(Q), Fdim, C.c_int64(qbs), kp, vp, ld_kv, _lib.ptr(lens_q), _lib.ptr(lens_k), B, Lq, Lk, Fdim,
                      n_heads, _lib.ptr(O), _lib.ptr(lse), _lib.current_stream(dev))
        ctx.save_for_backward(Q, K, V, O, lse, lens_q, lens_k)
        ctx.meta = (n_heads, packed, qbs)
        return O

    @staticmethod
    def backward(ctx, dO):
        Q, K, V, O, lse, lens_q, lens_k = ctx.saved_tensors
        n_heads, packed, qbs = ctx.meta
        B, Lk = K.shape[0], K.shape[1]
        Lq, Fdim = Q.shape[-2], Q.shape[-1]
        dev = K.device
        dO = dO.contiguous()
        dQ = torch.empty((B, Lq, Fdim), device=dev, dtype=torch.float32)
        dK = torch.empty_like(K)
        dV = None if packed else torch.empty_like(V)
        dvec = torch.empty_like(lse)
        ld_kv = 2 * Fdim if packed else Fdim
        kp, vp = (_voff(K, 0), _voff(K, Fdim)) if packed else (_lib.ptr(K), _lib.ptr(V))
        dkp, dvp = (_voff(dK, 0), _voff(dK, Fdim)) if packed else (_lib.ptr(dK), _lib.ptr(dV))
        with torch.cuda.device(dev):
            _lib.call("ptr_xattn_backward", _lib.ptr(Q), Fdim, C.c_int64(qbs), kp, vp, ld_kv, _lib.ptr(lens_q), _lib.ptr(lens_k), B, Lq, Lk, Fdim,
                      n_heads, _lib.ptr(O), _lib.ptr(dO), _lib.ptr(lse), _lib.ptr(dvec), _lib.ptr(dQ), dkp, dvp, _lib.current_stream(dev))
        if Q.dim() == 2:
            dQ = dQ.sum(0)                                  # the shared Q's gradient: a B x Lq x F reduction, not worth a kernel
        return dQ, dK, dV, None, None, None


def _lens(lens, dev, B, who):
    if lens is None:
        return None
    lens = lens.to(device=dev, dtype=torch.int32).contiguous()
    if lens.shape != (B,):
        raise ValueError(f"{who}: lens must have shape [{B}]")
    return lens


def _check(Q, K, V, n_heads, who):
    for t in (Q, K) + (() if V is None else (V,)):
        _need_gpu(t, who)
        if t.dtype != torch.float32:
            raise ValueError(f"{who} expects fp32 tensors")
    Fdim = Q.shape[-1]
    kw = Fdim if V is not None else 2 * Fdim
    if Q.dim() not in (2, 3) or K.dim() != 3 or K.shape[-1] != kw or (V is not None and V.shape != K.shape) or \
            (Q.dim() == 3 and Q.shape[0] != K.shape[0]):
        raise ValueError(f"{who} expects Q [Lq, F] or [B, Lq, F] and K, V [B, Lk, F] (or one packed [B, Lk, 2F])")
    if Fdim % n_heads != 0 or Fdim // n_heads > MAX_HEAD_DIM:
        raise ValueError(f"{who}: F = {Fdim} must be a multiple of n_heads = {n_heads} with a head dimension of at most {MAX_HEAD_DIM}")
    if min(Q.shape[-2], K.shape[1]) > MAX_SHORT:
        raise ValueError(f"{who}: min(Lq, Lk) = {min(Q.shape[-2], K.shape[1])} exceeds {MAX_SHORT}: one side must be short")


def cross_attention(Q, K, V, n_heads, lens_q=None, lens_k=None):
    """softmax(Q_h K_h^T / sqrt(d_h)) V_h per head h (column blocks of width F / n_heads) with Lq != Lk allowed and min(Lq, Lk) <= 64.
    Q [Lq, F] (one Q for all queries) or [B, Lq, F]; K, V [B, Lk, F]; returns O [B, Lq, F].  Keys >= lens_k[b] are excluded; query rows >=
    lens_q[b] give zeros and no gradient."""
    _check(Q, K, V, n_heads, "cross_attention")
    B = K.shape[0]
    return _XattnFn.apply(Q, K, V, _lens(lens_q, K.device, B, "cross_attention"), _lens(lens_k, K.device, B, "cross_attention"), int(n_heads))


def cross_attention_packed(Q, kv, n_heads, lens_q=None, lens_k=None):
    """Same, on one packed projection kv = [K | V] of shape [B, Lk, 2F], read in place; its gradient is dK | dV."""
    _check(Q, kv, None, n_heads, "cross_attention_packed")
    B = kv.shape[0]
    return _XattnFn.apply(Q, kv, None, _lens(lens_q, kv.device, B, "cross_attention_packed"), _lens(lens_k, kv.device, B, "cross_attention_packed"),
                          int(n_heads))


class MultiheadCrossAttention(nn.Module):
    """MHA(X, Y, Y): one Linear for Q, one packed Linear for K|V (the kernels read its two column blocks in place), one output Linear."""

    def __init__(self, hid_dim, n_heads):
        super().__init__()
        if hid_dim % n_heads != 0 or hid_dim // n_heads > MAX_HEAD_DIM:
            raise ValueError(f"hid_dim {hid_dim} must be a multiple of n_heads {n_heads} with a head dimension of at most {MAX_HEAD_DIM}")
        self.hid_dim, self.n_heads = hid_dim, n_heads
        self.w_q = FusedLinear(hid_dim, hid_dim)
        self.w_kv = FusedLinear(hid_dim, 2 * hid_dim)
        self.fc = FusedLinear(hid_dim, hid_dim)

    def forward(self, X, Y, lens_q=None, lens_k=None):
        q = linear(X, self.w_q.weight, self.w_q.bias)
        kv = linear(Y, self.w_kv.weight, self.w_kv.bias)
        return linear(cross_attention_packed(q, kv, self.n_heads, lens_q, lens_k), self.fc.weight, self.fc.bias)


class MAB(nn.Module):
    """Multi-head attention block: H = LN(X + Drop(MHA(X, Y, Y))), output LN(H + Drop(rFF(H)))."""

    def __init__(self, hid_dim, n_heads, dropout=0.1):
        super().__init__()
        self.mha = MultiheadCrossAttention(hid_dim, n_heads)
        self.norm1, self.norm2 = LayerNorm(hid_dim), LayerNorm(hid_dim)
        self.rff = PositionwiseFeedForward(hid_dim, hid_dim=hid_dim, dropout=dropout)
        self.dropout = nn.Dropout(dropout)

    def forward(self, X, Y, lens_q=None, lens_k=None):
        H = self.norm1(X + self.dropout(self.mha(X, Y, lens_q, lens_k)))
        return self.norm2(H + self.dropout(self.rff(H)))


class IMSAB(nn.Module):
    """Induced multi-head self-attention block: forward(X, lens) = MAB(X, MAB(I, X; lens_k = lens); lens_q = lens)."""

    def __init__(self, hid_dim, n_heads, n_induce=32, dropout=0.1):
        super().__init__()
        if not 1 <= n_induce <= MAX_SHORT:
            raise ValueError(f"n_induce = {n_induce}: the rectangular attention kernels hold the short side in LDS, 1 .. {MAX_SHORT} inducing points")
        self.I = nn.Parameter(nn.init.xavier_uniform_(torch.empty(n_induce, hid_dim)))
        self.mab_induce = MAB(hid_dim, n_heads, dropout)
        self.mab_docs = MAB(hid_dim, n_heads, dropout)

    def forward(self, X, lens=None):
        H = self.mab_induce(self.I, X, None, lens)
        return self.mab_docs(X, H, lens, None)


class SetRankEncoder(nn.Module):
    def __init__(self, layer, num_layers):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(num_layers)])
        for l in self.layers:                                 # every layer its own inducing points
            nn.init.xavier_uniform_(l.I)

    def forward(self, x, lens=None):
        for layer in self.layers:
            x = layer(x, lens)
        return x


def build_setrank(num_features=None, ff_dims=[128, 256, 512], n_heads=2, n_induce=32, encoder_layers=3, dropout=0.1, out_dim=1, AF='R',
                  TL_AF='GE', apply_tl_af=False, BN=True, bn_type=None, bn_affine=False, device=None, **_ignored):
    """{'head_ffnns', 'encoder', 'tail_ffnns'} as build_listsf makes them, the encoder a stack of IMSAB layers.  Keys build_listsf takes
    and this scorer has no use for (encoder_type) are ignored."""
    head_ffnns = build_stacked_ffnet([num_features] + list(ff_dims) + [num_features], AF=AF, TL_AF=AF, apply_tl_af=True,
                                     dropout=dropout, BN=BN, bn_type=bn_type, bn_affine=bn_affine, device=device)
    encoder = SetRankEncoder(IMSAB(num_features, n_heads, n_induce=n_induce, dropout=dropout), encoder_layers)
    tail_ffnns = build_stacked_ffnet([num_features] + list(ff_dims) + [out_dim], AF=AF, TL_AF=TL_AF, apply_tl_af=apply_tl_af,
                                     BN=BN, bn_type=bn_type, bn_affine=bn_affine, device=device)
    return {'head_ffnns': head_ffnns, 'encoder': encoder, 'tail_ffnns': tail_ffnns}


def setrank_forward(sf, batch_q_doc_vectors, lens=None):
    """[B, L, num_features] -> scores [B, L]."""
    out = sf['tail_ffnns'](sf['encoder'](sf['head_ffnns'](batch_q_doc_vectors), lens))
    return torch.squeeze(out, dim=2)


class SetRankScorerMixin:
    """Makes a ranker build the SetRank scorer under sf_id = 'listsf' (same three-module dict, so parameters, modes, save and load work as
    for the other listwise scorers) and routes `lens` of padded batches into the attention kernels, as FusedListScorerMixin does."""

    def ini_listsf(self, **kw):
        sf = build_setrank(device=self.device, **kw)
        return {k: m.to(self.device) for k, m in sf.items()} if self.gpu else sf

    def forward(self, batch_q_doc_vectors):
        return setrank_forward(self.list_sf, batch_q_doc_vectors, getattr(self, '_batch_lens', None))


def make_setrank_class(base=None):
    """The SetRank ranker on `base` (anything with the reference's AdhocNeuralRanker interface), made as make_ranker_classes makes the others."""
    from .host import DeviceEvaluator, PointScorerRanker
    from .rankers import DeviceTrainLoop, FusedScorerMixin, ListNetLoss
    base = PointScorerRanker if base is None else base

    class SetRank(ListNetLoss, SetRankScorerMixin, FusedScorerMixin, DeviceTrainLoop, DeviceEvaluator, base):
        """sf_para_dict = {'sf_id': 'listsf', 'opt', 'lr', 'listsf': build_setrank's arguments}; the loss is ListNet's softmax cross-entropy."""

        def __init__(self, sf_para_dict=None, gpu=False, device=None):
            assert 'listsf' == sf_para_dict['sf_id']
            sf_para_dict = copy.deepcopy(sf_para_dict)
            sf_para_dict['listsf'].setdefault('encoder_type', 'SetRank')       # the base reads the key; build_setrank ignores it
            base.__init__(self, id='SetRank', sf_para_dict=sf_para_dict, gpu=gpu, device=device)

    SetRank.__name__ = SetRank.__qualname__ = 'SetRank'
    SetRank.__module__ = __name__
    return SetRank


SetRank = make_setrank_class()
