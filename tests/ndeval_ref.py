"""float64 restatement of TREC ndeval 4.4 (the reference's ptranking/metric/srd/ndeval.c), one function per routine of the C file and
operation for operation: Python floats are IEEE doubles and nothing here is fused or reordered, so each function returns the bits the C
program computes (math.log is the C library's log, as in discount()).  tests/golden/make_golden_ndeval.py refuses to write its fixture
unless fields() below reproduces every per-topic field of the program's output string for string.

Data model (the diversity entry points'): rele [T, n] subtopic-by-document judgments, preds [n] scores or None (the input order).  A
"ranking" below is a list of per-document judgment rows (lists of 0 / 1 over the subtopics), top down — ndeval's rl->list[i].rel.
"""
import math

import numpy as np

DEPTH = 20
MEASURES = ("ERR-IA", "nERR-IA", "alpha-DCG", "alpha-nDCG", "NRBP", "nNRBP", "MAP-IA", "P-IA", "strec")
PER_K = ("ERR-IA", "nERR-IA", "alpha-DCG", "alpha-nDCG", "P-IA", "strec")          # the row order of ptr_ndeval_measures' per_k
PER_Q = ("NRBP", "nNRBP", "MAP-IA")                                                # ... and of per_q


def binarise(rele, n=None, nt=None):
    """ndeval.c:908 — any positive judgment is 1.  -> uint8 [n, T'] (document-major), the first n documents and nt subtopics."""
    rele = np.asarray(rele)
    nt = rele.shape[0] if nt is None else max(0, min(int(nt), rele.shape[0]))
    n = rele.shape[1] if n is None else max(0, min(int(n), rele.shape[1]))
    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray((rele[:nt, :n] > 0).T.astype(np.uint8))


def run_order(preds, n):
    """ptr_sort_desc's order of the first n scores: value descending, NaN first, original index ascending (-0.0 ties with +0.0)."""
    if preds is None:
        return np.arange(n)
    p = np.asarray(preds, np.float64)[:n]
    nan = np.isnan(p)
    key = np.where(nan, np.inf, p)
    return np.lexsort((np.arange(n), -key, ~nan))


def nrel_sub(rel):
    """nrelSub[j] (qrelPopulateResultList, :832) as Python ints."""
    return [int(x) for x in rel.sum(axis=0)] if rel.size else [0] * rel.shape[1]


def actual_subtopics(nrelsub):
    """actualSubtopics(), :336-345."""
    return sum(1 for x in nrelsub if x)


def ideal_order(rel, alpha):
    """idealResult(), :351-400 -> the document indices by ideal rank.  Each round scores every remaining document as the sum over its
    subtopics, ascending, of subtopicGain[j]; the largest score wins, a tie goes to the larger docno = the larger index.  (The scores are
    kept between rounds and recomputed — by the same ascending sum — only for the documents that share a subtopic with the last pick;
    once the best score is 0 nothing changes any more and the rest follows by descending index.)"""
    n, T = rel.shape
    gain = [1.0] * T
    relb = rel.astype(bool)
    score = np.zeros(n)
    for j in range(T):
        score = np.where(relb[:, j], score + gain[j], score)
    left = np.ones(n, bool)
    order = []
    for _ in range(n):
        cand = np.where(left, score, -1.0)
        best = cand.max()
        if not best > 0.0:
            break
        where = int(np.nonzero(cand == best)[0][-1])
        order.append(where)
        left[where] = False
        hit = np.zeros(n, bool)
        for j in range(T):
            if relb[where, j]:
                gain[j] *= (1.0 - alpha)
                hit |= relb[:, j]
        idx = np.nonzero(hit & left)[0]
        s = np.zeros(len(idx))
        for j in range(T):
            s = np.where(relb[idx, j], s + gain[j], s)
        score[idx] = s
    order.extend(int(i) for i in np.nonzero(left)[0][::-1])
    return order


def ideal_order_bruteforce(rel, alpha):
    """The same greedy as ndeval writes it: every round rescans every remaining document (quadratic; small pools only).  Also returns,
    per round, the scores of all remaining candidates, for the property test."""
    rel = np.asarray(rel).tolist()
    n, T = len(rel), len(rel[0])
    gain = [1.0] * T
    rank = [0] * n
    order, rounds = [], []
    for r in range(1, n + 1):
        where, max_score = -1, 0.0
        seen = {}
        for i in range(n):
            if rank[i] == 0:
                cur = 0.0
                for j in range(T):
                    if rel[i][j]:
                        cur += gain[j]
                seen[i] = cur
                if where == -1 or cur > max_score or (cur == max_score and i > where):
                    max_score, where = cur, i
        rank[where] = r
        order.append(where)
        rounds.append(seen)
        for j in range(T):
            if rel[where][j]:
                gain[j] *= (1.0 - alpha)
    return order, rounds


def discount(rank):
    """discount(), :567-590."""
    return math.log(2.0) / math.log(rank + 2.0) if rank > 0 else 1.0


def _position_scores(ranking, T, alpha, limit):
    """The loop computeDCG, computeERR and computeNRBP share: score of each of the first `limit` positions."""
    gain = [1.0] * T
    out = []
    for row in ranking[:limit]:
        score = 0.0
        if row is not None:
            for j in range(T):
                if row[j]:
                    score += gain[j]
                    gain[j] *= (1.0 - alpha)
        out.append(score)
    return out


def _ideal_ideal(S, alpha, disc):
    """The "ideal ideal" array of computeDCG / computeERR, cumulated."""
    g = float(S)
    ii = []
    for i in range(DEPTH):
        ii.append(disc(i, g))
        g *= (1.0 - alpha)
    for i in range(1, DEPTH):
        ii[i] += ii[i - 1]
    return ii


def _cumulated(ranking, T, S, alpha, disc):
    out = [0.0] * DEPTH
    if S == 0:
        return out
    for i, s in enumerate(_position_scores(ranking, T, alpha, DEPTH)):
        out[i] = disc(i, s)
    ii = _ideal_ideal(S, alpha, disc)
    for i in range(1, DEPTH):
        out[i] += out[i - 1]
    for i in range(1, DEPTH):                   # from index 1 on only (:641, :696)
        out[i] /= ii[i]
    return out


def compute_err(ranking, T, S, alpha):
    """computeERR(), :597-643."""
    return _cumulated(ranking, T, S, alpha, lambda i, x: x / float(i + 1))


def compute_dcg(ranking, T, S, alpha):
    """computeDCG(), :651-698."""
    return _cumulated(ranking, T, S, alpha, lambda i, x: x * discount(i))


def compute_nrbp(ranking, T, S, alpha, beta):
    """computeNRBP(), :531-562."""
    nrbp = 0.0
    if S == 0:
        return nrbp
    decay = 1.0
    for score in _position_scores(ranking, T, alpha, len(ranking)):
        nrbp += score * decay
        decay *= beta
    nrbp *= (1 - (1 - alpha) * beta) / S
    return nrbp


def compute_map(ranking, T, S, nrelsub):
    """computeMAP(), :484-525 -> MAP-IA."""
    if S == 0:
        return 0.0
    count = [0] * T
    total = [0.0] * T
    for i, row in enumerate(ranking):
        if row is not None:
            for j in range(T):
                if row[j]:
                    count[j] += 1
                    total[j] += count[j] / float(i + 1)
    map_ia = 0.0
    for j in range(T):
        if nrelsub[j]:
            map_ia += total[j] / nrelsub[j]
    return map_ia / S


def compute_strecall(ranking, T, S):
    """computeSTRecall(), :704-730."""
    out = [0.0] * DEPTH
    if S == 0:
        return out
    count, seen = 0, [0] * T
    for i in range(DEPTH):
        if i < len(ranking) and ranking[i] is not None:
            for j in range(T):
                if seen[j] == 0 and ranking[i][j]:
                    count += 1
                    seen[j] = 1
        out[i] = float(count) / float(S)
    return out


def compute_precision(ranking, T, S):
    """computePrecision(), :736-759."""
    out = [0.0] * DEPTH
    if S == 0:
        return out
    count = 0
    for i in range(DEPTH):
        if i < len(ranking) and ranking[i] is not None:
            count += sum(1 for j in range(T) if ranking[i][j])
        out[i] = float(count) / ((i + 1) * S)
    return out


def _div(a, b):
    """C's double division: 0 / 0 is NaN, x / 0 is +-inf."""
    if b == 0.0:
        return float("nan") if a == 0.0 or a != a else math.copysign(float("inf"), a)
    return a / b


def topic(preds, rele, alpha=0.5, beta=0.5, depth=0, n=None, nt=None):
    """One topic through applyQrels() -> dict: the six 20-deep arrays, the three scalars, 'actual_subtopics' and 'ideal_order'."""
    rel = binarise(rele, n, nt)
    n, T = rel.shape
    nrelsub = nrel_sub(rel)
    S = actual_subtopics(nrelsub)
    rows = rel.tolist()
    ideal = ideal_order(rel, alpha)
    iranking = [rows[i] for i in ideal]
    order = [int(i) for i in run_order(preds, n)]
    if depth and depth > 0:
        order = order[:depth]                                   # applyCutoff(), :1000-1020
    ranking = [rows[i] for i in order]
    q_dcg, q_err = compute_dcg(iranking, T, S, alpha), compute_err(iranking, T, S, alpha)
    q_nrbp = compute_nrbp(iranking, T, S, alpha, beta)
    dcg, err = compute_dcg(ranking, T, S, alpha), compute_err(ranking, T, S, alpha)
    nrbp = compute_nrbp(ranking, T, S, alpha, beta)
    ndcg, nerr = [0.0] * DEPTH, [0.0] * DEPTH
    for i in range(DEPTH):                                      # renormalize(), :1143-1156
        if dcg[i]:
            ndcg[i] = dcg[i] / q_dcg[i]
            nerr[i] = err[i] / q_err[i]
    return {"ERR-IA": err, "nERR-IA": nerr, "alpha-DCG": dcg, "alpha-nDCG": ndcg, "NRBP": nrbp, "nNRBP": _div(nrbp, q_nrbp),
            "MAP-IA": compute_map(ranking, T, S, nrelsub), "P-IA": compute_precision(ranking, T, S), "strec": compute_strecall(ranking, T, S),
            "actual_subtopics": S, "ideal_order": ideal}


FIELD_KS = (5, 10, 20)
FIELD_NAMES = tuple([f"{m}@{k}" for m in ("ERR-IA", "nERR-IA", "alpha-DCG", "alpha-nDCG") for k in FIELD_KS] + ["NRBP", "nNRBP", "MAP-IA"] +
                    [f"{m}@{k}" for m in ("P-IA", "strec") for k in FIELD_KS])


def field_values(r):
    """The 21 values of one line of outputMeasures(), :1236-1249, from topic()'s dict."""
    at = lambda m: [r[m][k - 1] for k in FIELD_KS]
    return at("ERR-IA") + at("nERR-IA") + at("alpha-DCG") + at("alpha-nDCG") + [r["NRBP"], r["nNRBP"], r["MAP-IA"]] + at("P-IA") + at("strec")


def fmt(x):
    """printf("%.6f"); a NaN prints as 'nan' or '-nan' by its sign bit, which no test relies on."""
    return "nan" if x != x else "%.6f" % x


def fields(r):
    return [fmt(x) for x in field_values(r)]


def same_field(a, b):
    """Field strings agree; 'nan' and '-nan' are both NaN."""
    return a == b or (a.lstrip("-") == "nan" and b.lstrip("-") == "nan")


def batch(preds, rele, ks=(5, 10, 20), alpha=0.5, beta=0.5, depth=0, lens=None, ntopics=None):
    """What ptr_ndeval_measures returns for a padded batch: per_k float64 [B, 6, nk] (PER_K order), per_q [B, 3] (PER_Q order),
    actual_subtopics int32 [B], ideal_order int32 [B, L] (-1 beyond lens)."""
    rele = np.asarray(rele)
    B, T, L = rele.shape
    per_k, per_q = np.zeros((B, 6, len(ks))), np.zeros((B, 3))
    S, ideal = np.zeros(B, np.int32), np.full((B, L), -1, np.int32)
    for q in range(B):
        n = L if lens is None else max(0, min(int(lens[q]), L))
        nt = T if ntopics is None else int(ntopics[q])
        r = topic(None if preds is None else preds[q], rele[q], alpha, beta, depth, n, nt)
        for a, m in enumerate(PER_K):
            per_k[q, a] = [r[m][k - 1] for k in ks]
        per_q[q] = [r[m] for m in PER_Q]
        S[q] = r["actual_subtopics"]
        ideal[q, :n] = r["ideal_order"]
    return per_k, per_q, S, ideal
