"""The ranking-metrics law of include/gatv2_abi.h ("ranking metrics") in numpy: per column one stable sort and counts from searchsorted.
rank_stats is what gat_eval_rank / gat_op_rank_stats must return; brute_force states the same law as an O(n^2) pairwise count (the CPU test
holds the two against each other and against sklearn).

scores [rows][C] float32; exactly one of labels [rows] int / targets [rows][C] float (NaN = missing); mask [rows] or None; ks: the K of
Hits@K.  The result is a dict of per-column arrays — n_pos, n_neg, n_nan (int64), auc_num (uint64), ap, mrr (float64), hits [C][len(ks)]
(int64) — plus the derived auc (NaN where n_pos * n_neg == 0) and hits_at = hits / n_pos (NaN without positives), the keys of
abi.rank_stats_dict.  The two float sums are math.fsum of correctly rounded fp64 terms, divided once by n_pos."""
import math

import numpy as np

EPS52 = 2.0 ** -52


def column_entries(scores, labels, targets, mask, c):
    """(score float32 [n], positive bool [n], n_nan) of the entries of column c that take part; -0.0 folded onto +0.0."""
    scores = np.asarray(scores, np.float32)
    rows = scores.shape[0]
    take = np.ones(rows, bool) if mask is None else np.asarray(mask).astype(bool)
    if targets is not None:
        t = np.asarray(targets, np.float32)[:, c]
        take = take & ~np.isnan(t)
        pos = t > np.float32(0.5)
    else:
        pos = np.asarray(labels) == c
    s = scores[:, c]
    nan = np.isnan(s)
    n_nan = int((take & nan).sum())
    take = take & ~nan
    return s[take] + np.float32(0.0), pos[take], n_nan


def _derived(out, n_ks):
    pn = out["n_pos"].astype(np.float64) * out["n_neg"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["auc"] = np.where(pn > 0, out["auc_num"].astype(np.float64) / (2.0 * pn), np.nan)
        out["hits_at"] = np.where(out["n_pos"][:, None] > 0, out["hits"].astype(np.float64) / out["n_pos"][:, None].astype(np.float64), np.nan)
    return out


def _empty(C, n_ks):
    return dict(n_pos=np.zeros(C, np.int64), n_neg=np.zeros(C, np.int64), n_nan=np.zeros(C, np.int64), auc_num=np.zeros(C, np.uint64),
                ap=np.zeros(C, np.float64), mrr=np.zeros(C, np.float64), hits=np.zeros((C, n_ks), np.int64))


def rank_stats(scores, labels=None, targets=None, mask=None, ks=()):
    assert (labels is None) != (targets is None)
    scores = np.asarray(scores, np.float32)
    C = scores.shape[1]
    ks = [int(k) for k in ks]
    out = _empty(C, len(ks))
    for c in range(C):
        s, pos, out["n_nan"][c] = column_entries(scores, labels, targets, mask, c)
        order = np.argsort(s, kind="stable")             # the one sort of the column
        s, pos = s[order], pos[order]
        neg, ps = s[~pos], s[pos]                        # both ascending
        P, N = len(ps), len(neg)
        out["n_pos"][c], out["n_neg"][c] = P, N
        below = np.searchsorted(neg, ps, "left").astype(np.int64)            # negatives strictly lower
        equal = np.searchsorted(neg, ps, "right").astype(np.int64) - below   # negatives that tie
        above = N - below - equal
        out["auc_num"][c] = int((2 * below + equal).sum())
        if P:
            at_or_above = len(s) - np.searchsorted(s, ps, "left").astype(np.int64)      # entries with score >= s
            tp = P - np.searchsorted(ps, ps, "left").astype(np.int64)                   # positives with score >= s
            out["ap"][c] = math.fsum(tp.astype(np.float64) / at_or_above.astype(np.float64)) / P
            out["mrr"][c] = math.fsum(1.0 / (1.0 + above.astype(np.float64) + 0.5 * equal.astype(np.float64))) / P
        for i, K in enumerate(ks):
            out["hits"][c, i] = P if N < K else int((ps > neg[N - K]).sum())
    return _derived(out, len(ks))


def brute_force(scores, labels=None, targets=None, mask=None, ks=(), chunk=256):
    """The law as pairwise counts: every positive against every entry of its column, in chunks of positives."""
    scores = np.asarray(scores, np.float32)
    C = scores.shape[1]
    ks = [int(k) for k in ks]
    out = _empty(C, len(ks))
    for c in range(C):
        s, pos, out["n_nan"][c] = column_entries(scores, labels, targets, mask, c)
        neg, ps = s[~pos], s[pos]
        P, N = len(ps), len(neg)
        out["n_pos"][c], out["n_neg"][c] = P, N
        auc, ap_terms, mrr_terms = 0, [], []
        for i in range(0, P, chunk):
            p = ps[i:i + chunk, None]
            lower = (neg[None, :] < p).sum(1).astype(np.int64)
            equal = (neg[None, :] == p).sum(1).astype(np.int64)
            higher = (neg[None, :] > p).sum(1).astype(np.int64)
            assert np.all(lower + equal + higher == N)
            tp = (ps[None, :] >= p).sum(1).astype(np.int64)
            fp = equal + higher
            auc += int((2 * lower + equal).sum())
            ap_terms += list(tp.astype(np.float64) / (tp + fp).astype(np.float64))
            mrr_terms += list(1.0 / (1.0 + higher.astype(np.float64) + 0.5 * equal.astype(np.float64)))
        out["auc_num"][c] = auc
        if P:
            out["ap"][c] = math.fsum(ap_terms) / P
            out["mrr"][c] = math.fsum(mrr_terms) / P
        top = np.sort(neg)[::-1]
        for i, K in enumerate(ks):
            out["hits"][c, i] = P if N < K else int((ps > top[K - 1]).sum())
    return _derived(out, len(ks))


INT_KEYS = ("n_pos", "n_neg", "n_nan", "auc_num", "hits")


def assert_same(got, want, what=""):
    """The seam's bars: integers exact, ap and mrr within (n_pos + 2) * 2^-52 relative (each term is one fp64 division in (0, 1], and a
    sum of n such terms in any order errs by at most n * 2^-53 of itself; the reference's own sum is exact up to one rounding and one
    division)."""
    for k in INT_KEYS:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), (what, k, got[k], want[k])
    for k in ("ap", "mrr"):
        bar = (np.asarray(want["n_pos"], np.float64) + 2.0) * EPS52 * np.abs(want[k])
        err = np.abs(np.asarray(got[k], np.float64) - want[k])
        assert np.all(err <= bar), (what, k, got[k], want[k], err, bar)
        assert np.all(np.asarray(got[k])[np.asarray(want["n_pos"]) == 0] == 0.0), (what, k)
