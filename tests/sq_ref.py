"""CPU reference of the IVF_SQ search — test infrastructure only.

Restates, step for step, the canonical numerics of the IVF_SQ index
(duckdb-lancedb_amd/csrc/ivf.h, DESIGN.md "IVF_SQ"); it does for IVF_SQ what
oracle/ivf.py does for IVF_PQ.  Every operation is f32, in the order written,
one rounding per step (no fused multiply-add):

  model   centroids + (lo, hi); s = (hi - lo) / 255 (1 when hi <= lo, or when
          the quotient is not a positive finite number), mid = lo + 128 s
  row     v = x (l2, dot) or x * f32(1 / sqrt(f64 sum x^2)) (cosine: the row
          scale the store keeps); c = clamp(rint((v - lo) / s), 0, 255),
          c' = c - 128; S1 = sum c', S2 = sum c'^2 (exact integers)
          rt = (f32(dim) (mid mid) + ((2 mid) s) f32(S1)) + (s s) f32(S2)
  query   qp = q (cosine: normalize_queries); sq = max|qp| / 127 (0 for a zero
          query); qi = rint(qp / sq)
  key     I = sum qi c' (exact); p = (sq s) f32(I) + (sq mid) f32(sum qi);
          key = rt - 2 p (l2) | -p (dot, cosine); then key + 0 (-0 -> +0)
  search  coarse top-nprobe (oracle.ivf.coarse_probes); per query the k *
          max(1, refine_factor) smallest (key, label ascending) of the live rows
          of the probed lists; the exact top-k of the unindexed tail; the union
          re-ranked exactly by (distance, label under the handle's tie rule).
"""
from __future__ import annotations

import numpy as np

from oracle import flat_knn
from oracle.ivf import _topk_exact, coarse_probes, normalize_queries

F32 = np.float32


def sq_params(lo, hi):
    """(s, mid) of the bounds."""
    lo, hi = F32(lo), F32(hi)
    s = F32(1.0)
    if hi > lo:
        with np.errstate(over="ignore"):
            s = F32(F32(hi - lo) / F32(255.0))
        if not (np.isfinite(s) and s > 0):
            s = F32(1.0)
    mid = F32(lo + F32(F32(128.0) * s))
    return s, mid


def row_values(X, metric):
    """The values that are quantised: x, or x times the stored row scale (cosine)."""
    X = np.asarray(X, F32)
    if flat_knn.normalize_metric(metric) != "cosine":
        return X
    n2 = np.einsum("ij,ij->i", X.astype(np.float64), X.astype(np.float64))
    sc = np.zeros(len(X), F32)
    nz = n2 > 0
    sc[nz] = (1.0 / np.sqrt(n2[nz])).astype(F32)
    return (X * sc[:, None]).astype(F32)


def sq_codes(X, lo, hi, metric="l2"):
    """Unshifted 8-bit codes c [n, dim] (uint8) of the rows X."""
    s, _ = sq_params(lo, hi)
    v = row_values(X, metric)
    t = ((v - F32(lo)).astype(F32) / s).astype(F32)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def row_terms(cp, lo, hi):
    """rt [n] (f32) from the shifted codes c' [n, dim] (int64)."""
    s, mid = sq_params(lo, hi)
    dim = cp.shape[1]
    S1 = cp.sum(1).astype(F32)
    S2 = (cp * cp).sum(1).astype(F32)
    a = F32(F32(dim) * F32(mid * mid))
    b = (F32(F32(F32(2.0) * mid) * s) * S1).astype(F32)
    c = (F32(s * s) * S2).astype(F32)
    return ((a + b).astype(F32) + c).astype(F32)


def query_codes(qp):
    """(qi int64 [dim], sq f32) of one prepared query."""
    qp = np.asarray(qp, F32)
    amax = F32(np.max(np.abs(qp))) if qp.size else F32(0.0)
    sq = F32(amax / F32(127.0))
    if not sq > 0:
        return np.zeros(qp.shape, np.int64), F32(0.0)
    qi = np.clip(np.rint((qp / sq).astype(F32)), -127, 127).astype(np.int64)
    return qi, sq


def sq_keys(cp, rt, qp, lo, hi, metric):
    """SQ keys (f32) of one prepared query against rows with shifted codes cp / row terms rt."""
    s, mid = sq_params(lo, hi)
    qi, sq = query_codes(qp)
    I = (cp @ qi).astype(F32)  # exact: |I| <= 127 * 128 * dim < 2^24 * 2^7; f32(I) rounds once
    a = F32(sq * s)
    b = F32(F32(sq * mid) * F32(qi.sum()))
    p = ((a * I).astype(F32) + b).astype(F32)
    if flat_knn.normalize_metric(metric) == "l2":
        key = (rt - (F32(2.0) * p).astype(F32)).astype(F32)
    else:
        key = (-p).astype(F32)
    return (key + F32(0.0)).astype(F32)


def ivf_sq_search(X, labels, live, lists, C, lo, hi, Q, k, nprobe, rf=1, metric="l2", tie=None):
    """IVF_SQ search.  X / labels / live / lists are per slot (ascending labels;
    lists == -1: not indexed yet).  Returns (labels [nq, k] -1 padded, dists
    [nq, k] NaN padded, counts)."""
    metric = flat_knn.normalize_metric(metric)
    X = np.asarray(X, F32)
    labels = np.asarray(labels, np.int64)
    live = np.asarray(live, bool)
    lists = np.asarray(lists, np.int64)
    Q = np.asarray(Q, F32)
    probes, _ = coarse_probes(C, Q, metric, nprobe)
    Qp = normalize_queries(Q) if metric == "cosine" else Q
    cp = sq_codes(X, lo, hi, metric).astype(np.int64) - 128
    rt = row_terms(cp, lo, hi)
    kk = k * max(1, rf)
    nq = len(Q)
    out_l = np.full((nq, k), -1, np.int64)
    out_d = np.full((nq, k), np.nan, F32)
    cnt = np.zeros(nq, np.int32)
    tail = np.nonzero(live & (lists < 0))[0]
    for i in range(nq):
        rows = np.nonzero(live & np.isin(lists, probes[i]))[0]
        sel = np.zeros(0, np.int64)
        if rows.size:
            key = sq_keys(cp[rows], rt[rows], Qp[i], lo, hi, metric)
            o = flat_knn._order(key, labels[rows], "label_asc")[:kk]
            sel = rows[o]
        ts, _ = _topk_exact(X, labels, tail, Q[i], k, metric, tie)
        allc = np.concatenate([sel, ts])
        s, d = _topk_exact(X, labels, allc, Q[i], k, metric, tie)
        n = len(s)
        out_l[i, :n], out_d[i, :n], cnt[i] = labels[s], d, n
    return out_l, out_d, cnt
