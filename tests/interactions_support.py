"""Shared by the interaction-value tests: float64 references for SHAP interaction values (OHXBoosterPredictInteractions).

Off the diagonal, the Shapley interaction index over the same value function v(S) as contribs_support.brute_force:
    Phi_ik = sum over S in N minus {i, k} of |S|! (M - |S| - 2)! / (2 (M - 1)!) * (v(S+i+k) - v(S+i) - v(S+k) + v(S))
On the diagonal phi_i - sum_{k != i} Phi_ik; row M and column M are 0 but for Phi_MM = phi_M, the bias.
"""
import math

import numpy as np

from tests import contribs_support as cs


def _values(trees, rows, missing, nfeat, ntree_limit):
    use = trees[:ntree_limit] if ntree_limit else trees
    out = []
    for x in rows:
        V = np.zeros(1 << nfeat)
        for t in use:
            V += cs._tree_values(t, x, missing, nfeat)
        out.append(V)
    return out


def _finish(phi, off):
    """The matrix from the contributions phi (nrow, M + 1) and the off-diagonals off (nrow, M, M), float64."""
    n, M = off.shape[0], off.shape[1]
    out = np.zeros((n, M + 1, M + 1))
    out[:, :M, :M] = off
    for i in range(M):
        out[:, i, i] = phi[:, i] - (off[:, i, :].sum(axis=1) - off[:, i, i])
    out[:, M, M] = phi[:, M]
    return out


def brute_force_interactions(trees, base, rows, missing, nfeat, ntree_limit=0):
    """(nrow, nfeat + 1, nfeat + 1) float64 Shapley interaction values over all 2^nfeat subsets (nfeat <= 10)."""
    M = nfeat
    phi = cs.brute_force(trees, base, rows, missing, nfeat, ntree_limit)
    if M < 2:
        return _finish(phi, np.zeros((len(rows), M, M)))
    masks = np.arange(1 << M)
    size = np.array([bin(m).count("1") for m in masks])
    weight = np.array([math.factorial(s) * math.factorial(M - s - 2) / (2 * math.factorial(M - 1)) if s <= M - 2
                       else 0.0 for s in size])
    off = np.zeros((len(rows), M, M))
    for r, V in enumerate(_values(trees, rows, missing, nfeat, ntree_limit)):
        for i in range(M):
            for k in range(M):
                if k == i:
                    continue
                S = masks[(((masks >> i) & 1) == 0) & (((masks >> k) & 1) == 0)]
                grad = V[S | (1 << i) | (1 << k)] - V[S | (1 << i)] - V[S | (1 << k)] + V[S]
                off[r, i, k] = np.sum(weight[S] * grad)
    return _finish(phi, off)


def _unwound(O, Z, d):
    """Per element k of d-element paths (O, Z: (paths, d, n) and (paths, d)): the unwound path sum W(path, k), float64,
    as contribs_support.treeshap64 evaluates it.  Returns (paths, d, n)."""
    dt = np.float64
    pw = np.zeros((d + 1,) + O[:, 0].shape, dt)
    pw[0] = 1
    for k in range(1, d + 1):
        z = Z[:, k - 1, None]; of = O[:, k - 1]
        for i in range(k - 1, -1, -1):
            pw[i + 1] += of * pw[i] * dt((i + 1) / (k + 1))
            pw[i] = z * pw[i] * dt((k - i) / (k + 1))
    W = np.zeros(O.shape, dt)
    for k in range(1, d + 1):
        z = Z[:, k - 1, None]; of = O[:, k - 1]
        zinv = np.divide(1.0, z, out=np.zeros_like(z), where=z != 0)
        nop = pw[d].copy(); tot = np.zeros_like(nop)
        for i in range(d - 1, -1, -1):
            tmp = nop * dt((d + 1) / (i + 1))
            nop = pw[i] - tmp * z * dt((d - i) / (d + 1))
            tot += np.where(of > 0, tmp, pw[i] * zinv * dt((d + 1) / (d - i)))
        W[:, k - 1] = tot
    return W


def interactions64(trees, base, rows, missing, nfeat, chunk=1024, ntree_limit=0):
    """Interaction values in float64, path by path as the kernels evaluate them: for every path holding feature i as
    element c, 1/2 (o_c - z_c) (o_k - z_k) leaf W(path without c, k) into Phi_ik; the diagonal and bias from
    contribs_support.treeshap64.  For boosters too wide for the brute force; checked against it in
    test_interactions_cpu.py."""
    trees = trees[:ntree_limit] if ntree_limit else trees
    dt = np.float64
    phi = cs.treeshap64(trees, base, rows, missing, nfeat)
    rows = cs._full_width(rows, nfeat)
    n = len(rows)
    off = np.zeros((nfeat, nfeat, n), dt)
    miss_all = np.isnan(rows) | (rows == missing)
    by_len = {}
    for t in trees:
        for path, v in cs._paths_of(t):
            by_len.setdefault(len(path), []).append((path, v))
    for d, paths in sorted(by_len.items()):
        if d < 2:
            continue
        for c0 in range(0, len(paths), chunk):
            part = paths[c0:c0 + chunk]
            feat = np.array([[e["f"] for e in p] for p, _ in part])
            lo = np.array([[np.nan if e["lo"] is None else e["lo"] for e in p] for p, _ in part], np.float32)
            hi = np.array([[np.nan if e["hi"] is None else e["hi"] for e in p] for p, _ in part], np.float32)
            bit = np.array([[e["m"] for e in p] for p, _ in part])
            Z = np.array([[e["z"] for e in p] for p, _ in part], dt)
            leaf = np.array([np.float32(v) for _, v in part], dt)
            x = rows.T[feat]
            inside = ~(x < lo[..., None]) & ~(x >= hi[..., None])
            O = np.where(miss_all.T[feat], bit[..., None], inside).astype(dt)
            for c in range(d):
                keep = [j for j in range(d) if j != c]
                W = _unwound(O[:, keep], Z[:, keep], d - 1)
                scale = 0.5 * (O[:, c] - Z[:, c, None]) * leaf[:, None]            # (paths, n)
                contrib = W * (O[:, keep] - Z[:, keep, None]) * scale[:, None]    # (paths, d - 1, n)
                np.add.at(off, (feat[:, c][:, None], feat[:, keep]), contrib)
    return _finish(phi, np.transpose(off, (2, 0, 1)))


def bound(ref, rel=1e-5):
    """rel * (1 + sum_ik |ref_ik|) per row, shaped to broadcast against (nrow, M + 1, M + 1)."""
    return rel * (1.0 + np.abs(ref).sum(axis=(1, 2)))[:, None, None]


def within(got, ref, rel=1e-5):
    """The worst |got - ref| / (rel (1 + sum_ik |ref_ik|)) over the rows."""
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got.astype(np.float64) - ref) / bound(ref, rel)))


def diagonal_f32(off_rows, phi):
    """1.6.0's diagonal in float32 from the returned matrix's off-diagonals and the contributions phi: from 0, for
    k = 0 .. M add phi_i at k == i, else subtract Phi_ik."""
    n, M1, _ = off_rows.shape
    diag = np.zeros((n, M1), np.float32)
    for i in range(M1):
        acc = np.zeros(n, np.float32)
        for k in range(M1):
            acc = (acc + phi[:, i]) if k == i else (acc - off_rows[:, i, k])
        diag[:, i] = acc
    return diag
