"""The audit of the boosting metrics and of the stop rule: what train_rmse[], eval_rmse[], rounds_run and best_round of a
boost call must hold, worked out from what the caller gave (rows, labels, weights, the held-out set with its own
`missing`, the metric, the slope, alpha, the starting margins of both sets) and from what the library left (the new
trees of XGBoosterSaveModel's JSON).  Standard library and numpy only; nothing here calls the code under test, and nothing
is imported from the grow_*_support restatements.

Margins.  Every set walks every saved tree by its raw float32 rows: a row steps left when x < split_condition; NaN, the
set's own `missing` and a column the matrix lacks take default_left.  One level a step, all rows at once; pred += leaf is
one float32 add per tree, in tree order.  No bins, no cuts: the header promises that this walk is the partition.

Exact sums.  z = pred - y is one float32 subtraction.  e = rint(z * 2^24) and hq = rint(w * 2^24) are formed in float64,
where the product is exact, and rounded to even; sq is the header's term of the metric; S = sum hq * sq and W = sum hq are
Python integers, whole - no hi/lo words, no P2/P1/P0.  The Eval call (`counted`) has S = sum e^2 over n rows.

The defined value.  float(int) rounds to nearest even, as a conversion from unsigned __int128 does; the scalings are exact:
    counted rmse        sqrt(float(S) * 2^-48 / n)
    rmse                sqrt((float(S) * 2^-72) / (float(W) * 2^-24))
    mae, pseudohuber    (float(S) * 2^-48) / (float(W) * 2^-24)
    quantile            (float(S) * 2^-72) / (float(W) * 2^-24)
The library's entry must equal it bit for bit (check "defined").

The stop rule runs over the exact S of the held-out set: best = 0; after tree t, best = t if S[t] < S[best], strictly;
stop at t - best >= patience where patience >= 1 (check "stop").

The true value takes nothing from the fixed point: with p, y, w the exact rationals of the float32 margins, labels and
weights, z = p - y exactly (fractions.Fraction over integers in units of 2^-149), and in decimal at 100 digits
    rmse          sqrt(sum w z^2 / sum w)
    mae           sum w |z| / sum w
    pseudohuber   sum w delta^2 (sqrt(1 + z^2/delta^2) - 1) / sum w, each term as z^2 / (1 + sqrt(1 + z^2/delta^2)), the
                  same number without the cancellation
    quantile      sum w (z < 0 ? alpha |z| : (1 - alpha) |z|) / sum w, alpha the float32 parameter: docs/32's pinball loss.
The returned double must lie within `bound` of it (check "truth").

The bound, from the roundings the header admits.  u = 2^-24.  Per row r, with zf the float32 residual:
    the subtraction       |zf - z| <= u |zf|                 (half an ulp of zf; the sign of zf is the sign of z)
    e                     |e 2^-24 - zf| <= 2^-25, so with ze = e 2^-24:  |ze - z| <= a_r = 2^-25 + u |zf|
    hq                    |hq 2^-24 - w| <= b = 2^-25        (0 where the call has no weights: hq = 2^24 is w = 1)
    alpha_q               |alpha_q 2^-24 - alpha| <= 2^-25
The term L^_r the library sums (sq scaled back) against the true term L(z_r), |L^_r - L(z_r)| <= eps_r:
    rmse          |ze^2 - z^2| = |ze - z| |ze + z| <= a_r (2 |ze| + a_r)
    mae           ||ze| - |z|| <= a_r
    quantile      c^ the factor used, c the true one, c <= c^ + 2^-25:
                  ||ze| c^ - |z| c| <= |ze| |c^ - c| + c |ze - z| <= |ze| 2^-25 + (c^ + 2^-25) a_r
    pseudohuber   L is Lipschitz: |L'(z)| = |z| / sqrt(1 + z^2/delta^2) <= delta, so |L(zf) - L(z)| <= delta u |zf|.  mf is
                  seven float32 operations on zf (d2, z2, the quotient, 1 +, the root, 1 +, the last quotient); the
                  quotient's three relative errors reach 1 + z2/d2 damped by z2/d2 / (1 + z2/d2) <= 1, the root halves
                  what it is given, so mf = L(zf) (1 + t) with |t| <= 6u + O(u^2) <= 8u; then sq rounds mf 2^24 to a whole
                  number, 2^-25 in mf.  A z2 that underflows has L(zf) < 2^-126 and sq = 0.  With F = (L^_r + 2^-25) / (1 - 8u)
                  an upper bound of L(zf):  eps_r = delta u |zf| + 8u F + 2^-25 + 2^-126
Numerator N = sum w L(z), N^ = sum w^ L^ with w^ = hq 2^-24; denominator D = sum w, D^ = sum w^:
    |N^ - N| <= dN = sum_r ( w^_r eps_r + b (L^_r + eps_r) )        |D^ - D| <= dD = n b
    N^/D^ - N/D = (N^ (D - D^) + D^ (N^ - N)) / (D^ D)   so   |N^/D^ - N/D| <= dM = ((N^/D^) dD + dN) / (D^ - dD)
The root of rmse: |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= |a - b| / sqrt(a), a = N^/D^ (sqrt(dM) at a = 0).
The doubles: two conversions and one division, each within 2^-53 relative, and for rmse a root that halves them and adds
its own: (1 + 2^-53)^3 - 1 < 4 * 2^-53 in either case.  So
    bound = (dM, or dM / sqrt(N^/D^) for rmse) + 4 * 2^-53 * |N^/D^ or its root|
computed in decimal from the audit's own integers.  Nothing in it is tuned, and nothing comes from the code under test.
"""
import decimal
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
METRICS = ("rmse", "mae", "pseudohuber", "quantile")
ONE = 1 << 24
CTX = decimal.Context(prec=100)
D = decimal.Decimal


# ---- the walk and the margins ----

def leaf_values(tree, x, missing, less=np.less, missing_left=None, flip_default=False):
    """The leaf value of every row of x (float32 [n][ncol]) in one tree of the saved JSON (python lists, visits_support.doc_trees).
    `less`, `missing_left` and `flip_default` are for planted faults and for the conditions: another comparison, a missing
    value sent one way whatever its default, a missing value sent against its default."""
    x = np.asarray(x, dtype=F32)
    n, ncol = x.shape
    left, right = np.asarray(tree["left_children"], np.int64), np.asarray(tree["right_children"], np.int64)
    feat, dl = np.asarray(tree["split_indices"], np.int64), np.asarray(tree["default_left"], np.int64) != 0
    cond = np.asarray(tree["split_conditions"], F32)      # the file prints a float32 in nine digits, which round-trip
    if missing_left is not None:
        dl = np.full(len(dl), bool(missing_left))
    if flip_default:
        dl = ~dl
    pos = np.zeros(n, np.int64)
    rows = np.arange(n)
    for _ in range(19):
        rows = rows[left[pos[rows]] >= 0]
        if len(rows) == 0:
            return cond[pos]
        p = pos[rows]
        f = feat[p]
        have = f < ncol
        v = np.where(have, x[rows, np.where(have, f, 0)], F32(np.nan)).astype(F32)
        miss = np.isnan(v)
        if not math.isnan(missing):
            miss |= v == F32(missing)
        with np.errstate(invalid="ignore"):
            go_left = np.where(miss, dl[p], less(v, cond[p]))
        pos[rows] = np.where(go_left, left[p], right[p])
    raise AssertionError("a tree deeper than 18 levels")


def margins(trees, x, missing, start, **planted):
    """[pred_0 .. pred_T], float32: pred_0 = start, pred_t = pred_{t-1} + leaf_t in one float32 add."""
    pred = np.asarray(start, dtype=F32).copy()
    assert pred.shape == (len(x),)
    out = [pred]
    for t in trees:
        pred = pred + leaf_values(t, x, missing, **planted)
        assert pred.dtype == F32
        out.append(pred)
    return out


# ---- the exact sums ----

def residual(pred, y):
    z = np.asarray(pred, F32) - np.asarray(y, F32)
    assert z.dtype == F32 and np.all(np.isfinite(z)) and np.all(np.abs(z) < F32(256.0)), "a residual the call refuses"
    return z


def fixed(v):
    """rint(v * 2^24) of float32 values, to even: the product is exact in float64 -> int64."""
    return np.rint(np.asarray(v, F32).astype(np.float64) * float(ONE)).astype(np.int64)


def weights_fixed(w, n):
    if w is None:
        return np.full(n, ONE, np.int64)
    w = np.asarray(w, F32)
    assert w.shape == (n,) and np.all(np.isfinite(w)) and np.all(w >= 0) and np.all(w < F32(256.0)), "a weight the call refuses"
    return fixed(w)


def alpha_fixed(alpha):
    return int(fixed(F32(alpha)))


def terms(metric, z, slope=1.0, alpha=0.5):
    """sq of every row, as the header words it -> an object array of Python ints."""
    assert metric in METRICS
    z = np.asarray(z, F32)
    if metric == "pseudohuber":
        d = F32(slope)
        with np.errstate(under="ignore"):
            d2 = d * d
            z2 = z * z
            s = np.sqrt(F32(1.0) + z2 / d2)
            mf = z2 / (F32(1.0) + s)
        assert mf.dtype == F32 and isinstance(d2, F32)
        return fixed(mf).astype(object)
    e = np.abs(fixed(z)).astype(object)
    if metric == "rmse":
        return e * e
    if metric == "mae":
        return e
    aq = alpha_fixed(alpha)
    return e * np.where(z < F32(0.0), aq, ONE - aq).astype(object)


def exact_sum(hq, sq=None):
    v = np.asarray(hq).astype(object)
    if sq is not None:
        v = v * sq
    return int(v.sum()) if len(v) else 0


def defined(metric, S, W, counted=False, n=0):
    """The double the header defines from the exact sums."""
    if counted:
        assert metric == "rmse"
        return math.sqrt(float(S) * 2.0 ** -48 / float(n))
    if metric == "rmse":
        return math.sqrt((float(S) * 2.0 ** -72) / (float(W) * 2.0 ** -24))
    return (float(S) * 2.0 ** (-72 if metric == "quantile" else -48)) / (float(W) * 2.0 ** -24)


def stop_rule(S, rounds, patience):
    """(rounds_run, best_round) of the header's rule over the exact held-out sums S[0 ..].  Where S ends before the rule
    does (fewer trees than the rule asks for), rounds_run is None."""
    best = 0
    for t in range(1, rounds + 1):
        if t >= len(S):
            return None, best
        if S[t] < S[best]:
            best = t
        if patience >= 1 and t - best >= patience:
            return t, best
    return rounds, best


# ---- the true value and the bound ----

def _units(v):
    """float32 values as exact integers in units of 2^-149."""
    out = []
    for f in np.asarray(v, F32).tolist():
        n, d = f.as_integer_ratio()
        out.append(n * ((1 << 149) // d))
    return out


def true_value(metric, pred, y, w, slope=1.0, alpha=0.5):
    """The weighted mean of the textbook loss over the exact rationals of the float32 inputs -> Decimal, 100 digits."""
    p, yy = _units(pred), _units(y)
    ww = _units(w) if w is not None else [1 << 149] * len(p)
    zs = [a - b for a, b in zip(p, yy)]
    den = sum(ww)
    unit = 1 << 149
    if metric == "rmse":
        q = Fraction(sum(wi * z * z for wi, z in zip(ww, zs)), den * unit * unit)
        return CTX.sqrt(CTX.divide(D(q.numerator), D(q.denominator)))
    if metric == "mae":
        q = Fraction(sum(wi * abs(z) for wi, z in zip(ww, zs)), den * unit)
        return CTX.divide(D(q.numerator), D(q.denominator))
    if metric == "quantile":
        an, ad = float(F32(alpha)).as_integer_ratio()
        q = Fraction(sum(wi * abs(z) * (an if z < 0 else ad - an) for wi, z in zip(ww, zs)), den * unit * ad)
        return CTX.divide(D(q.numerator), D(q.denominator))
    dn, dd = float(F32(slope)).as_integer_ratio()
    scale = D(unit * unit) * D(dn * dn) / D(dd * dd)             # delta^2 in units of 2^-298, exact
    total = D(0)
    for wi, z in zip(ww, zs):
        z2 = D(z * z)
        s = CTX.sqrt(CTX.add(D(1), CTX.divide(z2, scale)))
        total = CTX.add(total, CTX.multiply(D(wi), CTX.divide(z2, CTX.add(D(1), s))))
    return CTX.divide(total, D(den) * D(unit * unit))


def bound(metric, z, hq, sq, weighted, slope=1.0, alpha=0.5):
    """The module docstring's bound on |defined - true| -> Decimal.  z the float32 residuals, hq and sq the audit's integers.
    The per-row terms are evaluated in float64 and the total is widened by 2^-30 for that."""
    u, half = 2.0 ** -24, 2.0 ** -25
    b = half if weighted else 0.0
    shift = {"rmse": 48, "mae": 24, "pseudohuber": 24, "quantile": 48}[metric]
    azf = np.abs(np.asarray(z, F32).astype(np.float64))
    a = half + u * azf
    ze = np.abs(fixed(z)).astype(np.float64) * u
    L = np.asarray([float(Fraction(int(s), 1 << shift)) for s in sq], np.float64)
    if metric == "rmse":
        eps = a * (2.0 * ze + a)
    elif metric == "mae":
        eps = a
    elif metric == "quantile":
        aq = alpha_fixed(alpha)
        c = np.where(np.asarray(z, F32) < F32(0.0), aq, ONE - aq).astype(np.float64) * u
        eps = ze * half + (c + half) * a
    else:
        eps = float(F32(slope)) * u * azf + 8.0 * u * (L + half) / (1.0 - 8.0 * u) + half + 2.0 ** -126
    wh = np.asarray(hq).astype(np.float64) * u
    dN = Fraction(float(np.sum(wh * eps + b * (L + eps)))) * (1 + Fraction(1, 1 << 30))
    Nh, Dh = Fraction(exact_sum(hq, np.asarray(sq, dtype=object)), 1 << (shift + 24)), Fraction(exact_sum(hq), ONE)
    dD = Fraction(b) * len(azf)
    assert Dh > dD, "weights too small for a bound"
    M = Nh / Dh
    dM = (M * dD + dN) / (Dh - dD)
    to_d = lambda q: CTX.divide(D(q.numerator), D(q.denominator))
    doubles = D(4) / D(1 << 53)
    if metric != "rmse":
        return CTX.add(to_d(dM), CTX.multiply(doubles, to_d(M)))
    if M == 0:
        return CTX.sqrt(to_d(dM))
    root = CTX.sqrt(to_d(M))
    return CTX.add(CTX.divide(to_d(dM), root), CTX.multiply(doubles, root))


# ---- the audit of one call ----

class MetricAudit:
    """train = (x, missing, y, w or None, start); held = the same of the held-out set, or None; trees = the call's new trees
    from the saved JSON.  `counted`: the Eval call, S = sum e^2 over n rows.  truth=False leaves the second reference out
    (long rows).  sums[set][t], W[set], defined[set][t] for t = 0 .. len(trees); true[set][t] and bounds[set][t] with truth."""

    def __init__(self, metric, trees, train, held=None, slope=1.0, alpha=0.5, counted=False, truth=True, sq_metric=None, **planted):
        """sq_metric (a planted fault): the metric whose sq the sums and the defined value take, the true value keeping `metric`."""
        self.metric, self.counted, self.sets = metric, counted, {"train": train}
        self.slope, self.alpha, self.trees, self.sq_metric = slope, alpha, trees, sq_metric or metric
        if held is not None:
            self.sets["eval"] = held
        self.sums, self.W, self.defined, self.true, self.bounds, self.preds = {}, {}, {}, {}, {}, {}
        for name, (x, missing, y, w, start) in self.sets.items():
            assert not counted or w is None
            preds = margins(trees, x, missing, start, **planted)
            hq = self.hq(name)
            self.preds[name], self.W[name] = preds, exact_sum(hq)
            assert self.W[name] > 0, "a set without weight is refused"
            self.sums[name], self.defined[name], self.true[name], self.bounds[name] = [], [], [], []
            for pred in preds:
                z = residual(pred, y)
                sq = terms(self.sq_metric, z, slope, alpha)
                S = exact_sum(hq, sq)
                self.sums[name].append(S)
                self.defined[name].append(defined(self.sq_metric, S, self.W[name], counted, len(y)))
                if truth:
                    self.true[name].append(true_value(metric, pred, y, w, slope, alpha))
                    self.bounds[name].append(bound(metric, z, weights_fixed(w, len(y)), sq, w is not None, slope, alpha))

    def hq(self, name):
        """The integer every row's sq is multiplied by: rint(w * 2^24), or 1 in the call that counts rows."""
        x, missing, y, w, start = self.sets[name]
        return np.ones(len(y), np.int64) if self.counted else weights_fixed(w, len(y))

    @classmethod
    def from_sums(cls, metric, train_sums, train_W, eval_sums, eval_W):
        """An audit of hand-made exact sums: the defined values and the stop rule alone."""
        a = cls.__new__(cls)
        a.metric = a.sq_metric = metric
        a.counted, a.sets = False, {"train": None, "eval": None}
        a.sums, a.W = {"train": list(train_sums), "eval": list(eval_sums)}, {"train": train_W, "eval": eval_W}
        a.defined = {k: [defined(metric, S, a.W[k]) for S in a.sums[k]] for k in a.sums}
        a.true, a.bounds = {"train": [], "eval": []}, {"train": [], "eval": []}
        return a

    def without_row(self, name, t, r, pred=None):
        """The defined value of set `name` after t trees with row r dropped or, with `pred`, at another margin."""
        x, missing, y, w, start = self.sets[name]
        hq = int(self.hq(name)[r])
        one = lambda p: hq * int(terms(self.sq_metric, residual(np.asarray([p], F32), y[r:r + 1]), self.slope, self.alpha)[0])
        S = self.sums[name][t] - one(self.preds[name][t][r])
        if pred is not None:
            return defined(self.sq_metric, S + one(pred), self.W[name], self.counted, len(y))
        return defined(self.sq_metric, S, self.W[name] - hq, self.counted, len(y) - 1)

    def stop(self, rounds, patience):
        if "eval" not in self.sets:
            return rounds, rounds
        return stop_rule(self.sums["eval"], rounds, patience)

    def ratio(self, name, t, value):
        """|value - true| / bound."""
        return float(abs(D(float(value)) - self.true[name][t]) / self.bounds[name][t])

    def violations(self, got, rounds, patience=0):
        """got: the dict of a boost call (train_rmse, eval_rmse, rounds_run, best_round) -> [(check, set, round, got, want)]."""
        out = []
        run = got["rounds_run"]
        for name, key in (("train", "train_rmse"), ("eval", "eval_rmse")):
            if name not in self.sets:
                if got.get(key) is not None:
                    out.append(("defined", name, 0, got[key], None))
                continue
            arr = [float(v) for v in got[key]]
            if len(arr) != run + 1 or run >= len(self.defined[name]):
                out.append(("defined", name, len(arr) - 1, len(arr), min(run, len(self.defined[name]) - 1) + 1))
            for t, v in enumerate(arr[:len(self.defined[name])]):
                want = self.defined[name][t]
                if not (v == want and math.copysign(1.0, v) == math.copysign(1.0, want)):
                    out.append(("defined", name, t, v, want))
                if self.true[name] and not (math.isfinite(v) and abs(D(v) - self.true[name][t]) <= self.bounds[name][t]):
                    out.append(("truth", name, t, v, float(self.true[name][t])))
        want = self.stop(rounds, patience)
        if (run, got["best_round"]) != want:
            out.append(("stop", "eval" if "eval" in self.sets else "train", run, (run, got["best_round"]), want))
        return out


# ---- the cases of the GPU tests ----

KINDS = ("weighted", "sampled", "deep", "deep_sampled")
N, HELD, NFEAT, ROUNDS = 4097, 1300, 4, 3
MISSING = -999.0
SETTINGS = (("rmse", 1.0, 0.5), ("mae", 1.0, 0.5), ("pseudohuber", 0.5, 0.5), ("pseudohuber", 3.7, 0.5), ("quantile", 1.0, 0.05),
            ("quantile", 1.0, 0.95))
# (kind, metric, slope, alpha, form): every kind under every metric, the forms alternating; and the Eval call, which counts rows
CASES = tuple((kind, m, s, a, ("host", "device")[(i + j) % 2]) for i, kind in enumerate(KINDS) for j, (m, s, a) in enumerate(SETTINGS))
CASES += (("eval", "rmse", 1.0, 0.5, "device"),)
STOP_CASES = tuple(("weighted", m, s, a, p) for m, s, a in (SETTINGS[0], SETTINGS[1], SETTINGS[3], SETTINGS[4]) for p in (1, 2, 3))
STOP_CASES += tuple(("deep", "rmse", 1.0, 0.5, p) for p in (1, 2, 3))


def case_id(c):
    kind, metric, slope, alpha, last = c
    return "-".join((kind, metric + {"pseudohuber": "@%g" % slope, "quantile": "@%g" % alpha}.get(metric, ""), str(last)))
