"""Every device group-by path (csrc/kernels/relops.hip: hash_aggregate LOW / MID / PART and the clustered-key
run_aggregate, execution/kernels.py group_reduce) against an exact NumPy oracle.

* min / max of doubles: IEEE totalOrder of the bit patterns (-NaN < -inf < -0.0 < +0.0 < +inf < +NaN, a NaN is a
  value), compared bit for bit, so NaN sign and payload count.
* int64 min / max / sum: exact, the sum modulo 2**64.
* float64 sum: long-double reference. A group with non-finite members is decided by class (any NaN or both
  infinities: NaN; else its infinity). A group of c finite rows may err by gamma(c - 1) * S (any summation order;
  gamma(k) = k u / (1 - k u), u = 2**-53, S = sum |x|) plus c * 2**-63 * S for the reference's own rounding, which
  makes a one-row group exact. Two data families must be bit-exact in any order and so see a lost or doubled row:
  integer-valued doubles (|v| <= 2**20, groups of at most 2**20 rows: every partial sum is below 2**53) and
  subnormals whose total stays subnormal. A zero sum is +0.0 on every path.

Every GPU case is sized to the smallest shape that reaches its path and asserts the path from the status words; the
table sizes are those of relops_bind.cpp::hash_aggregate (mirrored in `_sizes`). Data comes from
np.random.default_rng seeded from the case id alone."""
import math
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

from netsdb_amd import _ext
from netsdb_amd.execution import kernels as K

DEV = "cuda:0"
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
MAG = np.int64(0x7FFF_FFFF_FFFF_FFFF)
U = 2.0 ** -53
LD = np.longdouble
LD_OK = np.finfo(LD).nmant >= 63          # else the sums fall back to math.fsum per group
# the reference's own rounding, relative to S: c * 2**-63 for a long-double running sum, one double rounding for fsum
ORACLE_EPS = 2.0 ** -63 if LD_OK else 2.0 ** -53


def _f64(*bits):
    return np.array(bits, dtype=np.uint64).view(np.float64)


NANS = _f64(0x7FF8000000000000, 0xFFF8000000000000, 0x7FF800000000BEEF, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF)
# +-0.0, +-inf, +-quiet NaN, a NaN with a payload, the two NaNs at the ends of the total order (their images are the
# min / max accumulators' identities), +-smallest subnormal, +-DBL_MAX, +-1.5
F64_POOL = np.concatenate([_f64(0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000), NANS,
                           np.array([5e-324, -5e-324, np.finfo(np.float64).max, -np.finfo(np.float64).max, 1.5, -1.5])])
F32_POOL = np.concatenate([np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
                                     0x7FC01234, 0x00000001, 0x80000001], dtype=np.uint32).view(np.float32),
                           np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max, 1.5, -1.5], np.float32)])
I64_POOL = np.array([I64_MIN, I64_MAX, -1, 0], dtype=np.int64)
SPECIAL_KEYS = [I64_MIN, I64_MAX, -1, 0]   # I64_MIN is the kernels' empty-slot marker


# ------------------------------------------------------------------------------------------------ the oracle
def _image(bits):
    """int64 bits of doubles -> the signed integers ordered like totalOrder (an involution; pipeline.py::_merge)."""
    return np.where(bits >= 0, bits, bits ^ MAG)


Groups = namedtuple("Groups", "keys count first inv agg S cls nfin")


def _group_sums(x, heads):
    """Per-group column sums of finite float64 rows x [n, F] (group starts `heads`), as long doubles."""
    if LD_OK:
        return np.add.reduceat(x.astype(LD), heads, axis=0)
    ends = list(heads[1:]) + [x.shape[0]]
    return np.array([[math.fsum(x[a:e, f].tolist()) for f in range(x.shape[1])] for a, e in zip(heads, ends)],
                    dtype=LD).reshape(len(heads), x.shape[1])


def oracle_groupby(keys, vals, op):
    """Group host rows by int64 key. Per distinct key in ascending order: the key, row count and smallest row index;
    the per-row inverse; and the aggregates of vals [n, F] (None: counts only):
      int64: exact min / max / sum (the sum modulo 2**64);
      float64 min / max: by totalOrder of the bits (returned as float64, compare the int64 views);
      float64 sum: `agg` the long-double sum of the group's finite rows, `S` the sum of their magnitudes, `nfin`
      their number, `cls` 0 finite / 1 sums to +inf / 2 to -inf / 3 to NaN (any NaN, or both infinities)."""
    keys = np.asarray(keys, dtype=np.int64)
    n = keys.size
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    heads = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    count = np.diff(np.concatenate([heads, [n]]))
    inv = np.empty(n, dtype=np.int64)
    inv[order] = np.repeat(np.arange(heads.size), count)
    agg = S = cls = nfin = None
    if vals is not None and vals.shape[1] > 0:
        vs = vals[order]
        if vals.dtype == np.int64:
            if op == "sum":
                agg = np.add.reduceat(vs.view(np.uint64), heads, axis=0).view(np.int64)
            else:
                agg = (np.minimum if op == "min" else np.maximum).reduceat(vs, heads, axis=0)
        elif op != "sum":
            img = _image(vs.view(np.int64))
            agg = _image((np.minimum if op == "min" else np.maximum).reduceat(img, heads, axis=0)).view(np.float64)
        else:
            fin = np.isfinite(vs)
            x = np.where(fin, vs, 0.0)
            agg = _group_sums(x, heads)
            S = _group_sums(np.abs(x), heads)
            nfin = np.add.reduceat(fin.astype(np.int64), heads, axis=0)
            nan = np.logical_or.reduceat(np.isnan(vs), heads, axis=0)
            pinf = np.logical_or.reduceat(vs == np.inf, heads, axis=0)
            ninf = np.logical_or.reduceat(vs == -np.inf, heads, axis=0)
            cls = np.where(nan | (pinf & ninf), 3, np.where(pinf, 1, np.where(ninf, 2, 0)))
    return Groups(ks[heads], count, order[heads], inv, agg, S, cls, nfin)


def sum_bound(c, S):
    """Allowed |device - reference| of a float64 sum of c finite rows with magnitude sum S (module docstring)."""
    k = np.maximum(c - 1, 0).astype(LD) * LD(U)
    return (k / (1 - k) + c.astype(LD) * LD(ORACLE_EPS)) * S


def _first_bad(ok):
    return tuple(int(i) for i in np.argwhere(~ok)[0])


def check_bits(dev, ref, what):
    """Bit-for-bit equality of two 8-byte arrays."""
    assert dev.shape == ref.shape and dev.dtype == ref.dtype, (what, dev.shape, ref.shape, dev.dtype, ref.dtype)
    d, r = dev.view(np.int64), ref.view(np.int64)
    ok = d == r
    if not ok.all():
        i = _first_bad(ok)
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} differ; first at {i}: device {dev[i]!r} "
                             f"({int(d[i]) & (2**64 - 1):#018x}), oracle {ref[i]!r} ({int(r[i]) & (2**64 - 1):#018x})")


def check_f64_sums(dev, o, exact_cols, what):
    """Device float64 sums [g, F] (oracle group order) against the oracle's classes, bound and exact families."""
    assert dev.shape == o.agg.shape and dev.dtype == np.float64, (what, dev.shape, dev.dtype)
    assert np.isnan(dev[o.cls == 3]).all(), f"{what}: a NaN-class group is not NaN"
    assert (dev[o.cls == 1] == np.inf).all() and (dev[o.cls == 2] == -np.inf).all(), f"{what}: infinite-class group"
    fin = o.cls == 0
    assert np.isfinite(dev[fin]).all(), f"{what}: a finite group summed to a non-finite value"
    err = np.abs(np.where(fin, dev, 0.0).astype(LD) - o.agg)
    bound = sum_bound(o.nfin, o.S)
    ok = ~fin | (err <= bound)
    if not ok.all():
        i = _first_bad(ok)
        raise AssertionError(f"{what}: {int((~ok).sum())} sums outside the bound; first at {i}: device {dev[i]!r}, "
                             f"oracle {o.agg[i]!r}, err {err[i]!r} > bound {bound[i]!r} ({int(o.nfin[i])} rows)")
    zero = dev == 0
    assert not np.signbit(dev[zero]).any(), f"{what}: a zero sum is -0.0"
    for f in exact_cols:
        assert fin[:, f].all()
        check_bits(dev[:, f], o.agg[:, f].astype(np.float64) + 0.0, f"{what} exact column {f}")


# ------------------------------------------------------------------------------------------------ data
def _rng(case_id):
    return np.random.default_rng(zlib.crc32(case_id.encode()))


def distinct_keys(rng, k):
    """k distinct int64 keys over the whole range; the first min(k, 4) are I64_MIN, I64_MAX, -1, 0."""
    head = SPECIAL_KEYS[:k]
    out = np.empty(0, dtype=np.int64)
    while out.size < k - len(head):
        draw = rng.integers(I64_MIN, I64_MAX, size=k + 64, dtype=np.int64, endpoint=True)
        out = np.unique(np.concatenate([out, draw[~np.isin(draw, SPECIAL_KEYS)]]))
    return np.concatenate([np.array(head, dtype=np.int64), rng.permutation(out)[:k - len(head)]])


def make_keys(rng, n, family, k):
    """equal: one key (I64_MIN) on every row; distinct: n keys; uniform: min(k, n) keys, each at least once; random:
    rows drawn from min(k, n) keys (about 63 % of them occur when k is n, in groups of 1 to a few rows); skew: one
    key on at least 90 % of the rows, the other min(k, n) - 1 keys (the special ones among them) once each."""
    if family == "equal":
        return np.full(n, I64_MIN, dtype=np.int64)
    if family == "distinct":
        return rng.permutation(distinct_keys(rng, n))
    k = min(k, n)
    pool = distinct_keys(rng, k)
    if family == "random":      # k candidate keys drawn with replacement: only the special ones are sure to occur
        keys = pool[rng.integers(0, k, n)]
        keys[:4] = pool[:4]
    elif family == "uniform":
        keys = pool[rng.integers(0, k, n)]
        keys[:k] = pool
    else:
        assert family == "skew"
        singles = min(k - 1, n - (9 * n + 9) // 10)
        keys = np.concatenate([np.full(n - singles, pool[k - 1]), pool[:singles]])
    return rng.permutation(keys)


def f64_minmax_vals(rng, ginv, F):
    """Rows from F64_POOL; in each column a fifth of the groups is all-NaN and a fifth holds only (both) zeros."""
    n = ginv.size
    v = F64_POOL[rng.integers(0, F64_POOL.size, (n, F))]
    for f in range(F):
        sel = (ginv + f) % 5
        v[sel == 0, f] = NANS[rng.integers(0, NANS.size, int((sel == 0).sum()))]
        z = np.flatnonzero(sel == 1)
        v[z, f] = np.where(rng.integers(0, 2, z.size) == 0, 0.0, -0.0)
    return v


SUM_KINDS = ("nonfinite", "int", "sub", "mixed")
EXACT_KINDS = ("int", "sub")


def f64_sum_col(rng, ginv, kind):
    n = ginv.size
    if kind in EXACT_KINDS:
        m = rng.integers(-(1 << 20), 1 << 20, n, endpoint=True).astype(np.float64)
        return m if kind == "int" else m * 5e-324        # an integer multiple of the smallest subnormal: exact
    v = np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0) * (1.0 + rng.random(n)) * 2.0 ** rng.integers(-30, 30, n,
                                                                                                     endpoint=True)
    if kind == "nonfinite":   # groups by class: +inf, -inf, both, a NaN, all -0.0, finite
        _, first = np.unique(ginv, return_index=True)
        cls = np.arange(first.size) % 6
        v[cls[ginv] == 4] = -0.0
        v[first[cls == 0]] = np.inf
        v[first[cls == 1]] = -np.inf
        v[first[cls == 3]] = NANS[rng.integers(0, NANS.size, int((cls == 3).sum()))]
        both = first[cls == 2]
        v[both] = np.inf
        last = np.full(first.size, -1)
        last[ginv] = np.arange(n)                         # the last row of each group
        v[last[cls == 2]] = np.where(last[cls == 2] == both, np.inf, -np.inf)   # (a one-row group keeps +inf)
    return v


def sum_kinds(F):
    """The float64 sum family of each column: F = 1 the non-finite classes, F = 2 the two exact families, more
    columns rotate through all four."""
    return ["nonfinite"] if F == 1 else ["int", "sub"] if F == 2 else [SUM_KINDS[f % 4] for f in range(F)]


def make_vals(rng, keys, F, dtype, op):
    """(vals [n, F] or None, exact float64 sum columns)."""
    if F == 0:
        return None, []
    n = keys.size
    if dtype == "i64":
        v = rng.integers(I64_MIN, I64_MAX, (n, F), dtype=np.int64, endpoint=True)   # sums of these wrap
        sp = rng.random((n, F)) < 0.3
        v[sp] = I64_POOL[rng.integers(0, 4, int(sp.sum()))]
        return v, []
    ginv = np.unique(keys, return_inverse=True)[1].reshape(-1)
    if op != "sum":
        return f64_minmax_vals(rng, ginv, F), []
    kinds = sum_kinds(F)
    v = np.stack([f64_sum_col(rng, ginv, kd) for kd in kinds], axis=1)
    return v, [f for f, kd in enumerate(kinds) if kd in EXACT_KINDS]


def to_device(vals, layout):
    if vals is None:
        return None
    if layout == "col":   # the transpose of a contiguous [F, n] stack: read in place through its strides
        return torch.from_numpy(np.ascontiguousarray(vals.T)).to(DEV).t()
    return torch.from_numpy(np.ascontiguousarray(vals)).to(DEV)


def check_aggs(dev, o, op, dtype, exact_cols, what):
    if dtype == "i64" or op != "sum":
        check_bits(dev, o.agg, what)
    else:
        check_f64_sums(dev, o, exact_cols, what)


# ------------------------------------------------------------------------------------------------ CPU: the oracle
def _total_less(a, b):
    """totalOrder(a, b) and a != b, from the definition: negative below positive, then by magnitude bits."""
    (ba,), (bb,) = np.array([a]).view(np.uint64).tolist(), np.array([b]).view(np.uint64).tolist()
    sa, sb, ma, mb = ba >> 63, bb >> 63, ba & int(MAG), bb & int(MAG)
    if sa != sb:
        return sa == 1
    return ma > mb if sa else ma < mb


def _brute(keys, vals, op, is_int):
    groups = {}
    for i, k in enumerate(keys.tolist()):
        groups.setdefault(k, []).append(i)
    out = []
    for k in sorted(groups):
        rows = groups[k]
        aggs = []
        for f in range(vals.shape[1]):
            xs = [vals[i, f] for i in rows]
            if is_int:
                t = sum(int(x) for x in xs) if op == "sum" else (min(xs) if op == "min" else max(xs))
                aggs.append(((int(t) + (1 << 63)) % (1 << 64)) - (1 << 63))
            elif op == "sum":
                fin = [float(x) for x in xs if math.isfinite(x)]
                nan = any(math.isnan(x) for x in xs) or (any(x == math.inf for x in xs) and
                                                         any(x == -math.inf for x in xs))
                cls = 3 if nan else 1 if any(x == math.inf for x in xs) else 2 if any(x == -math.inf for x in xs) else 0
                aggs.append((math.fsum(fin), math.fsum(abs(x) for x in fin), len(fin), cls))
            else:
                best = xs[0]
                for x in xs[1:]:
                    if (_total_less(x, best) if op == "min" else _total_less(best, x)):
                        best = x
                aggs.append(best)
        out.append((k, len(rows), rows[0], aggs))
    return out


@pytest.mark.parametrize("dtype", ["f64", "i64"])
@pytest.mark.parametrize("op", ["sum", "min", "max"])
def test_oracle_matches_brute_force(op, dtype):
    """oracle_groupby against a Python dict with math.fsum and an explicit totalOrder compare: 200 rows from the
    special-value pools, all float64 sum families, with I64_MIN / I64_MAX / -1 / 0 among the keys."""
    rng = _rng(f"oracle-{op}-{dtype}")
    keys = make_keys(rng, 200, "uniform", 12)
    vals, exact = make_vals(rng, keys, 4, dtype, op)
    o = oracle_groupby(keys, vals, op)
    ref = _brute(keys, vals, op, dtype == "i64")
    assert o.keys.tolist() == [r[0] for r in ref] and set(SPECIAL_KEYS) <= set(o.keys.tolist())
    assert o.count.tolist() == [r[1] for r in ref] and o.first.tolist() == [r[2] for r in ref]
    assert np.array_equal(o.keys[o.inv], keys)
    for g, (_, _, _, aggs) in enumerate(ref):
        for f, a in enumerate(aggs):
            if dtype == "i64":
                assert int(o.agg[g, f]) == a
            elif op != "sum":
                assert np.array([o.agg[g, f]]).view(np.int64)[0] == np.array([a]).view(np.int64)[0], (g, f)
            else:
                tot, mag, c, cls = a
                assert (int(o.cls[g, f]), int(o.nfin[g, f])) == (cls, c)
                assert abs(o.S[g, f] - LD(mag)) <= LD(U) * LD(mag) + c * LD(ORACLE_EPS) * o.S[g, f]
                assert abs(o.agg[g, f] - LD(tot)) <= LD(U) * abs(LD(tot)) + c * LD(ORACLE_EPS) * o.S[g, f]
                if f in exact:
                    assert float(o.agg[g, f]) == tot
    if dtype == "f64" and op == "sum":
        assert exact == [1, 2] and set(o.cls[:, 0].tolist()) == {0, 1, 2, 3}
        assert ((o.S[:, 0] == 0) & (o.cls[:, 0] == 0)).any()          # an all -0.0 group
    if dtype == "f64" and op != "sum":
        allnan = np.array([np.isnan(vals[o.inv == g, 0]).all() for g in range(o.keys.size)])
        assert allnan.any() and np.isnan(o.agg[allnan, 0]).all()


def test_oracle_total_order_and_bound():
    """The order the oracle promises, on the pool itself; the bound is zero-width only for a single row."""
    v = F64_POOL.reshape(-1, 1)
    keys = np.zeros(v.shape[0], dtype=np.int64)
    lo, hi = oracle_groupby(keys, v, "min").agg, oracle_groupby(keys, v, "max").agg
    assert lo.view(np.uint64)[0, 0] == 0xFFFFFFFFFFFFFFFF and hi.view(np.uint64)[0, 0] == 0x7FFFFFFFFFFFFFFF
    z = np.array([[0.0], [-0.0]])
    assert np.signbit(oracle_groupby(keys[:2], z, "min").agg[0, 0])
    assert not np.signbit(oracle_groupby(keys[:2], z, "max").agg[0, 0])
    one = np.array([[1.0], [np.nan]])
    assert oracle_groupby(keys[:2], one, "min").agg[0, 0] == 1.0
    assert np.isnan(oracle_groupby(keys[:2], one, "max").agg[0, 0])
    b = sum_bound(np.array([1, 2, 1 << 20]), np.array([1.0, 1.0, 1.0], dtype=LD))
    assert b[0] <= 2.0 ** -63 and 2.0 ** -53 <= b[1] <= 2.0 ** -52 and b[2] <= 2.0 ** -32
    # wrapping integer sum
    w = oracle_groupby(keys[:2], np.array([[I64_MAX], [1]], dtype=np.int64), "sum").agg
    assert int(w[0, 0]) == I64_MIN


# ------------------------------------------------------------------------------------------------ GPU: hash paths
def _p2_at_most(x):
    return 1 << (int(x).bit_length() - 1)


Sizes = namedtuple("Sizes", "lcap_low lcap_part lcap_mid gcap_low low_thr pbits")


def _sizes(n, F, thr):
    """The table sizes hash_aggregate (relops_bind.cpp) derives for n rows, F columns and low_threshold thr."""
    entry = 20 + 8 * F
    lcap_low = min(1024, _p2_at_most(65536 // entry))
    lcap_part = min(4096, _p2_at_most(131072 // entry))
    lcap_mid = min(4096, _p2_at_most(160 * 1024 // entry)) if thr <= 0 else 0
    pbits = 0
    while pbits < 8 and (n >> (pbits + 1)) >= 2048:
        pbits += 1
    low_thr = thr if thr > 0 else lcap_low // 4
    return Sizes(lcap_low, lcap_part, lcap_mid, max(4 * lcap_low, 8 * lcap_mid), low_thr, pbits)


# name -> (low_threshold, n, key family, distinct keys (by F), path, PART: pbits and whether the one bucket is split)
Shape = namedtuple("Shape", "thr n family k path pbits split")
SHAPES = {
    "low1": Shape(100_000, 1, "distinct", lambda F: 1, "LOW", None, None),
    "low63": Shape(100_000, 63, "uniform", lambda F: 40, "LOW", None, None),
    "low64": Shape(100_000, 64, "equal", lambda F: 1, "LOW", None, None),
    "low65": Shape(100_000, 65, "skew", lambda F: 40, "LOW", None, None),
    "low1023": Shape(100_000, 1023, "uniform", lambda F: 40, "LOW", None, None),
    "low1025": Shape(100_000, 1025, "skew", lambda F: 40, "LOW", None, None),
    "low4097": Shape(100_000, 4097, "uniform", lambda F: 40, "LOW", None, None),
    # the LOW global table (4 * lcap_low slots) gives up past half full: 4 * 256 at F = 16, 4 * 1024 at F <= 2
    "lowfail": Shape(100_000, 3000, "uniform", lambda F: 700 if F == 16 else 2300, "LOWFAIL", 0, None),
    "mid": Shape(0, 20_000, "uniform", lambda F: 700 if F == 16 else 1500, "MID", None, None),
    # one key on 90 % of the rows: the sample sees the other keys once each, estimates n groups and takes PART
    "partskew": Shape(0, 20_000, "skew", lambda F: 1500, "PART", 3, None),
    "part0d": Shape(1, 1000, "uniform", lambda F: 100, "PART", 0, False),
    "part0s": Shape(1, 4095, "uniform", lambda F: 3000, "PART", 0, True),
    "part0all": Shape(1, 4095, "distinct", lambda F: 4095, "PART", 0, True),
    "part1": Shape(1, 4101, "uniform", lambda F: 600, "PART", 1, None),
    "part8": Shape(1, 2 ** 19 + 3, "random", lambda F: 2 ** 19, "PART", 8, True),
    "partauto": Shape(0, 40_000, "uniform", lambda F: 30_000, "PART", 4, None),
}
Case = namedtuple("Case", "shape F dtype op layout want_inv want_first")


def _case_id(c):
    return (f"{c.shape}-F{c.F}-{c.dtype}-{c.op}-{c.layout}-" + ("inv" if c.want_inv else "noinv") +
            ("-first" if c.want_first else "-nofirst"))


def _hash_cases():
    cases = []
    full = ["low1", "low63", "low64", "low65", "low1023", "low1025", "low4097", "mid", "part0d", "part0s", "partauto"]
    for s in full:        # every path: F = 1 and 16, both dtypes, every op
        for F in (1, 16) + ((2,) if s == "mid" else ()):
            for dtype in ("f64", "i64"):
                for op in ("sum", "min", "max"):
                    cases.append(Case(s, F, dtype, op, "row", True, True))
    for dtype in ("f64", "i64"):
        for op in ("sum", "min", "max"):
            cases.append(Case("lowfail", 16, dtype, op, "row", True, True))
            cases.append(Case("part1", 2, dtype, op, "row", True, True))
    cases.append(Case("part8", 2, "f64", "sum", "row", True, True))
    # crossings: counts only, column-major values, the four (want_inv, want_first) combinations, other key families
    flags = [(True, True), (True, False), (False, True), (False, False)]
    ops3 = ("sum", "min", "max", "sum")
    for j, s in enumerate(["low1025", "low4097", "lowfail", "mid", "partskew", "part0d", "part0s", "part0all", "part1",
                           "partauto"]):
        cases.append(Case(s, 0, "i64", "sum", "row", True, True))
        for i, (wi, wf) in enumerate(flags):
            cases.append(Case(s, 2, ("f64", "i64")[(i + j) % 2], ops3[(i + j) % 4], ("col", "row")[i % 2], wi, wf))
        cases.append(Case(s, 16, "f64", ("min", "max", "sum")[j % 3], "col", False, True))
        cases.append(Case(s, 16, "i64", ("sum", "min", "max")[j % 3], "col", True, False))
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def _assert_path(shape, F, st, n):
    """The path a case claims, from the status words [groups, path, ok, sample estimate, scratch bytes]."""
    g, path, ok, est = st[0], st[1], st[2], st[3]
    z = _sizes(n, F, shape.thr)
    assert ok == 1, st
    mid_p = -(-est // (z.lcap_mid // 2)) if z.lcap_mid else None     # MID key partitions asked for (at most 3 run)
    if shape.path == "LOW":
        assert path == 0 and est <= z.low_thr and g <= 40, (st, z)
    elif shape.path == "LOWFAIL":     # the sample chose LOW, its global table overflowed, PART reran the rows
        assert path == 1 and est <= z.low_thr and g > z.gcap_low // 2, (st, z)
    elif shape.path == "MID":
        assert path == 0 and est > z.low_thr and mid_p <= 3 and g > z.lcap_low // 4, (st, z)
    else:
        assert path == 1 and est > z.low_thr and (mid_p is None or mid_p > 3), (st, z)
    if shape.pbits is not None:
        assert z.pbits == shape.pbits, z
    if shape.split is not None:       # agg_bucket_kernel: the bucket's share of the estimate against its LDS table
        share = (5 * (-(-est // (1 << z.pbits)))) // 4 + 16
        rows = n if z.pbits == 0 else 7 * (n >> z.pbits) // 8      # a bucket of the hash holds over 7/8 of the mean
        assert (4 * min(rows, share) > 3 * z.lcap_part) == shape.split, (st, z)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _hash_cases(), ids=_case_id)
def test_hash_aggregate_oracle(case):
    """One hash_aggregate call per case (SHAPES x value columns, dtype, op, layout, inverse / first-row flags): the
    path it claims, then keys, counts, first rows, the inverse and every aggregate against the oracle."""
    cid = _case_id(case)
    shape = SHAPES[case.shape]
    rng = _rng(cid)
    keys = make_keys(rng, shape.n, shape.family, shape.k(case.F))
    vals, exact = make_vals(rng, keys, case.F, case.dtype, case.op)
    o = oracle_groupby(keys, vals, case.op)
    kt = torch.from_numpy(keys).to(DEV)
    r = _ext.hip().hash_aggregate(kt, to_device(vals, case.layout), case.op, case.want_inv, shape.thr, case.want_first)
    st = r[5].tolist()
    _assert_path(shape, case.F, st, shape.n)
    reps, aggs, cnt, first, inv = (t.cpu().numpy() for t in r[:5])
    g = o.keys.size
    assert st[0] == g == reps.size == cnt.size and aggs.shape == (g, case.F)
    order = np.argsort(reps, kind="stable")
    assert np.array_equal(reps[order], o.keys), "group keys"
    assert np.array_equal(cnt[order], o.count), "row counts"
    if case.want_first:
        assert np.array_equal(first[order], o.first), "first rows"
    if case.want_inv:
        assert inv.shape == (shape.n,) and inv.min() >= 0 and inv.max() < g
        assert np.array_equal(reps[inv], keys), "reps[inv] == keys"
    else:
        assert inv.size == 0
    if case.F:
        want = np.float64 if case.dtype == "f64" else np.int64
        assert aggs.dtype == want
        check_aggs(aggs[order], o, case.op, case.dtype, exact, cid)


# ------------------------------------------------------------------------------------------------ GPU: run path
def run_keys(rng, n, layout):
    """Non-descending keys: one run, n runs, or runs of 1 to 8 rows with one run across every 8192-row tile edge."""
    if layout == "onerun":
        return np.full(n, I64_MIN, dtype=np.int64)
    if layout == "distinct":
        return np.sort(distinct_keys(rng, n))
    gid = np.repeat(np.arange(n), rng.integers(1, 9, n))[:n]
    for e in range(8192, n, 8192):
        gid[max(0, e - 3): e + 4] = gid[max(0, e - 3)]
    gid = np.maximum.accumulate(gid)
    return np.sort(distinct_keys(rng, int(gid[-1]) + 1))[gid]


RUN_N = (1, 2, 255, 256, 257, 8191, 8192, 8193, 20_000)
RUN_CASES = [(n, "runs") for n in RUN_N] + [(n, lay) for n in (2, 256, 8193) for lay in ("onerun", "distinct")]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "i64"])
@pytest.mark.parametrize("F", [1, 16])
@pytest.mark.parametrize("n,layout", RUN_CASES)
def test_run_aggregate_oracle(n, layout, F, dtype):
    cid = f"run-{n}-{layout}-F{F}-{dtype}"
    h = _ext.hip()
    for op in ("sum", "min", "max"):
        rng = _rng(f"{cid}-{op}")
        keys = run_keys(rng, n, layout)
        vals, exact = make_vals(rng, keys, F, dtype, op)
        o = oracle_groupby(keys, vals, op)
        for lay in ("row", "col") if (F > 1 and op == "min") else ("row",):
            r = h.run_aggregate(torch.from_numpy(keys).to(DEV), to_device(vals, lay), op)
            assert r, "non-descending keys must take the run path"
            rk, ra, rc, rf = (t.cpu().numpy() for t in r)
            # the groups come in row order, which for non-descending keys is the oracle's key order
            assert np.array_equal(rk, o.keys) and np.array_equal(rc, o.count) and np.array_equal(rf, o.first)
            assert ra.shape == (o.keys.size, F)
            check_aggs(ra, o, op, dtype, exact, f"{cid}-{op}-{lay}")
    r = h.run_aggregate(torch.from_numpy(keys).to(DEV), None, "sum")      # counts only
    assert r and np.array_equal(r[2].cpu().numpy(), o.count) and r[1].shape == (o.keys.size, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["min", "max"])
def test_run_aggregate_special_values_by_position(op):
    """The answer must not depend on where in its run a value sits: every pool member first, in the middle and last
    in a run of five, and every ordered pair of pool members as a run of two (so [1.5, NaN] and [NaN, 1.5],
    [+0.0, -0.0] and [-0.0, +0.0]); the same oracle as the hash paths, groups in row order."""
    rng = _rng(f"run-special-{op}")
    P = F64_POOL.size
    runs = []
    for p in range(P):
        for pos in (0, 2, 4):
            v = F64_POOL[rng.integers(0, P, 5)]
            v[pos] = F64_POOL[p]
            runs.append(v)
    for a in range(P):
        for b in range(P):
            runs.append(F64_POOL[[a, b]])
    vals = np.concatenate(runs).reshape(-1, 1)
    gid = np.repeat(np.arange(len(runs)), [r.size for r in runs])
    keys = np.sort(distinct_keys(rng, len(runs)))[gid]
    o = oracle_groupby(keys, vals, op)
    r = _ext.hip().run_aggregate(torch.from_numpy(keys).to(DEV), to_device(vals, "row"), op)
    assert r
    rk, ra, rc, rf = (t.cpu().numpy() for t in r)
    assert np.array_equal(rk, o.keys) and np.array_equal(rc, o.count)
    assert np.array_equal(rf, np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]])))   # the run heads
    check_bits(ra, o.agg, f"run {op}")
    # and the hash path on the same rows gives the same bits
    hr = _ext.hip().hash_aggregate(torch.from_numpy(keys).to(DEV), to_device(vals, "row"), op, False, 0, True)
    reps, aggs = hr[0].cpu().numpy(), hr[1].cpu().numpy()
    check_bits(aggs[np.argsort(reps, kind="stable")], ra, f"hash against run {op}")


# ------------------------------------------------------------------------------------------------ GPU: engine level
ENGINE_N, ENGINE_KEYS = 5000, 200
NP_DTYPE = {"float64": np.float64, "float32": np.float32, "int32": np.int32}


def _engine_vals(rng, keys, op, vdtype):
    """values [n, 2] of the column dtype and the exact float64 sum columns."""
    n = keys.size
    ginv = np.unique(keys, return_inverse=True)[1].reshape(-1)
    if vdtype == "int32":
        if op in ("min", "max"):
            v = rng.integers(-(1 << 31), (1 << 31) - 1, (n, 2), endpoint=True)
            v[rng.random((n, 2)) < 0.2] = -(1 << 31)
            v[rng.random((n, 2)) < 0.2] = (1 << 31) - 1
        else:
            v = rng.integers(-1000, 1000, (n, 2), endpoint=True)      # the sums stay inside int32, the output dtype
        return v.astype(np.int32), []
    if op in ("min", "max"):
        if vdtype == "float32":
            v = F32_POOL[rng.integers(0, F32_POOL.size, (n, 2))]
            v[ginv % 5 == 0, 0] = F32_POOL[4:7][rng.integers(0, 3, int((ginv % 5 == 0).sum()))]   # all-NaN groups
            return v, []
        return f64_minmax_vals(rng, ginv, 2), []
    if vdtype == "float32":
        v = np.stack([f64_sum_col(rng, ginv, "mixed").astype(np.float32),
                      f64_sum_col(rng, ginv, "int").astype(np.float32)], axis=1)
        return v, [1]
    return np.stack([f64_sum_col(rng, ginv, "nonfinite"), f64_sum_col(rng, ginv, "int")], axis=1), [1]


def _check_engine(agg, o, op, vdtype, exact, what):
    """group_reduce's aggregates [g, 2] against the oracle of the float64 / int64 images of the values, through the
    output conversion: rounding to the output dtype is monotone, so a sum inside [ref - b, ref + b] converts to a value
    inside [convert(ref - b), convert(ref + b)]; a mean adds the one rounding of its division."""
    out = np.float64 if (op == "mean" and vdtype == "int32") else NP_DTYPE[vdtype]
    assert agg.dtype == out and agg.shape == (o.keys.size, 2), (what, agg.dtype, agg.shape)
    if op in ("min", "max") or (vdtype == "int32" and op == "sum"):
        ref = o.agg.astype(out)
        assert np.array_equal(agg.view(np.uint8), ref.view(np.uint8)), (what, agg[agg != ref], ref[agg != ref])
        return
    c = o.count.reshape(-1, 1).astype(LD)
    if vdtype == "int32":             # mean of integers: the exact sum, one conversion-free division
        q = o.agg.astype(LD) / c
        lo, hi, cls = q - LD(U) * np.abs(q), q + LD(U) * np.abs(q), np.zeros(q.shape, dtype=np.int64)
    else:
        b = sum_bound(o.nfin, o.S)
        lo, hi, cls = o.agg - b, o.agg + b, o.cls
        if op == "mean":
            lo, hi = lo / c, hi / c
            w = LD(U) * (1 + LD(2.0 ** -10))
            lo, hi = lo - w * np.abs(lo), hi + w * np.abs(hi)
    assert np.isnan(agg[cls == 3]).all() and (agg[cls == 1] == np.inf).all() and (agg[cls == 2] == -np.inf).all(), what
    fin = cls == 0
    with np.errstate(over="ignore"):
        lo, hi = lo.astype(out), hi.astype(out)
    ok = ~fin | ((lo <= agg) & (agg <= hi))
    assert ok.all(), (what, agg[~ok], lo[~ok], hi[~ok])
    assert not np.signbit(agg[agg == 0]).any(), f"{what}: a zero result is -0.0"
    if op == "sum":
        for f in exact:
            assert np.array_equal(agg[:, f], (o.agg[:, f].astype(np.float64) + 0.0).astype(out)), (what, f)


@pytest.mark.gpu
@pytest.mark.parametrize("vdtype", ["float64", "float32", "int32"])
@pytest.mark.parametrize("op", ["sum", "min", "max", "mean", "count"])
def test_group_reduce_three_ways(op, vdtype, monkeypatch):
    """The same rows through K.group_reduce shuffled (hash path), sorted by key (run path) and in four chunks (chunk
    merge): each against the oracle, and bit-identical among themselves wherever the order of the rows cannot
    matter (min, max, count, integer sums and means)."""
    cid = f"engine-{op}-{vdtype}"
    rng = _rng(cid)
    keys = make_keys(rng, ENGINE_N, "uniform", ENGINE_KEYS) >> 40       # packed keys: the values themselves
    vals, exact = _engine_vals(rng, keys, op, vdtype)
    wide = vals.astype(np.int64 if vdtype == "int32" else np.float64)
    o = oracle_groupby(keys, wide, "sum" if op in ("mean", "count") else op)
    srt = np.argsort(keys, kind="stable")

    def run(rows, way):
        reps, agg = K.group_reduce(torch.from_numpy(keys[rows]).to(DEV), torch.from_numpy(vals[rows]).to(DEV), op)
        assert reps.dtype == torch.int64 and np.array_equal(reps.cpu().numpy(), o.keys), way
        agg = agg.cpu().numpy()
        if op == "count":
            assert agg.dtype == np.int64 and np.array_equal(agg, o.count), way
        else:
            _check_engine(agg, o, op, vdtype, exact, f"{cid}-{way}")
        return agg

    allrows = np.arange(ENGINE_N)
    K.LAST_RUN_AGG.update(tried=0, used=0)
    res = {"shuffled": run(allrows, "shuffled")}
    assert K.LAST_RUN_AGG["tried"] == 0 and K.LAST_AGG_STATUS["ok"] == 1
    with monkeypatch.context() as m:
        m.setattr(K, "RUN_AGG_MIN_ROWS", 1)
        res["sorted"] = run(srt, "sorted")
        assert K.LAST_RUN_AGG["used"] == 1, "sorted packed keys must take the run path"
    with monkeypatch.context() as m:
        m.setattr(K, "AGG_CHUNK_ROWS", ENGINE_N // 4 + 1)
        res["chunked"] = run(allrows, "chunked")
    assert K.LAST_RUN_AGG["used"] == 1
    if op in ("min", "max", "count") or vdtype == "int32":
        for way in ("sorted", "chunked"):
            assert np.array_equal(res[way].view(np.uint8), res["shuffled"].view(np.uint8)), way
