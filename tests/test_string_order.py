"""ORDER BY on string keys: StringColumn.order_words / cmp_rows / order_perm / order_codes / dict_encode(sorted=True)
(objects/strings.py over strings.hip str_order_words_kernel and str_cmp_pairs_kernel) and string keys in
K.order_by / K.order_limit / RecordBatch.order_by.

The order is the unsigned bytes of the UTF-8 encoding, lexicographically, a proper prefix first; equal strings tie and
the next key, then the ascending row id, decides. Every oracle is written here from Python's own bytes order and never
calls the code under test: the permutation is ``sorted(range(n), key=lambda i: (s[i].encode(), i))``, dense ranks come
from ``sorted(set(bytes))``, the words from ``int.from_bytes``. numpy appears with ``dtype=object`` only ('S' arrays
strip trailing NULs).

The strings share heavy prefixes: a random base of L bytes over NUL, 'a', 'b', 0x7F and multi-byte characters (bytes
>= 0x80), and every row a prefix of it, optionally followed by one more character, or the base itself. The CPU tests
run the numpy paths; the gpu tests run the same checks on cuda:0 with path="device" and path="torch" at 1, 2, 257,
2048 / 2049 (the order_limit / radix boundary), 4097 (one tile plus one) and 8193 rows, and bounds L = 0 (the
length-only group), 1, 7, 8, 9 (the chunk edge), 24 / 25 (one group against two: the first use of ids), 33 and 70
(three groups)."""
import random

import numpy as np
import pytest
import torch

from netsdb_amd.execution import kernels as K
from netsdb_amd.objects.record import RecordBatch
from netsdb_amd.objects.strings import StringColumn, string_order_plan

ALPHABET = ["\0", "a", "b", "\x7f", "é", "€", "\U0001F600"]
FIXED = ["ab", "ab\0", "ab\0\0", "", "a", "é", "€", "\U0001F600", "ab\x01", "abcdefgh", "abcdefg", "abcdefghi", "~"]
FIXED_CODES = [2, 3, 4, 0, 1, 10, 11, 12, 5, 7, 6, 8, 9]
BOUNDS = (0, 1, 7, 8, 9, 24, 25, 33, 70)
ROWS = (1, 2, 257, 2048, 2049, 4097, 8193)
GPU_CASES = sorted({(n, L) for n in (2049, 4097) for L in BOUNDS} | {(n, 25) for n in ROWS})
MIN64 = -(1 << 63)


# ---------------------------------------------------------------------------------------------- generator and oracles
def gen_strings(n, L, seed):
    """n rows of at most L bytes with heavy shared prefixes; row 0 is the base itself (exactly L bytes)."""
    rnd = random.Random(seed * 7919 + 131 * L + n)
    base, size = [], 0
    while size < L:
        ch = rnd.choice([c for c in ALPHABET if len(c.encode()) <= L - size])
        base.append(ch)
        size += len(ch.encode())
    rows = ["".join(base)]
    while len(rows) < n:
        kind = rnd.random()
        if kind < 0.15 or not base:
            rows.append("".join(base))
            continue
        k = rnd.randint(0, len(base))
        s = "".join(base[:k])
        if kind < 0.6:
            fit = [c for c in ALPHABET if len(s.encode()) + len(c.encode()) <= L]
            if fit:
                s += rnd.choice(fit)
        rows.append(s)
    assert max(len(s.encode()) for s in rows) == L
    return rows


def enc(strs):
    return [s.encode() for s in strs]


def perm_ref(strs):
    b = enc(strs)
    return sorted(range(len(b)), key=lambda i: (b[i], i))


def codes_ref(strs):
    b = enc(strs)
    rank = {v: r for r, v in enumerate(sorted(set(b)))}
    return [rank[v] for v in b]


def word_ref(b, t):
    """Chunk t of the bytes b as the signed sortable word: big-endian, zero padded, sign bit flipped."""
    u = int.from_bytes(b[8 * t:8 * t + 8].ljust(8, b"\0"), "big") ^ (1 << 63)
    return u - (1 << 64) if u >= (1 << 63) else u


def words_ref(strs, first, count, ids=None):
    b = enc(strs)
    rows = [b[i] if 0 <= i < len(b) else b"" for i in (range(len(b)) if ids is None else ids)]
    words = [np.array([word_ref(r, first + t) for r in rows], dtype=object) for t in range(count)]
    return words, [len(r) for r in rows]


def cmp_ref(x, y):
    return (x > y) - (x < y)


def sorted_by(n, *keys):
    """Row ids ordered by the given per-row key lists, ties by row id."""
    return sorted(range(n), key=lambda i: tuple(k[i] for k in keys) + (i,))


# ------------------------------------------------------------------------------------------------------ shared checks
def check_order_words(strs, dev, combos=((0, 1), (0, 4), (1, 3), (3, 2)), extra_ids=()):
    col = StringColumn.from_list(strs, dev)
    n = len(strs)
    rnd = random.Random(n)
    some = [rnd.randrange(n) for _ in range(max(1, n // 2))] + list(extra_ids)
    for first, count in combos:
        for ids in (None, some):
            for with_len in (False, True):
                t = None if ids is None else torch.tensor(ids, dtype=torch.int64)
                got = col.order_words(first, count, ids=t, with_len=with_len)
                want_w, want_l = words_ref(strs, first, count, ids)
                assert len(got) == count + int(with_len)
                for g, w in zip(got[:count], want_w):
                    assert g.dtype == torch.int64 and g.device.type == col.device.type
                    assert g.cpu().tolist() == list(w), (first, count, ids is not None)
                if with_len:
                    assert got[-1].dtype == torch.int32
                    assert got[-1].cpu().tolist() == want_l


def check_column(strs, dev, path=None):
    """order_perm, order_codes, cmp_rows, dict_encode(sorted=True) and the one-key ORDER BY of one list of strings."""
    n = len(strs)
    b = enc(strs)
    want_perm, want_codes = perm_ref(strs), codes_ref(strs)
    col = StringColumn.from_list(strs, dev)
    p = col.order_perm(path=path)
    assert p.dtype == torch.int64 and p.cpu().tolist() == want_perm
    codes = StringColumn.from_list(strs, dev).order_codes(path=path)
    assert codes.dtype == torch.int32 and codes.device.type == col.device.type
    assert codes.cpu().tolist() == want_codes
    rnd = random.Random(n + 1)
    m = min(4 * n, 4096)
    ia, ib = [rnd.randrange(n) for _ in range(m)], [rnd.randrange(n) for _ in range(m)]
    got = col.cmp_rows(torch.tensor(ia), col, torch.tensor(ib))
    assert got.dtype == torch.int8
    assert got.cpu().tolist() == [cmp_ref(b[x], b[y]) for x, y in zip(ia, ib)]
    dcodes, dictionary = StringColumn.from_list(strs, dev).dict_encode(sorted=True)
    assert dcodes.dtype == torch.int64 and dcodes.cpu().tolist() == want_codes
    assert [s.encode() for s in dictionary] == sorted(set(b))
    assert K.order_by([StringColumn.from_list(strs, dev)], path=path).cpu().tolist() == want_perm
    neg = [-c for c in want_codes]
    assert K.order_by([StringColumn.from_list(strs, dev)], True, path=path).cpu().tolist() == sorted_by(n, neg)


def check_mixed_keys(strs, dev, path=None):
    n = len(strs)
    g = torch.Generator().manual_seed(n)
    x = torch.randint(0, 5, (n,), generator=g, dtype=torch.int32)
    f = torch.randint(0, 3, (n,), generator=g).double() / 2
    k = torch.randint(-4, 4, (n,), generator=g, dtype=torch.int64)
    code = codes_ref(strs)
    xl, fl, kl = x.tolist(), f.tolist(), k.tolist()
    col = StringColumn.from_list(strs, dev)
    got = K.order_by([col, x.to(dev)], [True, False], path=path)
    assert got.cpu().tolist() == sorted_by(n, [-c for c in code], xl)
    limit = max(1, n // 3)
    got = K.order_by([f.to(dev), StringColumn.from_list(strs, dev), k.to(dev)], [False, False, True], limit=limit,
                     path=path)
    assert got.cpu().tolist() == sorted_by(n, fl, code, [-v for v in kl])[:limit]
    assert K.order_limit([StringColumn.from_list(strs, dev)], 10).cpu().tolist() == perm_ref(strs)[:10]
    # the string column arrives reordered: a take() view over the shuffled base
    shuffle = torch.randperm(n, generator=g)
    inv = torch.empty_like(shuffle)
    inv[shuffle] = torch.arange(n)
    base = StringColumn.from_list([strs[i] for i in shuffle.tolist()], dev)
    batch = RecordBatch({"name": base.take(inv.to(dev)), "x": x.to(dev), "row": torch.arange(n, device=dev)}, n)
    out = batch.order_by(["name", "x"])
    want = sorted_by(n, code, xl)
    assert out.columns["row"].cpu().tolist() == want
    assert out.columns["name"].tolist() == [strs[i] for i in want]
    assert batch.order_limit(["name", "x"], 7).columns["row"].cpu().tolist() == want[:7]
    # a host list[str] key beside a tensor key
    assert K.order_by([list(strs), x.to(dev)], path=path).cpu().tolist() == want


def check_views(dev, path=None):
    strs = gen_strings(300, 25, 5)
    base = StringColumn.from_list(strs, dev)
    base_codes = base.order_codes(path=path)
    assert base.order_codes() is base_codes                       # kept with the column
    idx = [7, 7, 299, 0, 7, 13, 0] + [i for i, s in enumerate(strs) if s == ""][:3]
    view = base.take(torch.tensor(idx))
    assert view._order_codes is None                              # the base's ranks are not the view's
    sel = [strs[i] for i in idx]
    assert view.order_codes(path=path).cpu().tolist() == codes_ref(sel)
    assert view.order_perm(path=path).cpu().tolist() == perm_ref(sel)
    none = base.take(torch.zeros(0, dtype=torch.int64))
    assert none.order_codes(path=path).numel() == 0 and none.order_perm(path=path).numel() == 0
    sub = base.substr(3, 9)
    cut = [s.encode()[3:12] for s in strs]
    rank = {v: r for r, v in enumerate(sorted(set(cut)))}
    assert sub.order_codes(path=path).cpu().tolist() == [rank[v] for v in cut]
    assert base.order_codes() is base_codes and base_codes.cpu().tolist() == codes_ref(strs)
    both = StringColumn.concat([base, view])
    assert both.order_codes(path=path).cpu().tolist() == codes_ref(strs + sel)


# --------------------------------------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("max_len,groups", [
    (0, [(0, 0, True)]), (8, [(0, 1, True)]), (24, [(0, 3, True)]), (25, [(1, 3, True), (0, 1, False)]),
    (33, [(2, 3, True), (0, 2, False)]), (70, [(6, 3, True), (2, 4, False), (0, 2, False)]),
    (7, [(0, 1, True)]), (9, [(0, 2, True)]), (32, [(1, 3, True), (0, 1, False)])])
def test_string_order_plan(max_len, groups):
    plan = string_order_plan(max_len, 1000)
    assert plan["groups"] == groups
    assert plan["chunks"] == (max_len + 7) // 8
    # the groups cover [chunk 0 .. chunk R-1, len] once, least significant first, at most 4 words each
    assert sum(c + int(w) for _, c, w in groups) == plan["chunks"] + 1
    assert all(c + int(w) <= 4 for _, c, w in groups) and [w for _, _, w in groups] == [True] + [False] * (len(groups) - 1)


def test_fixed_list_cpu():
    b = enc(FIXED)
    assert codes_ref(FIXED) == FIXED_CODES
    assert np.unique(np.array(b, dtype=object), return_inverse=True)[1].tolist() == FIXED_CODES
    check_column(FIXED, None)
    check_column(FIXED[::-1], None)          # "ab", "ab\0", "ab\0\0" no longer arrive in their own order
    col = StringColumn.from_list(FIXED)
    assert col.order_codes().tolist() == FIXED_CODES
    n = len(FIXED)
    ia = [i for i in range(n) for _ in range(n)]
    ib = [j for _ in range(n) for j in range(n)]
    got = col.cmp_rows(torch.tensor(ia), col, torch.tensor(ib)).tolist()
    assert got == [cmp_ref(b[i], b[j]) for i, j in zip(ia, ib)]
    codes, dictionary = col.dict_encode(sorted=True)
    assert codes.tolist() == FIXED_CODES and [s.encode() for s in dictionary] == sorted(set(b))


def test_order_words_cpu():
    strs = gen_strings(200, 40, 1) + FIXED                   # rows shorter than 8 * first included
    assert min(len(s.encode()) for s in strs) == 0
    check_order_words(strs, None, extra_ids=(len(strs), -1, 1 << 40))
    col = StringColumn.from_list(strs)
    (ln,) = col.order_words(0, 0, with_len=True)             # the length-only call
    assert ln.tolist() == [len(s.encode()) for s in strs]
    with pytest.raises(ValueError):
        col.order_words(0, 5)
    with pytest.raises(ValueError):
        col.order_words(0, 0)


@pytest.mark.parametrize("L", BOUNDS)
def test_column_cpu(L):
    check_column(gen_strings(300, L, 2), None)


def test_mixed_keys_cpu():
    check_mixed_keys(gen_strings(300, 25, 3), None)


def test_views_and_caching_cpu():
    check_views(None)


def test_empty_and_single_cpu():
    for strs in ([], ["x"], ["", ""]):
        col = StringColumn.from_list(strs)
        assert col.order_perm().tolist() == perm_ref(strs)
        assert col.order_codes().tolist() == codes_ref(strs)
        assert K.order_by([col]).tolist() == perm_ref(strs)


def test_dict_encode_default_unchanged():
    strs = gen_strings(200, 25, 4)
    codes, dictionary = StringColumn.from_list(strs).dict_encode()
    assert [dictionary[c] for c in codes.tolist()] == strs
    assert len(dictionary) == len(set(strs))


def test_device_path_needs_gpu_columns():
    with pytest.raises(ValueError):
        K.order_by([StringColumn.from_list(FIXED)], path="device")


# --------------------------------------------------------------------------------------------------------- GPU tests
DEV = "cuda:0"


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["device", "torch"])
@pytest.mark.parametrize("n,L", GPU_CASES)
def test_column_gpu(n, L, path):
    check_column(gen_strings(n, L, 11), DEV, path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["device", "torch", None])
def test_fixed_list_gpu(path):
    check_column(FIXED, DEV, path)
    check_column(FIXED[::-1], DEV, path)
    assert StringColumn.from_list(FIXED, DEV).order_codes(path=path).cpu().tolist() == FIXED_CODES


@pytest.mark.gpu
def test_order_words_gpu():
    strs = gen_strings(700, 40, 1) + FIXED
    check_order_words(strs, DEV)
    (ln,) = StringColumn.from_list(strs, DEV).order_words(0, 0, with_len=True)
    assert ln.cpu().tolist() == [len(s.encode()) for s in strs]


@pytest.mark.gpu
@pytest.mark.parametrize("last", [8, 9, 16])
def test_buffer_end_gpu(last):
    """The last row ends exactly at the payload's end; with the short rows before it, every chunk at or past a row's
    end — up to 8 * 5 bytes past the 16-byte pad here — must come out as the zero chunk without being read."""
    strs = ["", "a", "ab\0"] + ["b" * last]
    col = StringColumn.from_list(strs, DEV)
    assert int(col.ends[-1]) == col.payload and col.data.numel() == ((col.payload + 16 + 3) // 4) * 4
    check_order_words(strs, DEV, combos=((0, 1), (0, 4), (1, 3), (2, 4), (3, 2)))
    check_column(strs, DEV, "device")


@pytest.mark.gpu
def test_out_of_range_id_gpu():
    strs = gen_strings(100, 25, 6)
    col = StringColumn.from_list(strs, DEV)
    ids = [0, 100, -1, 1 << 40, 99, -(1 << 40)]
    w0, w1, ln = col.order_words(0, 2, ids=torch.tensor(ids), with_len=True)
    want_w, want_l = words_ref(strs, 0, 2, ids)
    assert w0.cpu().tolist() == list(want_w[0]) and w1.cpu().tolist() == list(want_w[1])
    assert ln.cpu().tolist() == want_l
    for j in (1, 2, 3, 5):                                   # the empty row: zero chunks, length 0
        assert w0[j].item() == MIN64 and w1[j].item() == MIN64 and ln[j].item() == 0


@pytest.mark.gpu
def test_cmp_rows_two_columns_gpu():
    sa, sb = gen_strings(500, 33, 7), gen_strings(300, 33, 7)[::-1] + FIXED
    a, b = StringColumn.from_list(sa, DEV), StringColumn.from_list(sb, DEV)
    rnd = random.Random(9)
    ia = [rnd.randrange(len(sa)) for _ in range(2000)]
    ib = [rnd.randrange(len(sb)) for _ in range(2000)]
    got = a.cmp_rows(torch.tensor(ia), b, torch.tensor(ib)).cpu().tolist()
    ea, eb = enc(sa), enc(sb)
    assert got == [cmp_ref(ea[i], eb[j]) for i, j in zip(ia, ib)]
    assert b.cmp_rows(None, a, None).cpu().tolist() == [cmp_ref(y, x) for x, y in zip(ea, eb)]


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["device", "torch", None])
def test_mixed_keys_gpu(path):
    check_mixed_keys(gen_strings(2500, 25, 3), DEV, path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["device", "torch"])
def test_views_and_caching_gpu(path):
    check_views(DEV, path)


@pytest.mark.gpu
def test_dispatch_counters_gpu():
    strs = gen_strings(4097, 25, 8)
    groups = string_order_plan(25, 4097)["groups"]
    stats = {}
    got = K.order_by([StringColumn.from_list(strs, DEV)], stats=stats, path="device")
    assert got.cpu().tolist() == perm_ref(strs)
    assert stats["device_string_order"] == 1
    assert stats["device_order_by"] == len(groups) + 1        # every group of the chain, then the sort of the ranks
    stats = {}
    K.order_by([StringColumn.from_list(strs, DEV)], stats=stats)
    assert stats["device_string_order"] == 1
    # 4, 2 and 1 keys of 4,097 rows all stay below order_by's measured thresholds: no radix call by default
    assert stats.get("device_order_by", 0) == 0


@pytest.mark.gpu
def test_repeatable_gpu():
    strs = gen_strings(8193, 33, 9)
    runs = [(StringColumn.from_list(strs, DEV).order_perm(path="device"),
             StringColumn.from_list(strs, DEV).order_codes(path="device")) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.gpu
def test_dict_encode_default_unchanged_gpu():
    strs = gen_strings(500, 25, 4)
    codes, dictionary = StringColumn.from_list(strs, DEV).dict_encode()
    assert [dictionary[c] for c in codes.cpu().tolist()] == strs
