"""K.order_limit (ORDER BY up to 4 keys, mixed directions, LIMIT k): exact row ids against references written here —
Python's sorted with an explicit key up to 4097 rows, the stable-argsort chain on CPU copies above. CPU tensors take
the argsort-chain path of kernels.py; the gpu tests run csrc/kernels/topk.hip."""
import math

import pytest
import torch

from netsdb_amd.execution import kernels as K
from netsdb_amd.objects.record import RecordBatch

SIZES = (1, 17, 64, 65, 4097, 200003)
SMALL = tuple(n for n in SIZES if n <= 4097)
NAN, INF = float("nan"), float("inf")


def _elem_key(v, desc):
    """One key value as a Python sort key: NaN above +inf, -0.0 == 0.0, reversed when descending."""
    if isinstance(v, float) and math.isnan(v):
        return (0, 0) if desc else (1, 0)
    return (1, -v) if desc else (0, v)


def _listify(descending, m):
    return [bool(descending)] * m if isinstance(descending, bool) else [bool(d) for d in descending]


def _ref(keys, k, descending=False):
    """Expected row ids; never calls the code under test."""
    keys = [c.cpu() for c in keys]
    desc = _listify(descending, len(keys))
    n = keys[0].numel()
    if k <= 0 or n == 0:
        return []
    if n <= 4097:
        cols = [c.tolist() for c in keys]
        rows = sorted(range(n), key=lambda i: tuple(_elem_key(c[i], d) for c, d in zip(cols, desc)) + (i,))
        return rows[:k]
    order = None
    for c, d in zip(reversed(keys), reversed(desc)):
        c = c.double() if c.dtype in (torch.float16, torch.bfloat16) else c
        if order is None:
            order = torch.argsort(c, descending=d, stable=True)
        else:
            order = order[torch.argsort(c[order], descending=d, stable=True)]
    return order[:k].tolist()


NATIVE = (torch.int32, torch.int64, torch.float32, torch.float64)


def _check(keys, k, descending, dev, stats=None):
    """K.order_limit against the reference; on the GPU also the kernel entry itself (the dispatch keeps torch's path
    where many rows are kept out of few), whenever it accepts the call."""
    dkeys = [c.to(dev) for c in keys]
    exp = _ref(keys, k, descending)
    got = K.order_limit(dkeys, k, descending, stats=stats)
    assert got.dtype == torch.int64 and got.dim() == 1 and got.device.type == torch.device(dev).type
    assert got.tolist() == exp
    if dkeys[0].is_cuda and all(c.dtype in NATIVE for c in dkeys) and min(k, dkeys[0].numel()) <= K.ORDER_LIMIT_MAX_K:
        from netsdb_amd import _ext

        raw = _ext.hip().order_limit(dkeys, _listify(descending, len(dkeys)), k)
        assert raw.dtype == torch.int64 and raw.is_cuda and raw.tolist() == exp
    return got


def _ks(n):
    return [k for k in (1, 5, 64, 65, 2048)] + ([n, n + 3] if n <= 2048 else [])


_MATRIX = {}


def _matrix_keys(n):
    """Two keys: float32 with about n / 4 distinct values (descending), then int64 with 3 distinct values."""
    if n not in _MATRIX:
        g = torch.Generator().manual_seed(1000 + n)
        a = torch.randint(0, max(2, n // 4), (n,), generator=g).float() * 0.5 - 3.0
        b = torch.randint(-1, 2, (n,), generator=g, dtype=torch.int64)
        _MATRIX[n] = ([a, b], [True, False])
    return _MATRIX[n]


def _float_edges(dtype):
    tiny = 1e-45 if dtype == torch.float32 else 5e-324        # smallest subnormals
    sub = 1e-40 if dtype == torch.float32 else 1e-310
    base = [1.0, NAN, -0.0, 0.0, INF, 1.0, -INF, tiny, -tiny, sub, -sub, NAN, 0.0, -0.0, -1.5, 3.0e38, -3.0e38]
    return torch.tensor(base * 5, dtype=dtype)


# ------------------------------------------------------------------------------------------------ CPU
def test_documented_order_of_float_specials():
    x = torch.tensor([1, NAN, -0.0, 0.0, INF, 1, -INF], dtype=torch.float64)
    assert K.order_limit([x], 7, True).tolist() == [1, 4, 0, 5, 2, 3, 6]
    assert K.order_limit([x], 7, False).tolist() == [6, 2, 3, 0, 5, 4, 1]
    assert _ref([x], 7, True) == [1, 4, 0, 5, 2, 3, 6] and _ref([x], 7, False) == [6, 2, 3, 0, 5, 4, 1]


@pytest.mark.parametrize("n", SMALL)
def test_matrix_cpu(n):
    keys, desc = _matrix_keys(n)
    for k in _ks(n):
        _check(keys, k, desc, "cpu")


def test_empty_and_nonpositive_k_cpu():
    e = K.order_limit([torch.empty(0, dtype=torch.float64)], 5)
    assert e.dtype == torch.int64 and e.numel() == 0
    x = torch.arange(9)
    for k in (0, -3):
        e = K.order_limit([x], k)
        assert e.dtype == torch.int64 and e.numel() == 0


def test_k_above_n_cpu():
    x = torch.tensor([3, 1, 2, 1], dtype=torch.int32)
    assert K.order_limit([x], 100).tolist() == [1, 3, 2, 0]
    assert K.order_limit([x], 100, True).tolist() == [0, 2, 1, 3]


def test_dtype_promotion_cpu():
    g = torch.Generator().manual_seed(3)
    b = torch.randint(0, 2, (50,), generator=g).bool()
    s = torch.randint(-300, 300, (50,), generator=g).to(torch.int16)
    h = (torch.randint(-8, 8, (50,), generator=g).float() / 4).half()
    h[7] = NAN
    _check([b, s, h], 20, [True, False, True], "cpu")
    _check([h], 50, False, "cpu")
    _check([s], 13, True, "cpu")


def test_descending_bool_or_list_cpu():
    keys, _ = _matrix_keys(65)
    assert torch.equal(K.order_limit(keys, 9, True), K.order_limit(keys, 9, [True, True]))
    assert torch.equal(K.order_limit(keys, 9), K.order_limit(keys, 9, [False, False]))
    _check(keys, 9, True, "cpu")
    _check(keys, 9, [False, True], "cpu")
    with pytest.raises(ValueError):
        K.order_limit(keys, 9, [True])
    with pytest.raises(ValueError):
        K.order_limit([], 3)
    with pytest.raises(ValueError):
        K.order_limit([keys[0]] * 5, 3)


def test_record_batch_order_limit_cpu():
    keys, desc = _matrix_keys(64)
    b = RecordBatch({"a": keys[0], "b": keys[1], "row": torch.arange(64)}, 64)
    out = b.order_limit(["a", "b"], 10, desc)
    exp = _ref(keys, 10, desc)
    assert out.n == 10 and out.columns["row"].tolist() == exp
    assert torch.equal(out.columns["a"], keys[0][exp])


# ------------------------------------------------------------------------------------------------ GPU
DEV = "cuda:0"


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_matrix_gpu(n):
    keys, desc = _matrix_keys(n)
    stats = {}
    for k in _ks(n):
        _check(keys, k, desc, DEV, stats=stats)
    assert stats["device_order_limit"] >= 3            # k = 1, 5 and 64 dispatch to the kernel at every size


@pytest.mark.gpu
def test_candidate_list_two_values_gpu():
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 2, (200003,), generator=g, dtype=torch.int64) * 7 - 3
    _check([x], 100, False, DEV)
    _check([x], 100, True, DEV)


@pytest.mark.gpu
def test_candidate_list_all_equal_gpu():
    x = torch.full((70000,), 42, dtype=torch.int64)
    assert K.order_limit([x.to(DEV)], 100).tolist() == list(range(100))
    assert K.order_limit([x.to(DEV), x.to(DEV).double()], 100, [True, False]).tolist() == list(range(100))


@pytest.mark.gpu
def test_narrow_ranges_gpu():
    g = torch.Generator().manual_seed(6)
    a = torch.randint(0, 1000, (4097,), generator=g, dtype=torch.int64)
    f = torch.rand(4097, generator=g, dtype=torch.float64) + 1.0
    e = torch.tensor([-2 ** 63, -1, 0, 2 ** 63 - 1] * 9 + [5, -5], dtype=torch.int64)
    for keys in ([a], [f], [e]):
        for d in (False, True):
            _check(keys, 64, d, DEV)
    _check([e], e.numel(), False, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_float_edge_values_gpu(dtype):
    x = _float_edges(dtype)
    for d in (False, True):
        for k in (1, 7, x.numel()):
            _check([x], k, d, DEV)


@pytest.mark.gpu
def test_multi_key_gpu():
    g = torch.Generator().manual_seed(7)
    n = 4097
    k0 = torch.randint(0, 3, (n,), generator=g, dtype=torch.int32)            # 3 values: the k-th row is inside a tie group
    k1 = torch.randn(n, generator=g, dtype=torch.float64).round(decimals=1)
    k2 = torch.randint(-50, 50, (n,), generator=g, dtype=torch.int64)
    k3 = torch.randn(n, generator=g).float().round(decimals=0)
    _check([k0, k1, k2], 65, [False, True, False], DEV)
    _check([k0, k1, k2, k3], 2048, [True, False, True, True], DEV)
    # keys 0..2 tie on every row: only key 3 (7 values) and then the row id decide
    c0 = torch.full((n,), 2.5, dtype=torch.float32)
    c1 = torch.full((n,), -9, dtype=torch.int64)
    c2 = torch.zeros(n, dtype=torch.int32)
    k3 = torch.randint(0, 7, (n,), generator=g, dtype=torch.int64)
    _check([c0, c1, c2, k3], 100, [True, False, True, False], DEV)
    _check([c0, c1, c2, k3], 100, [False, True, False, True], DEV)


@pytest.mark.gpu
def test_strided_and_promoted_input_gpu():
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2 * 4097, generator=g, dtype=torch.float64).to(DEV)
    v = x[::2]
    assert not v.is_contiguous()
    assert K.order_limit([v], 65, True).tolist() == _ref([v.cpu()], 65, True)
    h = (torch.randint(-8, 8, (300,), generator=g).float() / 4).half()
    b = torch.randint(0, 2, (300,), generator=g).bool()
    _check([b, h], 17, [True, False], DEV)


@pytest.mark.gpu
def test_deterministic_gpu():
    keys, desc = _matrix_keys(200003)
    dk = [c.to(DEV) for c in keys]
    assert torch.equal(K.order_limit(dk, 2048, desc), K.order_limit(dk, 2048, desc))


@pytest.mark.gpu
def test_graph_capture_gpu():
    """The whole call is a data-independent chain of launches: captured once, replayed on new data in place."""
    g = torch.Generator().manual_seed(9)
    n = 4097
    a0 = torch.randint(0, 5, (n,), generator=g, dtype=torch.int64)
    b0 = torch.randn(n, generator=g, dtype=torch.float64)
    a1 = torch.randint(-(2 ** 40), 2 ** 40, (n,), generator=g, dtype=torch.int64)
    b1 = torch.full((n,), 1.25, dtype=torch.float64)
    a, b = a0.to(DEV), b0.to(DEV)
    desc = [False, True]
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        warm = K.order_limit([a, b], 64, desc)
    torch.cuda.synchronize(DEV)
    assert warm.tolist() == _ref([a0, b0], 64, desc)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = K.order_limit([a, b], 64, desc)
    a.copy_(a1.to(DEV))
    b.copy_(b1.to(DEV))
    torch.cuda.synchronize(DEV)
    graph.replay()
    torch.cuda.synchronize(DEV)
    assert out.tolist() == _ref([a1, b1], 64, desc)


@pytest.mark.gpu
def test_above_k_cap_falls_back_gpu():
    assert K.ORDER_LIMIT_MAX_K == 2048
    keys, desc = _matrix_keys(4097)
    stats = {"device_order_limit": 0}
    _check(keys, K.ORDER_LIMIT_MAX_K + 1, desc, DEV, stats=stats)
    assert stats == {"device_order_limit": 0}
    big, bdesc = _matrix_keys(200003)
    _check(big, K.ORDER_LIMIT_MAX_K, bdesc, DEV, stats=stats)
    assert stats == {"device_order_limit": 1}
