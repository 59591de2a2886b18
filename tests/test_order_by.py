"""K.order_by (ORDER BY up to 4 keys, mixed directions, no LIMIT needed): exact row ids against references written
here — Python's sorted with an explicit key up to 4097 rows, the stable-argsort chain on CPU copies above. CPU tensors
take the argsort-chain path of kernels.py; the gpu tests run csrc/kernels/sort.hip through path="device"."""
import math

import pytest
import torch

from netsdb_amd.execution import kernels as K
from netsdb_amd.objects.record import RecordBatch

TILE = K.ORDER_BY_TILE
NAN, INF = float("nan"), float("inf")
DEV = "cuda:0"


def _elem_key(v, desc):
    """One key value as a Python sort key: NaN above +inf, -0.0 == 0.0, reversed when descending."""
    if isinstance(v, float) and math.isnan(v):
        return (0, 0) if desc else (1, 0)
    return (1, -v) if desc else (0, v)


def _listify(descending, m):
    return [bool(descending)] * m if isinstance(descending, bool) else [bool(d) for d in descending]


def _ref(keys, descending=False, limit=None):
    """Expected row ids; never calls the code under test."""
    keys = [c.cpu() for c in keys]
    desc = _listify(descending, len(keys))
    n = keys[0].numel()
    k = n if limit is None else min(limit, n)
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


_MATRIX = {}


def _matrix_keys(n):
    """Two keys: float32 with about n / 4 distinct values (descending), then int64 with 3 distinct values."""
    if n not in _MATRIX:
        g = torch.Generator().manual_seed(2000 + n)
        a = torch.randint(0, max(2, n // 4), (n,), generator=g).float() * 0.5 - 3.0
        b = torch.randint(-1, 2, (n,), generator=g, dtype=torch.int64)
        _MATRIX[n] = ([a, b], [True, False])
    return _MATRIX[n]


_MATRIX_REF = {}


def _matrix_ref(n):
    """The full expected order of _matrix_keys(n), computed once."""
    if n not in _MATRIX_REF:
        keys, desc = _matrix_keys(n)
        _MATRIX_REF[n] = _ref(keys, desc)
    return _MATRIX_REF[n]


# ------------------------------------------------------------------------------------------------ CPU
def test_documented_order_of_float_specials():
    x = torch.tensor([1, NAN, -0.0, 0.0, INF, 1, -INF], dtype=torch.float64)
    assert K.order_by([x], True).tolist() == [1, 4, 0, 5, 2, 3, 6]
    assert K.order_by([x], False).tolist() == [6, 2, 3, 0, 5, 4, 1]
    assert _ref([x], True) == [1, 4, 0, 5, 2, 3, 6] and _ref([x], False) == [6, 2, 3, 0, 5, 4, 1]


@pytest.mark.parametrize("n", (1, 17, 2049, 4097))
def test_matrix_cpu(n):
    keys, desc = _matrix_keys(n)
    exp = _matrix_ref(n)
    got = K.order_by(keys, desc)
    assert got.dtype == torch.int64 and got.dim() == 1 and got.tolist() == exp
    for limit in (1, 5, 2049, n, n + 3):
        assert K.order_by(keys, desc, limit=limit).tolist() == exp[:limit]
    assert K.order_by(keys, desc, path="torch").tolist() == exp


def test_empty_and_nonpositive_limit_cpu():
    e = K.order_by([torch.empty(0, dtype=torch.float64)])
    assert e.dtype == torch.int64 and e.numel() == 0 and e.device.type == "cpu"
    e = K.order_by([torch.empty(0, dtype=torch.float64)], limit=5)
    assert e.dtype == torch.int64 and e.numel() == 0
    x = torch.arange(9)
    for limit in (0, -3):
        e = K.order_by([x], limit=limit)
        assert e.dtype == torch.int64 and e.numel() == 0


def test_dtype_promotion_cpu():
    g = torch.Generator().manual_seed(3)
    b = torch.randint(0, 2, (50,), generator=g).bool()
    s = torch.randint(-300, 300, (50,), generator=g).to(torch.int16)
    h = (torch.randint(-8, 8, (50,), generator=g).float() / 4).half()
    h[7] = NAN
    assert K.order_by([b, s, h], [True, False, True]).tolist() == _ref([b, s, h], [True, False, True])
    assert K.order_by([h]).tolist() == _ref([h])
    assert K.order_by([s], True, limit=13).tolist() == _ref([s], True, 13)
    assert K.order_by(h, True).tolist() == _ref([h], True)              # a bare tensor is one key


def test_descending_bool_or_list_cpu():
    keys, _ = _matrix_keys(17)
    assert torch.equal(K.order_by(keys, True), K.order_by(keys, [True, True]))
    assert torch.equal(K.order_by(keys), K.order_by(keys, [False, False]))
    assert K.order_by(keys, True).tolist() == _ref(keys, True)
    assert K.order_by(keys, [False, True]).tolist() == _ref(keys, [False, True])


def test_value_errors_cpu():
    keys, _ = _matrix_keys(17)
    with pytest.raises(ValueError):
        K.order_by(keys, [True])
    with pytest.raises(ValueError):
        K.order_by([])
    with pytest.raises(ValueError):
        K.order_by([keys[0]] * 5)
    with pytest.raises(ValueError):
        K.order_by([keys[0], keys[1][:5]])
    with pytest.raises(ValueError):
        K.order_by([keys[0].reshape(1, -1)])
    with pytest.raises(ValueError):
        K.order_by(keys, path="fastest")


def test_record_batch_order_by_cpu():
    keys, desc = _matrix_keys(2049)
    b = RecordBatch({"a": keys[0], "b": keys[1], "row": torch.arange(2049)}, 2049)
    exp = _matrix_ref(2049)
    out = b.order_by(["a", "b"], desc)
    assert out.n == 2049 and out.columns["row"].tolist() == exp
    assert torch.equal(out.columns["a"], keys[0][exp])
    out = b.order_by(["a", "b"], desc, limit=10)
    assert out.n == 10 and out.columns["row"].tolist() == exp[:10]


def test_device_path_on_cpu_raises():
    keys, desc = _matrix_keys(17)
    with pytest.raises(ValueError):
        K.order_by(keys, desc, path="device")
    with pytest.raises(ValueError):
        K.order_by_plan([torch.float32, torch.int64], 5000, False, "device")


def test_plan_is_torch_on_cpu():
    for n in (0, 1, 2049, 1 << 24):
        assert K.order_by_plan([torch.float32, torch.int64], n, False) == {"path": "torch"}
    assert K.order_by_plan([torch.float64], 5000, True, "torch") == {"path": "torch"}
    assert K.order_by_plan([torch.float64], 2 ** 31, True) == {"path": "torch"}
    stats = {}
    keys, desc = _matrix_keys(2049)
    K.order_by(keys, desc, stats=stats)
    assert stats == {}


# ------------------------------------------------------------------------------------------------ GPU
def _check_dev(keys, descending=False, limit=None, exp=None):
    """path="device" against the reference, after the plan has named the arm; the radix arm counts itself."""
    dkeys = [c.to(DEV) for c in keys]
    n = dkeys[0].numel()
    plan = K.order_by_plan([c.dtype for c in dkeys], n, True, "device")
    assert plan["path"] == ("radix" if n > K.ORDER_LIMIT_MAX_K else "order_limit")
    if exp is None:
        exp = _ref(keys, descending, limit)
    stats = {}
    got = K.order_by(dkeys, descending, stats=stats, limit=limit, path="device")
    assert got.dtype == torch.int64 and got.dim() == 1 and got.is_cuda
    got = got.tolist()
    assert len(got) == len(exp)
    assert got == exp
    if plan["path"] == "radix":
        assert stats == {"device_order_by": 1}
        assert plan["tile"] == TILE and plan["tiles"] == -(-n // TILE)
    return plan


@pytest.mark.gpu
def test_tile_is_the_extensions_gpu():
    from netsdb_amd import _ext

    assert _ext.hip().ORDER_BY_TILE == TILE
    assert _ext.hip().ORDER_LIMIT_MAX_K == K.ORDER_LIMIT_MAX_K == 2048


@pytest.mark.gpu
@pytest.mark.parametrize("n", (2049, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 200003))
def test_tile_edges_gpu(n):
    keys, desc = _matrix_keys(n)
    exp = _matrix_ref(n)
    _check_dev(keys, desc, exp=exp)
    _check_dev(keys, desc, limit=2049, exp=exp[:2049])
    dkeys = [c.to(DEV) for c in keys]
    assert K.order_by(dkeys, desc).tolist() == exp                       # the default dispatch, whichever arm
    assert K.order_by(dkeys, desc, path="torch").tolist() == exp


def _random_bits(dtype, n, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype in (torch.int32, torch.float32):
        bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    else:
        bits = torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), generator=g, dtype=torch.int64)
    if dtype == torch.float32:
        bits[9], bits[10] = 0x7FC12345, 0x7F800001 - 2 ** 32 + 2 ** 31       # NaNs of both signs, with payloads
    if dtype == torch.float64:
        bits[9], bits[10] = 0x7FF8000000012345, -0x0007FFFFFFFFFFFF
    return bits.view(dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (4097, 70001))
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.float32, torch.float64])
def test_every_dtype_gpu(dtype, n):
    """Random bit patterns: every byte varies; float words hold NaN payloads, infinities' neighbours and subnormals."""
    x = _random_bits(dtype, n, 11 + n)
    if dtype.is_floating_point:
        x[5], x[n - 3], x[77] = INF, -INF, NAN
        assert torch.isnan(x[9:11]).all() and torch.isnan(x).sum() >= 3
    for d in (False, True):
        plan = _check_dev([x], d)
        assert plan["passes"] == x.element_size() and plan["word_bits"] == 8 * x.element_size()


def _float_edges(dtype):
    tiny = 1e-45 if dtype == torch.float32 else 5e-324        # smallest subnormals
    sub = 1e-40 if dtype == torch.float32 else 1e-310
    base = [1.0, NAN, -0.0, 0.0, INF, 1.0, -INF, tiny, -tiny, sub, -sub, NAN, 0.0, -0.0, -1.5, 3.0e38, -3.0e38]
    return torch.tensor(base * 121, dtype=dtype)              # 2057 rows


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_float_edge_values_gpu(dtype):
    x = _float_edges(dtype)
    assert x.numel() > K.ORDER_LIMIT_MAX_K
    for d in (False, True):
        _check_dev([x], d)


@pytest.mark.gpu
def test_live_pass_parity_gpu():
    """1, 2 and 3 live passes with dead passes before, between and after them: the source buffer of a pass is the
    number of LIVE passes before it."""
    g = torch.Generator().manual_seed(12)
    n = 4097
    term = [(torch.randint(0, 256, (n,), generator=g, dtype=torch.int64) << (8 * b)) for b in range(4)]

    def i32(x):
        x = x & 0xFFFFFFFF                               # (byte 3 reaches the sign bit: wrap by hand)
        return torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32)

    cases = [i32(term[b]) for b in range(4)]
    cases += [i32(term[0] + term[2]), i32(term[1] + term[3]), i32(term[0] + term[3]), i32(term[1] + term[2])]
    cases += [i32(term[0] + term[1] + term[3]), i32(term[0] + term[2] + term[3]), i32(term[1] + term[2] + term[3])]
    e = torch.tensor([-2 ** 63, -1, 0, 2 ** 63 - 1], dtype=torch.int64)[torch.randint(0, 4, (n,), generator=g)]
    cases += [e, torch.randint(0, 1000, (n,), generator=g, dtype=torch.int64)]
    for x in cases:
        for d in (False, True):
            _check_dev([x], d)


@pytest.mark.gpu
def test_no_live_pass_gpu():
    n = 70000
    x = torch.full((n,), 42, dtype=torch.int64)
    y = torch.full((n,), -2.5, dtype=torch.float64)
    ident = list(range(n))
    _check_dev([x], False, exp=ident)
    _check_dev([x, y], [True, False], exp=ident)
    _check_dev([x, y], [True, False], limit=100, exp=ident[:100])


@pytest.mark.gpu
def test_four_keys_gpu():
    g = torch.Generator().manual_seed(13)
    n = 4097
    k0 = torch.randint(0, 3, (n,), generator=g, dtype=torch.int32)
    k1 = torch.randn(n, generator=g, dtype=torch.float64).round(decimals=1)
    k2 = torch.randint(-50, 50, (n,), generator=g, dtype=torch.int64)
    k3 = torch.randn(n, generator=g).float().round(decimals=0)
    _check_dev([k0, k1, k2, k3], [True, False, True, True])
    _check_dev([k0, k1, k2, k3], [False, True, False, False])
    # keys 0..2 tie on every row: only key 3 (7 values) and then the row id decide
    c0 = torch.full((n,), 2.5, dtype=torch.float32)
    c1 = torch.full((n,), -9, dtype=torch.int64)
    c2 = torch.zeros(n, dtype=torch.int32)
    s3 = torch.randint(0, 7, (n,), generator=g, dtype=torch.int64)
    _check_dev([c0, c1, c2, s3], [True, False, True, False])
    _check_dev([c0, c1, c2, s3], [False, True, False, True])
    # a constant key between two varying ones: its load and passes are skipped, the parity carries over it
    _check_dev([k0, c1, k3], [False, False, True])
    _check_dev([k0, c0, k2, k3], [True, True, False, False])


@pytest.mark.gpu
def test_sorted_inputs_gpu():
    n = 200003
    up = torch.arange(n, dtype=torch.int64) - 1000
    swapped = up.clone()
    swapped[[70001, 70002]] = swapped[[70002, 70001]]
    for x in (up, up.flip(0), swapped):
        for d in (False, True):
            _check_dev([x], d)
    _check_dev([up.double()], True)


@pytest.mark.gpu
def test_strided_and_promoted_input_gpu():
    g = torch.Generator().manual_seed(14)
    n = 4097
    x = torch.randn(2 * n, generator=g, dtype=torch.float64).to(DEV)
    v = x[::2]
    assert not v.is_contiguous()
    assert K.order_by_plan([v.dtype], n, True, "device")["path"] == "radix"
    assert K.order_by([v], True, path="device").tolist() == _ref([v.cpu()], True)
    h = (torch.randint(-8, 8, (n,), generator=g).float() / 4).half()
    h[7] = NAN
    b = torch.randint(0, 2, (n,), generator=g).bool()
    _check_dev([b, h], [True, False])


@pytest.mark.gpu
def test_many_tiles_gpu():
    """More tiles than one os_scan_kernel workgroup covers in one step: the scan's carry across steps."""
    probe = K.order_by_plan([torch.int32, torch.int64], TILE + 1, True, "device")
    n = min(probe["scan_step"] * probe["tile"] + 1 + 3, 1 << 23)
    g = torch.Generator().manual_seed(15)
    a = torch.randint(0, 50000, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    b = torch.randint(-1, 2, (n,), generator=g, dtype=torch.int64)
    plan = _check_dev([a, b], [True, False])
    assert plan["tiles"] > plan["scan_step"] or n == 1 << 23


@pytest.mark.gpu
def test_default_dispatch_gpu():
    """Whatever arm the default dispatch picks, order_by_plan names it, only the radix arm counts itself, and the rows
    are the reference's. Three keys at 2^18 rows and one row below: both sides of the one measured threshold."""
    g = torch.Generator().manual_seed(18)
    for n in ((1 << 18) - 1, 1 << 18):
        a = torch.randint(0, n // 16, (n,), generator=g).double() / 7
        b = torch.randint(0, 2500, (n,), generator=g, dtype=torch.int64).to(torch.int32)
        c = torch.randint(0, 1 << 40, (n,), generator=g, dtype=torch.int64)
        desc = [True, False, False]
        exp = _ref([a, b, c], desc)
        for keys in ([a, b, c], [a, b], [c]):
            dk = [x.to(DEV) for x in keys]
            d = desc[:len(keys)]
            plan = K.order_by_plan([x.dtype for x in dk], n, True)
            assert plan["path"] in ("radix", "torch")
            stats = {}
            got = K.order_by(dk, d, stats=stats)
            assert stats == ({"device_order_by": 1} if plan["path"] == "radix" else {})
            assert got.tolist() == (exp if len(keys) == 3 else _ref(keys, d))


@pytest.mark.gpu
def test_agrees_with_order_limit_gpu():
    keys, desc = _matrix_keys(200003)
    dk = [c.to(DEV) for c in keys]
    full = K.order_by(dk, desc, path="device")
    from netsdb_amd import _ext

    for k in (1, 64, 2048):
        assert torch.equal(full[:k], _ext.hip().order_limit(dk, desc, k))
        assert torch.equal(full[:k], K.order_limit(dk, k, desc))


@pytest.mark.gpu
def test_deterministic_gpu():
    keys, desc = _matrix_keys(200003)
    dk = [c.to(DEV) for c in keys]
    assert torch.equal(K.order_by(dk, desc, path="device"), K.order_by(dk, desc, path="device"))


@pytest.mark.gpu
def test_graph_capture_gpu():
    """The whole call is a data-independent chain of launches: captured once on data with few live passes and a
    constant key, replayed on data in which every pass of both keys is live."""
    g = torch.Generator().manual_seed(16)
    n = 4097
    a0 = torch.randint(0, 5, (n,), generator=g, dtype=torch.int64)
    b0 = torch.full((n,), 1.25, dtype=torch.float64)
    a1 = _random_bits(torch.int64, n, 17)
    a1[:64] = a1[64:128]                                  # rows that tie on the first key: the second decides
    b1 = torch.randn(n, generator=g, dtype=torch.float64)
    a, b = a0.to(DEV), b0.to(DEV)
    desc = [False, True]
    assert K.order_by_plan([a.dtype, b.dtype], n, True, "device")["path"] == "radix"
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        warm = K.order_by([a, b], desc, path="device")
    torch.cuda.synchronize(DEV)
    assert warm.tolist() == _ref([a0, b0], desc)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = K.order_by([a, b], desc, path="device")
    a.copy_(a1.to(DEV))
    b.copy_(b1.to(DEV))
    torch.cuda.synchronize(DEV)
    graph.replay()
    torch.cuda.synchronize(DEV)
    assert out.tolist() == _ref([a1, b1], desc)
