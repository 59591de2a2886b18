"""The 8-phase GEMM streaming one operand from its k-tile-major packed copy (ops.pack_ktile, gemm_nt a_packed= /
b_packed=, plan kernel "8ph_pk") on the GPU. Only the addressing of that operand's global -> LDS stream differs from
the row-major launch, so the two launches of one call must agree bit for bit (torch.equal), and on small-integer
operands, where every partial sum is exact in f32, both equal the fp32 reference exactly."""
import tempfile

import pytest
import torch

from netsdb_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(200, 264), (520, 300), (1000, 1000)]
KS = [64, 128, 192, 320, 448, 456, 1000]      # 1-3 k-tiles, odd counts, ragged last tiles


def _ints(rows, K, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-3, 4, (rows, K), device=DEV, generator=g).to(torch.bfloat16)


def _both(A, B, side, **kw):
    """(packed launch, row-major launch) of one cfg-2 call; the plan must really take the packed kernel."""
    plan_kw = dict(splits=kw.get("splits", 0), cfg=2, out_dtype=kw.get("out_dtype", torch.bfloat16),
                   bias_mode=kw.get("bias_mode", 0))
    plan = ops.gemm_plan(A.shape[0], B.shape[0], A.shape[1], packed=side, **plan_kw)
    base = ops.gemm_plan(A.shape[0], B.shape[0], A.shape[1], **plan_kw)
    assert plan == dict(base, kernel="8ph_pk", packed=side) and base["kernel"] == "8ph"
    pk = {"a_packed": ops.pack_ktile(A)} if side == 1 else {"b_packed": ops.pack_ktile(B)}
    return ops.gemm_nt(A, B, cfg=2, **kw, **pk), ops.gemm_nt(A, B, cfg=2, **kw)


def test_pack_ktile_kernel_is_the_definition():
    for rows, K, ld in [(1, 8, 8), (255, 72, 72), (257, 1000, 1000), (300, 456, 512), (1000, 4096, 4096)]:
        t = _ints(rows, ld, rows)[:, :K]
        got = ops.pack_ktile(t)
        assert got.is_cuda and torch.equal(got.cpu(), ops.pack_ktile(t.cpu()))


@pytest.mark.parametrize("side", [1, 2], ids=["packed_a", "packed_b"])
@pytest.mark.parametrize("M,N", SHAPES)
def test_packed_equals_row_major_and_fp32(M, N, side):
    for K in KS:
        A, B = _ints(M, K, 3 * K + 1), _ints(N, K, 3 * K + 2)
        got, row = _both(A, B, side, out_dtype=torch.float32, splits=1)
        assert torch.equal(got, row), K
        assert torch.equal(got, A.float() @ B.float().t()), K


@pytest.mark.parametrize("side", [1, 2], ids=["packed_a", "packed_b"])
@pytest.mark.parametrize("M,N,K,splits", [(520, 300, 456, 3), (200, 264, 1000, 3), (1000, 1000, 448, 3),
                                          (1000, 1000, 65536, 16), (520, 300, 65000, 16)])
def test_packed_split_k(M, N, K, splits, side):
    """Split-K slabs and the reducer; 456 / 1000 / 65000 leave the last split short and its last k-tile ragged."""
    A, B = _ints(M, K, 11), _ints(N, K, 12)
    assert ops.gemm_plan(M, N, K, splits=splits, cfg=2, packed=side)["splits"] == splits
    got, row = _both(A, B, side, out_dtype=torch.float32, splits=splits)
    assert torch.equal(got, row)
    assert torch.equal(got, A.float() @ B.float().t())


@pytest.mark.parametrize("side", [1, 2], ids=["packed_a", "packed_b"])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
def test_packed_epilogue(out_dtype, splits, side):
    """bias + relu + dropout: the epilogue (and the dropout hash's element indices) are the row-major launch's."""
    M, N, K = 520, 300, 1000
    g = torch.Generator(device=DEV).manual_seed(4)
    A = (torch.randn(M, K, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    B = (torch.randn(N, K, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    bias = torch.randn(N, device=DEV, generator=g)
    kw = dict(bias=bias, bias_mode=ops.BIAS_COL, act=ops.ACT_RELU, out_dtype=out_dtype, splits=splits)
    got, row = _both(A, B, side, dropout=0.3, seed=9, **kw)
    assert torch.equal(got, row)
    assert 0.2 < float((got == 0).float().mean()) < 0.9          # the dropout ran
    got, row = _both(A, B, side, **kw)
    assert torch.equal(got, row)
    ref = torch.relu(A.float() @ B.float().t() + bias)
    err = (got.float() - ref).abs().max().item()
    # f32: accumulation order only; bf16: one rounding of values below 2 (2^-8 relative)
    assert err <= (1e-4 if out_dtype == torch.float32 else 2 ** -8 * max(1.0, ref.max().item())), err


@pytest.mark.parametrize("side", [1, 2], ids=["packed_a", "packed_b"])
def test_packed_with_strided_a_view(side):
    M, N, K = 520, 300, 456
    A = _ints(M, 1024, 21)[:, :K]
    B = _ints(N, K, 22)
    assert A.stride(0) == 1024
    got, row = _both(A, B, side, out_dtype=torch.float32, splits=1)
    assert torch.equal(got, row)
    assert torch.equal(got, A.float() @ B.float().t())


@pytest.mark.parametrize("side", [1, 2], ids=["packed_a", "packed_b"])
def test_packed_identity_asymmetric(side):
    """A = I with an asymmetric B: a transposed or row-permuted stream of either operand shows."""
    n = 256
    A = torch.eye(n, device=DEV, dtype=torch.bfloat16)
    B = (torch.arange(n * n, device=DEV, dtype=torch.float32).reshape(n, n) % 97 - 48).to(torch.bfloat16)
    got, row = _both(A, B, side, out_dtype=torch.float32)
    assert torch.equal(got, row)
    assert torch.equal(got, B.float().t().contiguous())


def test_dropped_request_reads_the_row_major_operand():
    """A request the plan drops (the 128x128 tile kernel) launches as if it were not there."""
    A, B = _ints(200, 320, 31), _ints(264, 320, 32)
    assert ops.gemm_plan(200, 264, 320, cfg=0, packed=2)["kernel"] == "tile128"
    got = ops.gemm_nt(A, B, cfg=0, out_dtype=torch.float32, b_packed=torch.zeros_like(ops.pack_ktile(B)))
    assert torch.equal(got, A.float() @ B.float().t())


def test_planner_packs_a_model_weight_once():
    """A two-layer FF through inference_unit: layer 1 (200 x 264 x 65536, an 8-phase launch) streams W1 from its
    packed copy, made on the first call and found in ops._DERIVED on the next two; the output is the one the same
    model gives with W1's locality left at "job", where the planner does not pack."""
    from netsdb_amd.client import PDBClient
    from netsdb_amd.models import ff
    from netsdb_amd.models.blocks import to_tensor

    assert ops.gemm_plan(264, 200, 65536, bias_mode=1, packed=1)["kernel"] == "8ph_pk"
    assert ops.gemm_plan(200, 264, 65536, bias_mode=2, packed=2)["kernel"] == "8ph_pk"
    c = PDBClient(root=tempfile.mkdtemp(), device=DEV)
    ff.load_model(c, "ff", 200, 65536, 264, 300, 64, 4096, seed=77)

    def tags():
        return [k for k in (ops._DERIVED or {}) if k[0] == "ktile64"]

    before = tags()
    calls = []
    real = ops.pack_ktile
    try:
        ops.pack_ktile = lambda t: (calls.append(tuple(t.shape)), real(t))[1]
        outs = []
        for _ in range(3):
            ff.inference_unit(c, "ff", "w1", "wo", "inputs", "b1", "bo", "output", dropout_rate=0.0, seed=0)
            outs.append(to_tensor(c, "ff", "output").float().clone())
        new = [k for k in tags() if k not in before]
        assert calls == [(264, 65536)] and len(new) == 1          # packed once, two _DERIVED hits
        assert tuple(ops._DERIVED[new[0]][1].shape) == (1024, 512, 64)
        c.set_locality("ff", "w1", "job")
        ff.inference_unit(c, "ff", "w1", "wo", "inputs", "b1", "bo", "output", dropout_rate=0.0, seed=0)
        assert calls == [(264, 65536)]                             # a "job" set is not packed
        plain = to_tensor(c, "ff", "output").float()
    finally:
        ops.pack_ktile = real
    assert all(torch.equal(o, plain) for o in outs)
