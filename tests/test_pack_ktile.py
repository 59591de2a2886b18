"""ops.pack_ktile on the CPU: the torch fallback against the definition of the k-tile-major packed copy,
out[kt][r][c] = t[r][64 kt + c] and zero outside rows x K, shape [ceil(K/64), roundup(rows, 256), 64]."""
import pytest
import torch

from netsdb_amd import ops


def _definition(t):
    rows, K = t.shape
    out = torch.zeros((K + 63) // 64, (rows + 255) // 256 * 256, 64, dtype=torch.bfloat16)
    for kt in range(out.shape[0]):
        w = min(64, K - 64 * kt)
        out[kt, :rows, :w] = t[:, 64 * kt: 64 * kt + w]
    return out


@pytest.mark.parametrize("K", [8, 64, 72, 1000])
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_pack_ktile_fallback_is_the_definition(rows, K):
    g = torch.Generator().manual_seed(rows * 1009 + K)
    t = torch.randn(rows, K, generator=g).to(torch.bfloat16)
    t[t == 0] = 1.0                       # every zero of the copy is padding
    got = ops.pack_ktile(t)
    assert got.dtype == torch.bfloat16 and got.is_contiguous()
    assert got.shape == ((K + 63) // 64, (rows + 255) // 256 * 256, 64)
    assert torch.equal(got, _definition(t))
    assert int((got != 0).sum()) == rows * K


@pytest.mark.parametrize("rows,K,ld", [(257, 72, 80), (3, 1000, 1024), (256, 64, 4096)])
def test_pack_ktile_fallback_strided_rows(rows, K, ld):
    g = torch.Generator().manual_seed(ld)
    big = torch.randn(rows, ld, generator=g).to(torch.bfloat16)
    t = big[:, :K]
    assert t.stride(0) == ld > K
    assert torch.equal(ops.pack_ktile(t), _definition(t.contiguous()))
