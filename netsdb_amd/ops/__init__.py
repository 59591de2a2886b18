"""Tensor operators used by the netsDB UDF library (block GEMM, conv2d, softmax, ...).

GPU tensors run on the hand-written CDNA4 HIP kernels in ``netsdb_amd/csrc/kernels``; there is
no silent eager fallback on a GPU (a missing extension raises).  CPU tensors run the plain fp32
PyTorch reference of the same op — that is the CPU pseudo-cluster path (the reference netsDB is a
CPU system) and the numerics oracle of the kernel tests.
"""
from __future__ import annotations

import contextlib
import threading

import numpy as np
import torch

from .. import _ext

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_EXP, ACT_TANH = 0, 1, 2, 3, 4
_ACT_NAMES = {"none": 0, None: 0, "relu": 1, "sigmoid": 2, "exp": 3, "tanh": 4}

BIAS_NONE, BIAS_ROW, BIAS_COL, BIAS_MAT = 0, 1, 2, 3


def act_code(act) -> int:
    if isinstance(act, int):
        return act
    return _ACT_NAMES[act]


def _apply_act(x: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_RELU:
        return torch.relu(x)
    if act == ACT_SIGMOID:
        return torch.sigmoid(x)
    if act == ACT_EXP:
        return torch.exp(x)
    if act == ACT_TANH:
        return torch.tanh(x)
    return x


def hash_uniform(seed: int, idx: np.ndarray) -> np.ndarray:
    """Host twin of the kernels' counter-based RNG (common.h hash_uniform)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + idx.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def _dropout_ref(v: torch.Tensor, p: float, seed: int, base: int = 0) -> torch.Tensor:
    if p <= 0:
        return v
    idx = np.arange(v.numel(), dtype=np.uint64) + np.uint64(base)
    u = torch.from_numpy(hash_uniform(seed, idx)).reshape(v.shape)
    return torch.where(u < p, torch.zeros_like(v), v / (1.0 - p))


def _use_hip(*ts) -> bool:
    on_gpu = any(t is not None and t.is_cuda for t in ts)
    if on_gpu:
        _ext.hip()  # raises loudly when the kernels are missing
    return on_gpu


def gemm_operands(A, B):
    """bf16, K-contiguous operands with 16-B rows and equal (multiple-of-8) K, as the MFMA kernels read them."""
    # compute dtype is bf16 on the matrix cores (f32 operands are rounded once here)
    if A.dtype != torch.bfloat16:
        A = A.to(torch.bfloat16)
    if B.dtype != torch.bfloat16:
        B = B.to(torch.bfloat16)
    if A.stride(-1) != 1 or A.stride(-2) % 8:
        A = pad_k(A.contiguous())
    if B.stride(-1) != 1 or B.stride(-2) % 8:
        B = pad_k(B.contiguous())
    if A.shape[-1] != B.shape[-1] or A.shape[-1] % 8:
        k = max(A.shape[-1], B.shape[-1])
        k = (k + 7) // 8 * 8
        A = torch.nn.functional.pad(A, (0, k - A.shape[-1])) if A.shape[-1] < k else A
        B = torch.nn.functional.pad(B, (0, k - B.shape[-1])) if B.shape[-1] < k else B
    return A, B


_STREAMS = None


def _streams():
    """execution.streams, imported once (it imports this module lazily: no import cycle at load time)."""
    global _STREAMS
    if _STREAMS is None:
        from ..execution import streams

        _STREAMS = streams
    return _STREAMS


def gemm_nt(A, B, bias=None, bias_mode=BIAS_NONE, act=ACT_NONE, out_dtype=torch.bfloat16, alpha=1.0,
            dropout=0.0, seed=0, splits=0, out=None, accumulate=False, cfg=None, epi=None, mfma=None, fixup=None,
            a_packed=None, b_packed=None):
    """epilogue(alpha * A @ B^T) [+ out when accumulate]: A [..,M,K], B [..,N,K] (K-contiguous),
    bias f32 per row/col. ``accumulate`` adds into an existing f32 ``out`` (C += A.B^T). ``cfg`` forces the
    tile config of THIS call (0 = 128x128, 2 = 256x256 8-phase, 3 / 4 = 256x128 / 128x256 skinny long-K stream;
    None = auto); ``epi`` the 8-phase kernel's
    unsplit epilogue (0 = LDS-staged, 1 = direct register stores; None = auto: direct); ``mfma`` the 8-phase main
    loop's matrix instruction (16 = 16x16x32, 32 = 32x32x16; None = the thread's ``kernel_options(gemm_mfma=...)``,
    else the library default); ``fixup`` (8-phase split-K launches) 1 = the split-K reduction inside the launch (each
    split reduces 1/splits of its tile's rows after the tile's splits meet; no reducer launch), 0 = the separate
    reducer (None = the thread's ``kernel_options(gemm_fixup=...)``, else 0). An operand prefetch armed on
    the current stream (streams.arm_operand_prefetch: a later kernel's operand read into the Infinity Cache by this
    launch's workgroups as they finish) is handed to this launch when it is long enough to take it — per call and
    per stream, so GEMMs on other lanes or threads never see it. ``a_packed`` / ``b_packed`` is ``pack_ktile`` of A / B
    as passed (a weight's k-tile-major copy, made once): a request like the others, the launch streams that operand from
    the copy when its plan says ``8ph_pk`` (``gemm_plan(..., packed=1 / 2)``) and reads the row-major one otherwise, with
    bit-identical results; the CPU path ignores it."""
    act = act_code(act)
    if _use_hip(A, B):
        if bias is not None and bias.dtype != torch.float32:
            bias = bias.float()
        A0, B0 = A, B
        A, B = gemm_operands(A, B)
        if A is not A0:         # the copy describes the operand as passed, not a converted or re-padded one
            a_packed = None
        if B is not B0:
            b_packed = None
        pf = None
        streams = _streams()
        if streams._armed_pf:
            batch = A.shape[0] if A.dim() == 3 else 1
            if gemm_plan(A.shape[-2], B.shape[-2], A.shape[-1], batch, splits, cfg)["prefetch_eligible"]:
                pf = streams.take_operand_prefetch(A.device)
        return _ext.hip().gemm_nt(A, B, bias, int(bias_mode if bias is not None else 0), act,
                                  out_dtype == torch.float32, float(alpha), float(dropout), int(seed),
                                  int(splits), out, bool(accumulate), -1 if cfg is None else int(cfg),
                                  -1 if epi is None else int(epi), pf,
                                  int(mfma if mfma is not None else _kopt("gemm_mfma", 0)),
                                  int(fixup if fixup is not None else _kopt("gemm_fixup", 0)), a_packed, b_packed)
    v = torch.matmul(A.float(), B.float().transpose(-1, -2)) * alpha
    if bias is not None:
        b = bias.float()
        v = v + (b if bias_mode == BIAS_MAT else b.unsqueeze(-1) if bias_mode == BIAS_ROW else b.unsqueeze(-2))
    v = _apply_act(v, act)
    v = _dropout_ref(v, dropout, seed)
    if accumulate:
        out.add_(v.to(out.dtype))
        return out
    v = v.to(out_dtype)
    if out is not None:
        out.copy_(v)
        return out
    return v


def gemm_nt_f32(A, B, alpha=1.0, out=None, accumulate=False):
    """alpha * A @ B^T (+ out) at fp32 precision: A [M, K], B [N, K]. GPU tensors run the exact-f32 MFMA kernel
    (csrc/kernels/gemm_f32.hip; f64 inputs are computed in f32 there); CPU tensors keep their dtype (the
    reference analytics run in double)."""
    if _use_hip(A, B):
        A = A.float()
        B = B.float()
        if A.stride(-1) != 1 or A.stride(-2) % 4 or A.shape[-1] % 4:
            A = _pad_k4(A)
        if B.stride(-1) != 1 or B.stride(-2) % 4 or B.shape[-1] % 4:
            B = _pad_k4(B)
        if out is not None and (out.dtype != torch.float32 or out.stride(-1) != 1):
            r = _ext.hip().gemm_nt_f32(A, B, float(alpha))
            if accumulate:
                out.add_(r.to(out.dtype))
            else:
                out.copy_(r)
            return out
        return _ext.hip().gemm_nt_f32(A, B, float(alpha), out, bool(accumulate))
    dt = torch.promote_types(A.dtype, B.dtype)
    v = (A.to(dt) @ B.to(dt).transpose(-1, -2)) * alpha
    if out is not None:
        if accumulate:
            out.add_(v.to(out.dtype))
        else:
            out.copy_(v)
        return out
    return v


def _pad_k4(X):
    k = (X.shape[-1] + 3) // 4 * 4
    Y = torch.zeros(X.shape[:-1] + (k,), dtype=X.dtype, device=X.device)
    Y[..., : X.shape[-1]] = X
    return Y


def gemm_nt_softmax(A, B, bias=None, bias_mode=BIAS_NONE, axis=1, alpha=1.0, out=None, force_fallback=False,
                    epi=None):
    """softmax(alpha * A @ B^T + bias) along ``axis`` 1 (each row of the [M, N] result) or 2 (each column), f32.
    On the GPU the normalisation is fused into the GEMM epilogue (max-subtracted, no exp'd round trip through
    HBM; ``epi`` 0 = LDS-staged final store, 1 / None = direct register stores when C rows are 16-B aligned);
    the CPU oracle is the same max-subtracted softmax in fp32."""
    if _use_hip(A, B):
        if bias is not None and bias.dtype != torch.float32:
            bias = bias.float()
        A = A.to(torch.bfloat16) if A.dtype != torch.bfloat16 else A
        B = B.to(torch.bfloat16) if B.dtype != torch.bfloat16 else B
        if A.stride(-1) != 1 or A.stride(-2) % 8 or A.shape[-1] % 8:
            A = pad_k(A.contiguous())
        if B.stride(-1) != 1 or B.stride(-2) % 8 or B.shape[-1] % 8:
            B = pad_k(B.contiguous())
        if A.shape[-1] != B.shape[-1]:
            k = max(A.shape[-1], B.shape[-1])
            A = torch.nn.functional.pad(A, (0, k - A.shape[-1])) if A.shape[-1] < k else A
            B = torch.nn.functional.pad(B, (0, k - B.shape[-1])) if B.shape[-1] < k else B
        return _ext.hip().gemm_nt_softmax(A, B, bias, int(bias_mode if bias is not None else 0), int(axis), out,
                                          float(alpha), bool(force_fallback), -1 if epi is None else int(epi))
    v = torch.matmul(A.float(), B.float().transpose(-1, -2)) * alpha
    if bias is not None:
        b = bias.float()
        v = v + (b.unsqueeze(-1) if bias_mode == BIAS_ROW else b.unsqueeze(-2))
    y = torch.softmax(v, dim=-1 if axis == 1 else -2)
    if out is not None:
        out.copy_(y)
        return out
    return y


def gemm_nt_segmented(A, Bg, bias=None, bias_mode=BIAS_NONE, act=ACT_NONE, out_dtype=torch.bfloat16, dropout=0.0,
                      seed=0, out=None):
    """epilogue(A . Bcat^T) with Bcat [N, S*seg_k] held as an all-gathered [S, N, seg_k] chunk (rank s's K slab
    of every row): the GPU kernel walks the K segments in place (no permute copy); seg_k % 64 == 0."""
    act = act_code(act)
    if _use_hip(A, Bg):
        if bias is not None and bias.dtype != torch.float32:
            bias = bias.float()
        return _ext.hip().gemm_nt_bseg(A.to(torch.bfloat16), Bg.to(torch.bfloat16).contiguous(), bias,
                                       int(bias_mode if bias is not None else 0), act, out_dtype == torch.float32,
                                       1.0, float(dropout), int(seed), out)
    S, N, sk = Bg.shape
    Bcat = Bg.permute(1, 0, 2).reshape(N, S * sk)     # the CPU oracle may copy
    return gemm_nt(A, Bcat, bias, bias_mode, act, out_dtype, dropout=dropout, seed=seed, out=out)


def gemm_splits(M, N, K, batch=1) -> int:
    return int(_ext.hip().gemm_splits(M, N, K, batch))


def gemm_plan(M, N, K, batch=1, splits=0, cfg=None, epi=None, mfma=None, fixup=None, out_dtype=torch.bfloat16,
              accumulate=False, bias_mode=BIAS_NONE, ldc=None, c_align=16, seg_k=0, packed=0) -> dict:
    """What a GPU ``gemm_nt`` call of this shape and these options becomes (the options are requests): ``kernel``
    ("tile128", "8ph", "8ph32", "8ph_fixup", "stream256x128", "stream128x256", "8ph_pk"), ``cfg``, the effective ``splits``,
    ``reducer`` ("none", "plain", "wide", "in_launch"), ``direct_epi``, ``kinter``, ``wgs``, ``prefetch_eligible`` and
    ``packed`` (the request ``packed`` = 1 / 2, "A / B also comes as its ``pack_ktile`` copy", as the launch honours it:
    kernel "8ph_pk", or 0 with the plan it has without the request).
    Host arithmetic only: the function of gemm_plan.h that the launch itself follows. ``mfma`` / ``fixup`` None take the
    calling thread's ``kernel_options``, as in ``gemm_nt``; ``ldc`` is C's row stride (default N), ``c_align`` the
    alignment of its address in bytes, ``seg_k`` the segment length of ``gemm_nt_segmented``'s B."""
    return _ext.hip().gemm_plan(int(M), int(N), int(K), int(batch), int(splits), -1 if cfg is None else int(cfg),
                                -1 if epi is None else int(epi),
                                int(mfma if mfma is not None else _kopt("gemm_mfma", 0)),
                                int(fixup if fixup is not None else _kopt("gemm_fixup", 0)),
                                out_dtype == torch.float32, bool(accumulate), int(bias_mode),
                                -1 if ldc is None else int(ldc), int(c_align), int(seg_k), int(packed))


def pack_ktile(t: torch.Tensor) -> torch.Tensor:
    """The k-tile-major packed copy of a GEMM operand ``t`` [rows, K] (bf16): [ceil(K/64), roundup(rows, 256), 64]
    with element [kt, r, c] = t[r, 64 kt + c] and zero outside rows x K. The 8-phase GEMM streams a weight from this
    copy in 32 KiB runs per tile and k-tile (``gemm_nt(..., a_packed= / b_packed=)``) instead of one 128-B line per
    row; it costs the weight's size again, so it is made once (``derived``)."""
    rows, K = t.shape
    if _use_hip(t):
        if t.dtype != torch.bfloat16:
            t = t.to(torch.bfloat16)
        if t.stride(1) != 1 or t.stride(0) % 8 or K % 8:
            t = pad_k(t.contiguous())
        if t.data_ptr() % 16:
            t = t.clone()
        return _ext.hip().pack_ktile(t)
    kt, rp = (K + 63) // 64, (rows + 255) // 256 * 256
    return torch.nn.functional.pad(t.to(torch.bfloat16), (0, kt * 64 - K, 0, rp - rows)).view(rp, kt, 64) \
        .permute(1, 0, 2).contiguous()


_DERIVED: "OrderedDict" = None


_NO_CACHE_STORAGES: set = set()      # storages whose derivations are recomputed (execution/graphs.py inputs)


def derived(t: torch.Tensor, tag: str, fn):
    """Memoise a tensor derived from an unchanged source tensor (model weights / biases converted or
    re-laid-out once, not on every inference call). Keyed by storage pointer, in-place version
    counter, shape, dtype and device, so any write to the source invalidates the entry."""
    global _DERIVED
    from collections import OrderedDict

    if _NO_CACHE_STORAGES and t.untyped_storage().data_ptr() in _NO_CACHE_STORAGES:
        return fn(t)        # a captured job's input: the derivation must be part of the recorded kernels
    if _DERIVED is None:
        _DERIVED = OrderedDict()
    key = (tag, t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()), t.dtype, str(t.device))
    hit = _DERIVED.get(key)
    if hit is not None:
        _DERIVED.move_to_end(key)
        return hit[1]
    val = fn(t)
    _DERIVED[key] = (t, val)           # keep the source alive so its pointer is not reused
    if len(_DERIVED) > 256:
        _DERIVED.popitem(last=False)
    return val


def pad_k(t: torch.Tensor, mult: int = 8) -> torch.Tensor:
    """Zero-pad the last dim to a multiple of ``mult`` (block storage keeps rows 16-B aligned)."""
    k = t.shape[-1]
    kp = (k + mult - 1) // mult * mult
    if kp == k:
        return t
    return torch.nn.functional.pad(t, (0, kp - k))


def conv_filter_fragments(Wflat, C, KH, KW):
    """The filter [OC, >=C*KH*KW] (im2col (c, kh, kw) order) re-laid in the warp-specialised conv kernel's MFMA
    B-fragment order: [ceil(OC/64)][4 n-tiles][6 k-steps][64 lanes][8] bf16, lane l of n-tile nt / k-step ks
    holding oc = 64 t + 16 nt + (l & 15), taps kw = 0..7 of filter row q = 4 ks + (l >> 4) (q = c * KH + kh),
    zero past KW / C*KH / OC. The kernel then loads each fragment with one 16-B read (conv2d.hip conv2d_ws_kernel)."""
    OC = Wflat.shape[0]
    ckh = C * KH
    oct_ = (OC + 63) // 64
    dev = Wflat.device
    nt = torch.arange(4, device=dev).view(4, 1, 1, 1)
    ks = torch.arange(6, device=dev).view(1, 6, 1, 1)
    ln = torch.arange(64, device=dev).view(1, 1, 64, 1)
    kw = torch.arange(8, device=dev).view(1, 1, 1, 8)
    ocl = nt * 16 + (ln & 15)
    q = ks * 4 + (ln >> 4)
    kidx = (q.clamp(max=max(ckh - 1, 0)) * KW + kw.clamp(max=KW - 1)).expand(4, 6, 64, 8)
    valid = ((q < ckh) & (kw < KW)).expand(4, 6, 64, 8)
    Wp = torch.zeros(oct_ * 64, Wflat.shape[1], dtype=torch.bfloat16, device=dev)
    Wp[:OC] = Wflat.to(torch.bfloat16)
    out = []
    for t in range(oct_):
        rows = (t * 64 + ocl).expand(4, 6, 64, 8)
        out.append(torch.where(valid, Wp[rows, kidx], torch.zeros((), dtype=torch.bfloat16, device=dev)))
    return torch.stack(out).contiguous()


_KOPTS = threading.local()
_KOPT_KEYS = {"conv_kernel", "conv_blocks", "conv_generic", "conv_variant", "conv_contig", "rownorm_plain_loads",
              "hash_groupby", "gemm_mfma", "gemm_fixup"}


@contextlib.contextmanager
def kernel_options(**kw):
    """Kernel launch options for the HIP calls made by THIS thread inside the block (nested blocks override):
    conv_kernel (conv2d row kernel: 5 warp-specialised = default, 1 full-row, 0 two-pass; 2/3/4/6 diagnostics),
    conv_blocks (row-kernel grid cap, default 512; 0 = one block per row group), conv_generic (bool: the generic
    gather kernel), conv_variant / conv_contig (row-kernel diagnostics), rownorm_plain_loads (bool: row normalise
    with cache-allocating loads), hash_groupby (bool: device hash-table group ids, default off), gemm_mfma (16 / 32:
    the 8-phase GEMM main loop's MFMA shape; default the library's), gemm_fixup (0 / 1: split-K reduction inside the
    8-phase launch). Every option is
    passed per call to the kernel library, which keeps no process-wide launch state: other threads (server requests, job lanes on their own threads) never see them."""
    bad = set(kw) - _KOPT_KEYS
    if bad:
        raise ValueError(f"unknown kernel options {sorted(bad)}")
    prev = getattr(_KOPTS, "d", {})
    _KOPTS.d = {**prev, **{k: v for k, v in kw.items() if v is not None}}
    try:
        yield
    finally:
        _KOPTS.d = prev


def set_kernel_options(**kw) -> dict:
    """Set kernel launch options for the calling THREAD until changed (study scripts; ``kernel_options`` is the
    scoped form). A value of None removes the option. Returns the previous options (restore_kernel_options)."""
    bad = set(kw) - _KOPT_KEYS
    if bad:
        raise ValueError(f"unknown kernel options {sorted(bad)}")
    prev = getattr(_KOPTS, "d", {})
    d = dict(prev)
    for k, v in kw.items():
        if v is None:
            d.pop(k, None)
        else:
            d[k] = v
    _KOPTS.d = d
    return prev


def restore_kernel_options(prev: dict):
    _KOPTS.d = dict(prev)


def _kopt(name, default):
    return getattr(_KOPTS, "d", {}).get(name, default)


CONV_MAX_IMAGE_BYTES = 0x7FFFFFF0      # conv2d.hip: a masked load's byte offset; the bf16 image set must end below it


def _conv_packs_filter(C, KH, KW, stride, pad, dil) -> bool:
    """Shapes for which ``conv2d`` hands the kernels the MFMA-fragment packed filter (conv_filter_fragments)."""
    return stride == 1 and dil == 1 and pad == 0 and KW <= 8 and C * KH <= 24


def conv2d_plan(N, C, H, W, OC, KH, KW, stride=1, pad=0, dil=1, ldw=None, nchw_out=False,
                out_dtype=torch.bfloat16, has_wfrag=None) -> str:
    """The kernel a GPU ``conv2d`` call of this geometry gets under the calling thread's ``kernel_options``: "igemm"
    (generic gather), "rows" / "rows_staged" (two-pass row kernel, direct / LDS-staged stores), "rowfull", "ws"
    (warp-specialised) or "diag" (a timing build: conv_kernel 2/3/4/6 or conv_variant != 0, whose output is not the
    convolution). Host arithmetic only: the same function of conv2d.hip that the launch itself consults. ``ldw`` is
    the filter's row length (default K rounded up to 8); ``has_wfrag`` defaults to what ``conv2d`` would pass."""
    if ldw is None:
        ldw = (C * KH * KW + 7) // 8 * 8
    if has_wfrag is None:
        has_wfrag = _conv_packs_filter(C, KH, KW, stride, pad, dil)
    return _ext.hip().conv2d_plan(N, C, H, W, OC, KH, KW, stride, pad, dil, ldw, bool(nchw_out),
                                  out_dtype == torch.float32, bool(has_wfrag), int(_kopt("conv_kernel", -1)),
                                  int(_kopt("conv_blocks", -1)), bool(_kopt("conv_generic", False)),
                                  int(_kopt("conv_variant", 0)), int(_kopt("conv_contig", 0)))


def conv2d(X, Wflat, bias=None, KH=1, KW=1, stride=1, pad=0, dil=1, act=ACT_NONE, nchw_out=False,
           out_dtype=torch.bfloat16):
    """Fused implicit-GEMM conv. X [N,C,H,W]; Wflat [OC, >=C*KH*KW] in (c,kh,kw) im2col order, zero in the columns
    past C*KH*KW. Launch options come from the calling thread's ``kernel_options`` scope; ``conv2d_plan`` names the
    kernel a call gets. The bf16 image set must be smaller than 0x7ffffff0 bytes (RuntimeError otherwise). The row
    kernels ("rows", "rows_staged", "rowfull", "ws") read 8 taps per filter row with zero weights past KW, so a NaN or
    Inf pixel at column c makes outputs ow in [c-7, c] of its rows non-finite, not only [c-KW+1, c] as in the generic
    kernel and the CPU path."""
    act = act_code(act)
    if _use_hip(X, Wflat):
        if bias is not None and bias.dtype != torch.float32:
            bias = bias.float()
        C = X.shape[1]
        wfrag = None
        if _conv_packs_filter(C, KH, KW, stride, pad, dil):
            # small-C row-kernel shapes: the packed B fragments (cached per filter tensor and version)
            wfrag = derived(Wflat, f"conv_frag_{C}_{KH}_{KW}", lambda t: conv_filter_fragments(t, C, KH, KW))
        return _ext.hip().conv2d(X, Wflat, bias, KH, KW, stride, pad, dil, act, bool(nchw_out),
                                 out_dtype == torch.float32, wfrag, int(_kopt("conv_kernel", -1)),
                                 int(_kopt("conv_blocks", -1)), bool(_kopt("conv_generic", False)),
                                 int(_kopt("conv_variant", 0)), int(_kopt("conv_contig", 0)))
    N, C = X.shape[0], X.shape[1]
    OC = Wflat.shape[0]
    if X.numel() * 2 >= CONV_MAX_IMAGE_BYTES:
        raise RuntimeError("conv2d: image set too large (the kernels address it with 31-bit byte offsets)")
    w = Wflat[:, : C * KH * KW].float().reshape(OC, C, KH, KW)
    y = torch.nn.functional.conv2d(X.float(), w, bias.float() if bias is not None else None, stride, pad, dil)
    y = _apply_act(y, act)
    if not nchw_out:
        y = y.permute(0, 2, 3, 1).reshape(-1, OC)
    return y.to(out_dtype)


def im2col(X, KH, KW, stride=1, pad=0, dil=1, ldk=None):
    C = X.shape[1]
    K = C * KH * KW
    ldk = ldk or (K + 7) // 8 * 8
    if _use_hip(X):
        return _ext.hip().im2col(X, KH, KW, stride, pad, dil, ldk)
    # a pure gather, like the kernel: 16-bit elements travel as their bit patterns (exact in f64), so NaN payloads,
    # -0 and denormals come out as they went in
    bits = {2: torch.int16, 4: torch.int32}.get(X.element_size()) if X.is_floating_point() else None
    src = X.view(bits).double() if bits is not None else X.double()
    cols = torch.nn.functional.unfold(src, (KH, KW), dilation=dil, padding=pad, stride=stride)
    cols = torch.nn.functional.pad(cols.transpose(1, 2).reshape(-1, K), (0, ldk - K))
    return cols.to(bits).view(X.dtype) if bits is not None else cols.to(X.dtype)


_PREFETCH_SINK = {}


def prefetch(tensors, blocks=64):
    """Warm the GPU caches (Infinity Cache) with a read of each tensor on the current stream (HIP prefetch_kernel:
    one 16-B load per 128-B line, nothing written). For operands a later kernel reads after a cache-flushing
    one (the FF output weights after layer 1's 2.4 GB stream). CPU tensors: no-op."""
    ts = [t for t in tensors if isinstance(t, torch.Tensor) and t.is_cuda and t.numel()]
    if not ts:
        return
    dev = ts[0].device
    sink = _PREFETCH_SINK.get(dev)
    if sink is None:
        sink = _PREFETCH_SINK[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    _ext.hip().prefetch(ts, sink, int(blocks))


def softmax_rows(X, bias=None, out_dtype=torch.float32, log=False):
    if _use_hip(X):
        return _ext.hip().softmax_rows(X, bias, out_dtype == torch.float32, 1 if log else 0)
    v = X.float() + (bias.float() if bias is not None else 0.0)
    r = torch.log_softmax(v, dim=-1) if log else torch.softmax(v, dim=-1)
    return r.to(out_dtype)


def row_normalize(X, out_dtype=torch.float32):
    """x / rowsum(x) (FFOutputLayer over exp'd scores)."""
    if _use_hip(X):
        return _ext.hip().softmax_rows(X, None, out_dtype == torch.float32, 2,
                                       bool(_kopt("rownorm_plain_loads", False)))
    v = X.float()
    return (v / v.sum(-1, keepdim=True)).to(out_dtype)


def bias_act(X, bias=None, bias_mode=BIAS_COL, act=ACT_NONE, dropout=0.0, seed=0, out_dtype=torch.bfloat16):
    act = act_code(act)
    if _use_hip(X):
        if bias is not None and bias.dtype != torch.float32:
            bias = bias.float()
        return _ext.hip().bias_act(X.contiguous(), bias, int(bias_mode), act, float(dropout), int(seed),
                                   out_dtype == torch.float32)
    v = X.float()
    if bias is not None:
        v = v + (bias.float().unsqueeze(-1) if bias_mode == BIAS_ROW else bias.float())
    v = _dropout_ref(_apply_act(v, act), dropout, seed)
    return v.to(out_dtype)


def lstm_cell(gates, c_prev=None, h_dtype=torch.float32):
    if _use_hip(gates):
        return tuple(_ext.hip().lstm_cell(gates.contiguous(), c_prev, h_dtype == torch.float32))
    g = gates.float()
    H = g.shape[1] // 4
    i, f, gg, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), \
        torch.sigmoid(g[:, 3 * H:])
    c = f * (c_prev.float() if c_prev is not None else 0.0) + i * gg
    h = o * torch.tanh(c)
    return h.to(h_dtype), c


def lstm_two_sum(f, cp, i, g):
    """LSTMTwoSum: f * c_prev + i * g (f32, elementwise HIP kernel on the GPU)."""
    if _use_hip(f):
        t = [x.float().contiguous() for x in (f, cp, i, g)]
        return _ext.hip().lstm_ew(0, t[0], t[1], t[2], t[3])
    return f.float() * cp.float() + i.float() * g.float()


def lstm_hidden(o, c):
    """LSTMHiddenState: o * tanh(c)."""
    if _use_hip(o):
        return _ext.hip().lstm_ew(1, o.float().contiguous(), c.float().contiguous())
    return o.float() * torch.tanh(c.float())


def embedding_bag(table, idx, offsets, weights=None, mode="sum"):
    m = 1 if mode == "mean" else 0
    if _use_hip(table):
        return _ext.hip().embedding_bag(table, idx.long().contiguous(), offsets.long().contiguous(), weights, m)
    out = torch.zeros(offsets.numel() - 1, table.shape[1], dtype=torch.float32)
    t = table.float()
    for b in range(offsets.numel() - 1):
        s, e = int(offsets[b]), int(offsets[b + 1])
        if e > s:
            rows = t[idx[s:e].long()]
            if weights is not None:
                rows = rows * weights[s:e].float().unsqueeze(-1)
            out[b] = rows.sum(0) / ((e - s) if m == 1 else 1)
    return out


__all__ = [n for n in dir() if not n.startswith("_")]
