"""Every kernel form of the block GEMM (csrc/kernels/gemm.hip, gemm_common.h, gemm_plan.h) and the exact-f32 GEMM
(gemm_f32.hip) against a float64 oracle written from the definition.

Oracle. ``_oracle(A, B, bias, mode, alpha, act, dropout, seed, C0)`` is ``A.double() @ B.double().transpose(-1, -2)``
on the CPU, then alpha, then the bias (per row, per column or a matrix), then the activation, then dropout, then
``+ C0``. It calls nothing from ``ops``: the dropout uniform is ``_hash_uniform``, a NumPy transcription of
``hash_uniform`` in common.h, over the element index ``(b * M + row) * N + col`` (N, not the row stride of C); an
element is kept when ``u >= p`` and scaled by ``1 / (1 - p)``. Each case runs twice against the same oracle: on the
``ops`` CPU fallback (unmarked) and on the HIP kernels (``gpu`` mark). Every GPU case first asserts
``ops.gemm_plan``: ``kernel``, ``splits``, ``reducer``, ``direct_epi``, ``kinter`` and ``packed``, so a case can
never run another kernel than its id says. ``test_case_table_reaches_every_kernel_and_reducer`` checks the whole
table against the planner without a GPU and requires all seven kernel names and all four reducer names.

Forms (``FORMS``): ``tile128`` (cfg 0); ``8ph_lds`` / ``8ph_direct`` (cfg 2 with epi 0 / 1); ``8ph32`` (mfma 32);
``8ph_fixup`` (the in-launch reducer); ``8ph_pk_a`` / ``8ph_pk_b`` (A / B streamed from its pack_ktile copy);
``stream256x128`` / ``stream128x256`` (cfg 3 / 4) and their k-interleaved twins (cfg 5 / 6). The direct epilogue,
``8ph32`` and ``8ph_fixup`` exist only where C rows (unsplit) or slabs (split) take 4-column vector stores; with
N % 4 != 0, an unaligned C, a matrix bias or ``accumulate`` the planner gives such a request the LDS-staged ``8ph``
kernel. Those fall-backs are asserted where the epilogue matrix and the output views reach them; the N % 4 != 0
shapes of the sweep run on ``tile128``, ``8ph_lds``, ``8ph_pk`` and the stream tiles. ``8ph_fixup`` is a split-K
form and ``kinter`` only means something for a split launch, so neither has unsplit cases of its own (one unsplit
cfg 5 / 6 case asserts ``kinter`` false). The planner gives the in-launch fix-up and the packed kernel to unbatched
calls only, so the batched cases run on every other form (``BATCHABLE``). ``gemm_nt_segmented`` always runs one split per K segment or more: its
"unsplit" cases have one split per segment, its split case two.

Exact cases (no tolerance anywhere). A holds integers in [-4, 4], B integers in [-3, 3] times 0.25, the bias and
C0 multiples of 0.5 in [-4, 4]: all exact in bf16. alpha is one of 1, -2, 0.5 and dropout one of 0, 0.5, 0.75 (keep
scale exactly 2 or 4). Every product is a multiple of 0.25 of magnitude <= 3, so every partial sum, in any order
and under any split of K, is a multiple of 0.25 below 3 K + 4 < 2**22 (``_exact`` asserts it): at most 24
significant bits, f32 accumulation is exact. alpha, bias, keep scale and C0 keep the value a multiple of 0.125 below
2**16. Hence an f32 output must EQUAL the oracle and a bf16 output must equal ``oracle.to(bfloat16)``, the
round-to-nearest-even of an exact value. The comparison is by value with identical NaN positions.

sigmoid / exp / tanh. B is scaled by a further 2**-3 and K = 72, so the pre-activation s stays exact and
|s| <= 72 * 4 * 3/32 + 4 = 31. The output is compared with the float64 activation of s. The LDS-staged epilogue
(unsplit launches without ``direct_epi``) uses ``apply_act``: ``__expf`` = ``v_exp_f32(x * log2e)`` (argument
rounding |x| * 6e-8 plus 1 ulp), one division, ``tanhf``: the bounds tests/test_rowops.py derives for it, f32
``1e-5 * |ref| + 1e-30``. The reducers and the direct epilogues use ``apply_act_compact``: exp and sigmoid are the same
expressions with ``__frcp_rn`` for the division (same bound); tanh is ``2 * rcp(1 + t) - 1`` with t = exp(-2 v).
With x = |2 v| <= 62, t carries a relative error e_t <= x * 2**-24 + 2**-23 (argument rounding, instruction), and
s = rcp(1 + t) <= 1 carries e_t * t / (1 + t) plus 2 * 2**-24 (the sum and the reciprocal round). The absolute error
of 2 s - 1 is at most 2 * (e_t * t / (1 + t)**2 + 2 * 2**-24) and t / (1 + t)**2 <= min(1/4, exp(-x)), x * exp(-x) <=
1/e: at most (4 + 2 * (1/e + 1/2)) * 2**-24 < 6 * 2**-24, plus half an ulp of the result. The bound used is
``8 * 2**-24 + 2**-23 * |ref|``: an absolute term, because near v = 0 the subtraction cancels. bf16 outputs add
half a bf16 ulp: ``(2**-8 + 2**-16) * |ref|`` in place of the relative term.

Rounded data. A = randn and B = 0.1 * randn, both rounded to bf16 (the oracle reads the rounded values), f32 bias.
Products of two bf16 values are exact in f32, so only the additions round. With S the oracle evaluated on |A|, |B|,
|alpha|, |bias| (an upper bound of every partial sum's magnitude), each of the K accumulated terms, each of the
``splits`` slab additions, alpha, the bias and the store may cost one f32 ulp of the running magnitude:
``|y - ref| <= (K + splits + 4) * 2**-23 * S`` per element, in any summation order; bf16 output adds
``2**-8 * |ref|``. Derived, not measured; the worst err / bound per form, output dtype and device is printed in the
``GEMM_WORST`` line, the rounded-data and activation cases under ``rounded:<form>`` and ``<act>:<form>`` (exact
cases count 0, or inf when they fail).

Views. Operands are views ``big[r0 : r0 + rows, :K]`` of a parent with 5 more rows and 24 more columns whose other
elements are all NaN (batched: NaN gaps between the batches): a read past K, past the last row or before the first
one makes outputs NaN. Outputs are views ``wide[2 : 2 + M, c0 : c0 + N]`` of a buffer filled with a NaN-payload bit
pattern; every element outside the view must keep that pattern bit for bit.

Non-finite operands. ``A[i0, k0] = NaN`` and ``A[i1, k1] = +Inf`` where column k1 of B has no zero: row i0 of C is
NaN, row i1 is ``sign(alpha * B[j, k1]) * Inf``, every other row equals the finite oracle. With relu NaN stays NaN
(as ``torch.relu`` and the CPU path) and -Inf becomes 0.
"""
import collections
import functools
import json
import zlib

import numpy as np
import pytest
import torch

from netsdb_amd import ops

F32, BF16 = torch.float32, torch.bfloat16
DT = {"f32": F32, "bf16": BF16}
ACTS = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "sigmoid": ops.ACT_SIGMOID, "exp": ops.ACT_EXP,
        "tanh": ops.ACT_TANH}
MODES = {"none": ops.BIAS_NONE, "row": ops.BIAS_ROW, "col": ops.BIAS_COL, "mat": ops.BIAS_MAT}
BF16_RTOL = 2.0 ** -8 + 2.0 ** -16
GPU_MARK = pytest.mark.gpu
DEVS = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=GPU_MARK)]

# form -> the request (gemm_nt / gemm_plan options) and the kernel it names
FORMS = {
    "tile128": dict(cfg=0, kernel="tile128"),
    "8ph_lds": dict(cfg=2, epi=0, kernel="8ph"),
    "8ph_direct": dict(cfg=2, epi=1, kernel="8ph"),
    "8ph32": dict(cfg=2, mfma=32, kernel="8ph32"),
    "8ph_fixup": dict(cfg=2, fixup=1, kernel="8ph_fixup"),
    "8ph_pk_a": dict(cfg=2, epi=0, packed=1, kernel="8ph_pk"),
    "8ph_pk_b": dict(cfg=2, epi=0, packed=2, kernel="8ph_pk"),
    "stream256x128": dict(cfg=3, kernel="stream256x128"),
    "stream128x256": dict(cfg=4, kernel="stream128x256"),
    "stream256x128_ki": dict(cfg=5, kernel="stream256x128"),
    "stream128x256_ki": dict(cfg=6, kernel="stream128x256"),
}
SPLIT_ONLY = ("8ph_fixup", "stream256x128_ki", "stream128x256_ki")
EIGHT_PHASE = ("8ph_lds", "8ph_direct", "8ph32", "8ph_fixup", "8ph_pk_a", "8ph_pk_b")
# the in-launch fix-up and the packed kernel are planned for batch == 1 only
BATCHABLE = tuple(f for f in FORMS if f not in ("8ph_fixup", "8ph_pk_a", "8ph_pk_b"))

Epi = collections.namedtuple("Epi", "mode alpha act dropout seed acc", defaults=("none", 1.0, "none", 0.0, 0, False))

_WORST = {}                 # "[<kind>:]<form>/<out dtype>/<device>" -> worst err / bound seen in this run (exact: 0)
_PLANNED = []               # (id, gemm_plan arguments, the plan the case expects): every GPU case of the tables


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nGEMM_WORST " + json.dumps({k: float(f"{v:.3g}") for k, v in sorted(_WORST.items())}))


def _note(form, y, ratio):
    form = form if y.is_cuda or ":" in form else "cpu"
    key = f"{form}/{'f32' if y.dtype == F32 else 'bf16'}/{'gpu' if y.is_cuda else 'cpu'}"
    _WORST[key] = max(_WORST.get(key, 0.0), float(ratio))


# ---------------------------------------------------------------------------------------------------------- oracle

def _hash_uniform(seed, idx):
    """common.h hash_uniform, transcribed: a splitmix64 round of seed + idx * golden, the top 24 bits / 2**24."""
    mask = (1 << 64) - 1
    with np.errstate(over="ignore"):
        z = np.uint64(seed & mask) + idx.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float64) / 16777216.0


def _act64(v, act):
    if act == "relu":
        return torch.where(v < 0, torch.zeros_like(v), v)          # NaN stays NaN, -Inf becomes 0
    if act == "sigmoid":
        return 1 / (1 + torch.exp(-v))
    if act == "exp":
        return torch.exp(v)
    if act == "tanh":
        return torch.tanh(v)
    return v


def _oracle(A, B, bias=None, mode="none", alpha=1.0, act="none", dropout=0.0, seed=0, C0=None):
    y = A.double() @ B.double().transpose(-1, -2)
    y = y * alpha
    if mode == "row":
        y = y + bias.double().unsqueeze(-1)
    elif mode == "col":
        y = y + bias.double().unsqueeze(-2)
    elif mode == "mat":
        y = y + bias.double()
    y = _act64(y, act)
    if dropout > 0:
        batch = y.shape[0] if y.dim() == 3 else 1
        M, N = y.shape[-2:]
        b = np.arange(batch, dtype=np.uint64)[:, None, None]
        r = np.arange(M, dtype=np.uint64)[None, :, None]
        c = np.arange(N, dtype=np.uint64)[None, None, :]
        u = _hash_uniform(seed, (b * np.uint64(M) + r) * np.uint64(N) + c)
        keep = torch.from_numpy(u >= dropout).reshape(y.shape)
        y = torch.where(keep, y * (1.0 / (1.0 - dropout)), torch.zeros_like(y))
    if C0 is not None:
        y = y + C0.double()
    return y


def test_hash_uniform_transcription_matches_the_host_twin():
    """The oracle's own transcription against the package's host twin (both claim to be common.h hash_uniform)."""
    idx = np.concatenate([np.arange(4096, dtype=np.uint64), np.uint64(2 ** 33) + np.arange(64, dtype=np.uint64)])
    for seed in (0, 99, 2 ** 32 + 12345, 2 ** 40 + 7):
        mine = _hash_uniform(seed, idx)
        assert np.array_equal(mine, ops.hash_uniform(seed, idx).astype(np.float64))
        assert 0.3 < float((mine < 0.5).mean()) < 0.7


# ------------------------------------------------------------------------------------------------------------ data

def _gen(*key):
    """A generator seeded by the key alone (crc32 of its repr: the same data in every process)."""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def _exact(M, N, K, batch=0, wshift=0):
    """Integer-valued operands (see the module docstring): A bf16 [.., M, K], B bf16 [.., N, K]."""
    assert 3 * K + 4 < 2 ** 22
    g = _gen(M, N, K, batch, wshift)
    pre = (batch,) if batch else ()
    A = torch.randint(-4, 5, pre + (M, K), generator=g).to(BF16)
    B64 = torch.randint(-3, 4, pre + (N, K), generator=g).double() * (0.25 * 2.0 ** -wshift)
    B = B64.to(BF16)
    assert torch.equal(B.double(), B64)
    return A, B


@functools.lru_cache(maxsize=None)
def _halves(*shape):
    """Multiples of 0.5 in [-4, 4], f32 (a bias or C0)."""
    return torch.randint(-8, 9, shape, generator=_gen("h", *shape)).float() * 0.5


def _bias_for(mode, M, N, batch=0, shared=True):
    pre = (batch,) if batch and not shared else ()
    if mode == "none":
        return None
    return _halves(*(pre + {"row": (M,), "col": (N,), "mat": (M, N)}[mode]))


def _align(t):
    a = t.data_ptr() | 16
    return a & -a


# ---------------------------------------------------------------------------------------------------------- plans

def _want(form, N, splits, reducer, staged_only=False, vec_c=None):
    """The plan a case expects, from the rules gemm_plan.h documents: the direct epilogue needs 4-column vector
    stores (C rows when unsplit, slabs when split) and, unsplit, neither C += nor a matrix bias; 8ph32 and the
    in-launch reducer need the direct epilogue; kinter needs a split launch."""
    req = FORMS[form]
    vec_ws = N % 4 == 0
    vec_c = vec_ws if vec_c is None else vec_c
    direct = False
    kernel = req["kernel"]
    if form in EIGHT_PHASE:
        asks = req.get("epi", -1) != 0
        direct = asks and ((splits == 1 and not staged_only and vec_c) or (splits > 1 and vec_ws))
        if form == "8ph32" and not direct:
            kernel = "8ph"
        if form == "8ph_fixup" and not (direct and splits > 1 and reducer == "in_launch"):
            kernel = "8ph"
    return dict(kernel=kernel, splits=splits, reducer=reducer if splits > 1 else "none", direct_epi=direct,
                kinter=req["cfg"] >= 5 and splits > 1, packed=req.get("packed", 0) if kernel == "8ph_pk" else 0)


def _plan_args(form, M, N, K, batch, splits, yout, e, ldc=None, c_align=16):
    req = FORMS[form]
    return dict(M=M, N=N, K=K, batch=max(batch, 1), splits=splits, cfg=req["cfg"], epi=req.get("epi"),
                mfma=req.get("mfma", 16), fixup=req.get("fixup", 0), out_dtype=DT[yout], accumulate=e.acc,
                bias_mode=MODES[e.mode], ldc=ldc, c_align=c_align, packed=req.get("packed", 0))


def _assert_plan(args, want, what=""):
    got = ops.gemm_plan(**args)
    assert {k: got[k] for k in want} == want, f"{what}: planned {got}, the case is meant for {want}"


def _gemm(dev, form, A, B, bias, e, splits, yout, want, out=None):
    """ops.gemm_nt on tensors that already live on ``dev``; on the GPU the planner must first confirm ``want``."""
    kw = dict(bias=bias, bias_mode=MODES[e.mode], act=ACTS[e.act], out_dtype=DT[yout], alpha=e.alpha,
              dropout=e.dropout, seed=e.seed, out=out, accumulate=e.acc)
    if dev == "cuda":
        req = FORMS[form]
        M, N, K = A.shape[-2], B.shape[-2], A.shape[-1]
        batch = A.shape[0] if A.dim() == 3 else 0
        ldc, c_align = (out.stride(-2), _align(out)) if out is not None else (None, 16)
        _assert_plan(_plan_args(form, M, N, K, batch, splits, yout, e, ldc, c_align), want, form)
        kw.update(splits=splits, cfg=req["cfg"], epi=req.get("epi"), mfma=req.get("mfma", 16),
                  fixup=req.get("fixup", 0))
        if req.get("packed") == 1:
            kw["a_packed"] = ops.pack_ktile(A)
        elif req.get("packed") == 2:
            kw["b_packed"] = ops.pack_ktile(B)
    y = ops.gemm_nt(A, B, **kw)
    assert y.dtype == DT[yout] and y.device.type == dev
    return y


def _check_exact(form, y, ref):
    """y == ref (f32 output) or y == ref.to(bf16) (bf16 output) at every element, NaN where and only where the
    oracle has NaN: no tolerance."""
    assert tuple(y.shape) == tuple(ref.shape), (tuple(y.shape), tuple(ref.shape))
    want = ref.to(y.dtype).double()
    got = y.detach().cpu().double()
    bad = (got != want) & ~(got.isnan() & want.isnan())
    _note(form, y, float("inf") if bad.any() else 0.0)
    if bad.any():
        at = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(
            f"{form}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result; first at {at}: got "
            f"{float(got[at])!r}, oracle {float(ref[at])!r} (-> {float(want[at])!r}); rows "
            f"{sorted(set(bad.nonzero()[:, -2].tolist()))[:8]}, columns "
            f"{sorted(set(bad.nonzero()[:, -1].tolist()))[:8]}")


def _check_bound(form, y, ref, bound, kind):
    """|y - ref| <= bound elementwise (finite oracle); reports the worst element (GEMM_WORST key "<kind>:<form>")."""
    got = y.detach().cpu().double()
    assert ref.isfinite().all()
    assert got.isfinite().all(), f"{form}: non-finite output at {got.isfinite().logical_not().nonzero()[0].tolist()}"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    w = tuple((ratio == ratio.max()).nonzero()[0].tolist())
    _note(f"{kind}:{form if y.is_cuda else 'cpu'}", y, float(ratio[w]))
    assert float(ratio[w]) <= 1.0, (
        f"{form}: worst element {w}: got {float(got[w])!r}, oracle {float(ref[w])!r}, err {float(err[w]):.3e} > "
        f"bound {float(bound[w]):.3e}")


# ------------------------------------------------------------------------------------------------- the exact cases

# (M, N, K, splits, reducer): one past / one short of a tile edge, the N % 4 pair, K below / at / ragged after 1, 2, 8
# k-tiles, a short last split (K 520 = 9 k-tiles in 3 x 3, the last one 8 wide), a split of one ragged k-tile (K 136 in
# 2 + 1), one split per k-tile (9: the wide reducer when N % 4 == 0 and the output is small, else the plain one)
SHAPES_128 = [
    (127, 132, 8, 1, "none"), (129, 130, 64, 1, "none"), (257, 129, 72, 1, "none"), (129, 260, 136, 1, "none"),
    (257, 258, 520, 1, "none"), (127, 128, 72, 1, "none"), (129, 127, 136, 1, "none"), (257, 255, 72, 1, "none"),
    (129, 127, 520, 3, "plain"), (127, 255, 136, 2, "plain"),      # N % 4 == 3: a last 4-column group of 3
    (129, 132, 520, 3, "plain"), (127, 130, 520, 3, "plain"), (257, 132, 136, 2, "plain"),
    (129, 257, 136, 2, "plain"), (129, 132, 520, 9, "wide"), (129, 130, 520, 9, "plain"),
    (1157, 300, 72, 1, "none"),        # 10 x 3 tiles: the partial last group of grouped_tile, xcd_remap's remainder
]
SHAPES_256_VEC = [
    (255, 516, 8, 1, "none"), (255, 260, 64, 1, "none"), (513, 260, 72, 1, "none"), (257, 516, 136, 1, "none"),
    (257, 256, 520, 1, "none"),
    (257, 516, 520, 3, "plain"), (513, 516, 136, 2, "plain"), (255, 260, 520, 9, "wide"),
    (2309, 516, 72, 1, "none"),        # 10 x 3 tiles
]
SHAPES_256_ODD = [
    (257, 514, 64, 1, "none"), (255, 258, 520, 1, "none"), (513, 257, 72, 1, "none"),
    (255, 514, 520, 3, "plain"), (257, 514, 136, 2, "plain"), (257, 258, 520, 9, "plain"),
    (257, 255, 136, 1, "none"), (513, 511, 72, 1, "none"), (257, 255, 520, 3, "plain"), (255, 511, 136, 2, "plain"),
]
SHAPES_S3 = [                          # 256 x 128 tiles
    (255, 8, 72, 1, "none"), (257, 132, 8, 1, "none"), (255, 130, 64, 1, "none"), (513, 127, 136, 1, "none"),
    (257, 129, 520, 1, "none"),
    (257, 132, 520, 3, "plain"), (255, 130, 520, 3, "plain"), (513, 8, 136, 2, "plain"), (257, 127, 136, 2, "plain"),
    (255, 132, 520, 9, "wide"), (257, 130, 520, 9, "plain"),
    (2309, 300, 72, 1, "none"),        # 10 x 3 tiles
]
SHAPES_S4 = [                          # 128 x 256 tiles
    (127, 8, 72, 1, "none"), (129, 260, 8, 1, "none"), (127, 258, 64, 1, "none"), (129, 255, 136, 1, "none"),
    (257, 513, 520, 1, "none"),
    (129, 516, 520, 3, "plain"), (127, 514, 520, 3, "plain"), (129, 8, 136, 2, "plain"), (127, 257, 136, 2, "plain"),
    (129, 260, 520, 9, "wide"), (127, 258, 520, 9, "plain"),
    (1157, 516, 72, 1, "none"),        # 10 x 3 tiles
]
# one ragged shape per form (M, N, K): the epilogue matrix, the views, the non-finite, rounded and activation cases
RAGGED = {f: (129, 132) for f in ("tile128",)}
RAGGED.update({f: (257, 260) for f in EIGHT_PHASE})
RAGGED.update({"stream256x128": (257, 132), "stream256x128_ki": (257, 132),
               "stream128x256": (129, 260), "stream128x256_ki": (129, 260)})

COLB = Epi(mode="col")
_EXACT_CASES = []
_CPU_IDS = set()


def _register(table, cid, values, plan_args, want, cpu_id=None):
    """One GPU case of ``table``: its pytest param (device first, the expected plan last) and its ``_PLANNED`` entry,
    which ``test_case_table_reaches_every_kernel_and_reducer`` checks; with ``cpu_id``, the CPU-fallback twin of the
    same values, once per id and table (the CPU path has no forms and no splits)."""
    table.append(pytest.param("cuda", *values, want, id=cid + "-gpu", marks=GPU_MARK))
    _PLANNED.append((cid, plan_args, want))
    if cpu_id is not None and (id(table), cpu_id) not in _CPU_IDS:
        _CPU_IDS.add((id(table), cpu_id))
        table.append(pytest.param("cpu", *values, None, id=cpu_id))


def _per_form(Ks):
    """(form, M, N, K, splits, reducer) on the form's ragged shape for every (K, splits) of ``Ks`` the form takes."""
    for form, (M, N) in RAGGED.items():
        for K, splits in Ks:
            if form in SPLIT_ONLY and splits == 1:
                continue
            yield form, M, N, K, splits, "in_launch" if form == "8ph_fixup" else "plain"


def _eid(e):
    s = e.mode
    if e.alpha != 1.0:
        s += f"_a{e.alpha:g}"
    if e.act != "none":
        s += "_" + e.act
    if e.dropout:
        s += f"_p{e.dropout:g}"
    return s + ("_acc" if e.acc else "")


def _add(form, M, N, K, splits, reducer, youts=("f32", "bf16"), e=COLB, batch=0, bshare=False, bias_shared=True):
    """One GPU case per output dtype; the CPU fallback (which has no forms and no splits) once per problem."""
    staged_only = e.mode == "mat" or e.acc
    want = _want(form, N, splits, reducer, staged_only)
    for yout in youts:
        cid = (f"{M}x{N}x{K}" + (f"_b{batch}" if batch else "") + ("_bshare" if bshare else "")
               + ("" if bias_shared else "_biasb") + f"-{_eid(e)}-{yout}")
        prob = (M, N, K, e, yout, batch, bshare, bias_shared)
        _register(_EXACT_CASES, f"{form}-s{splits}-{cid}", (form, prob, splits),
                  _plan_args(form, M, N, K, batch, splits, yout, e), want, cpu_id=f"cpu-{cid}")


EPILOGUES = [
    Epi(mode="none"), Epi(mode="row", alpha=-2.0), Epi(mode="col", alpha=0.5, act="relu"), Epi(mode="mat", act="relu"),
    Epi(mode="mat", alpha=0.5, dropout=0.5, seed=2 ** 32 + 12345),
    Epi(mode="row", act="relu", dropout=0.75, seed=2 ** 40 + 7),
    Epi(mode="none", alpha=-2.0, dropout=0.5, seed=2 ** 33 + 1),
]
ACC_EPILOGUES = [Epi(mode="none", acc=True),
                 Epi(mode="col", alpha=0.5, act="relu", dropout=0.5, seed=2 ** 32 + 5, acc=True)]


def _build_exact_cases():
    sweep = {"tile128": SHAPES_128, "8ph_lds": SHAPES_256_VEC + SHAPES_256_ODD, "8ph_direct": SHAPES_256_VEC,
             "8ph32": SHAPES_256_VEC, "8ph_fixup": SHAPES_256_VEC, "stream256x128": SHAPES_S3,
             "stream128x256": SHAPES_S4, "stream256x128_ki": SHAPES_S3, "stream128x256_ki": SHAPES_S4}
    for form, shapes in sweep.items():
        unsplit_done = False
        for M, N, K, splits, reducer in shapes:
            if form == "8ph_fixup":
                if splits == 1 or splits >= 8:      # the in-launch reducer: split launches below 8 splits here
                    continue
                reducer = "in_launch"
            elif form in SPLIT_ONLY and splits == 1:
                if unsplit_done:                    # one unsplit cfg 5 / 6 case: the plan says kinter false
                    continue
                unsplit_done = True
            _add(form, M, N, K, splits, reducer)
    # the packed forms: tests/test_gemm_packed_gpu.py covers them; one unsplit and one split case per side
    _add("8ph_pk_a", 257, 516, 136, 1, "none")
    _add("8ph_pk_a", 255, 514, 520, 3, "plain")
    _add("8ph_pk_b", 513, 257, 72, 1, "none")
    _add("8ph_pk_b", 257, 516, 520, 3, "plain")
    # the epilogue matrix on one ragged shape per form, unsplit and split (K 520 = 8 k-tiles + a ragged one, in
    # 3 + 3 + 3; long enough that results pass 64 = 2**8 * 0.25 and a bf16 output has bits to round)
    for form, (M, N) in RAGGED.items():
        for splits in (1, 3):
            if form in SPLIT_ONLY and splits == 1:
                continue
            reducer = "in_launch" if form == "8ph_fixup" else "plain"
            for e in EPILOGUES:
                _add(form, M, N, 520, splits, reducer, e=e)
            for e in ACC_EPILOGUES:
                _add(form, M, N, 520, splits, reducer, youts=("f32",), e=e)
    # the scalar paths of the plain reducer and of the LDS-staged store (N % 4 != 0) under alpha, bias, dropout
    for e in EPILOGUES[1:5] + ACC_EPILOGUES[1:]:
        for splits in (1, 3):
            _add("tile128", 129, 130, 520, splits, "plain", youts=("f32",) if e.acc else ("f32", "bf16"), e=e)
            _add("8ph_lds", 257, 258, 520, splits, "plain", youts=("f32",) if e.acc else ("f32", "bf16"), e=e)
    # the wide reducer (one split per k-tile, N % 4 == 0, a small output) under alpha, bias, dropout and C +=
    for form, (M, N) in (("tile128", (129, 132)), ("8ph_lds", (257, 260)), ("stream256x128_ki", (257, 132))):
        _add(form, M, N, 520, 9, "wide", e=EPILOGUES[4])
        _add(form, M, N, 520, 9, "wide", youts=("f32",), e=ACC_EPILOGUES[1])
    # batched: 3 problems with their own A and B, B broadcast with stride 0, bias per batch / shared, dropout 0.5
    # (the batch term of the element index)
    drop = Epi(mode="col", dropout=0.5, seed=2 ** 32 + 77)
    for form in BATCHABLE:
        M, N = RAGGED[form]
        for splits in (1, 2):
            if form in SPLIT_ONLY and splits == 1:
                continue
            _add(form, M, N, 136, splits, "plain", e=drop, batch=3, bias_shared=False)
            _add(form, M, N, 136, splits, "plain", youts=("f32",), e=Epi(mode="row", alpha=-2.0), batch=3, bshare=True)
            _add(form, M, N, 136, splits, "plain", youts=("bf16",), e=Epi(mode="mat", act="relu"), batch=3,
                 bias_shared=False)
            _add(form, M, N + 1, 72, splits, "plain", youts=("f32",), e=drop, batch=3)


_build_exact_cases()


def _problem(prob):
    """CPU tensors of an exact problem: A, B, bias, C0 and the oracle."""
    M, N, K, e, yout, batch, bshare, bias_shared = prob
    A, B = _exact(M, N, K, batch)
    if bshare:
        B = B[0].unsqueeze(0).expand(batch, N, K)           # one B for every batch: stride 0
    bias = _bias_for(e.mode, M, N, batch, bias_shared)
    C0 = _halves(*(((batch,) if batch else ()) + (M, N, 2)))[..., 0].contiguous() if e.acc else None
    ref = _oracle(A, B, bias, e.mode, e.alpha, e.act, e.dropout, e.seed, C0)
    return A, B, bias, C0, ref


@pytest.mark.parametrize("dev,form,prob,splits,want", _EXACT_CASES)
def test_gemm_exact(dev, form, prob, splits, want):
    e, yout, bshare = prob[3], prob[4], prob[6]
    A, B, bias, C0, ref = _problem(prob)
    Bd = B[0].to(dev).unsqueeze(0).expand(B.shape) if bshare else B.to(dev)
    if bshare:
        assert Bd.stride(0) == 0
    out = C0.clone().to(dev) if e.acc else None
    y = _gemm(dev, form, A.to(dev), Bd, None if bias is None else bias.to(dev), e, splits, yout, want, out)
    _check_exact(form, y, ref)
    if form == "8ph_fixup" and dev == "cuda":
        # the in-launch reduction leaves its arrival words zero: a second launch gives the same bits
        out2 = C0.clone().to(dev) if e.acc else None
        y2 = _gemm(dev, form, A.to(dev), Bd, None if bias is None else bias.to(dev), e, splits, yout, want, out2)
        assert torch.equal(y2.view(torch.int32 if yout == "f32" else torch.int16),
                           y.view(torch.int32 if yout == "f32" else torch.int16))


def test_exact_data_is_exact_and_dropout_drops():
    """The claims the exact cases rest on: the oracle of an exact problem holds multiples of 0.125 below 2**16 (exact
    in f32); a dropout case has dropped and kept elements; and at K = 520 a bf16 output has values to round, some of
    which truncation would get wrong."""
    A, B = _exact(129, 132, 520)
    e = EPILOGUES[4]
    ref = _oracle(A, B, _bias_for("mat", 129, 132), e.mode, e.alpha, e.act, e.dropout, e.seed)
    assert torch.equal(ref * 8, (ref * 8).round()) and float(ref.abs().max()) < 2 ** 16
    assert torch.equal(ref.float().double(), ref)
    raw = _oracle(A, B, _bias_for("mat", 129, 132), e.mode, e.alpha, e.act)
    dropped = ((ref == 0) & (raw != 0)).float().mean()
    assert 0.3 < float(dropped) < 0.7 and torch.equal(ref[ref != 0], 2 * raw[ref != 0])
    rne = ref.to(BF16).double()
    trunc = (ref.float().view(torch.int32) & -65536).view(F32).double()
    assert int((rne != ref).sum()) > 100 and int((rne != trunc).sum()) > 50


def test_case_table_reaches_every_kernel_and_reducer():
    """Every GPU case of the tables gets the plan it names (the planner is host arithmetic: no GPU needed to ask),
    and together they reach all seven kernels and all four reducers of gemm_plan.h, each kernel with both output
    dtypes."""
    seen = collections.defaultdict(set)
    reducers = set()
    for cid, args, want in _PLANNED:
        _assert_plan(args, want, cid)
        seen[want["kernel"]].add(args["out_dtype"])
        reducers.add(want["reducer"])
        if want["kernel"].startswith("stream"):
            seen[(want["kernel"], want["kinter"])].add(args["out_dtype"])
    kernels = {"tile128", "8ph", "8ph32", "8ph_fixup", "stream256x128", "stream128x256", "8ph_pk"}
    assert {k for k in seen if isinstance(k, str)} == kernels
    assert reducers == {"none", "plain", "wide", "in_launch"}
    for k, dts in seen.items():
        assert dts == {F32, BF16}, (k, dts)
    for k in ("stream256x128", "stream128x256"):
        assert (k, True) in seen and (k, False) in seen
    assert {w["packed"] for _, _, w in _PLANNED} == {0, 1, 2}
    assert {(w["kernel"], w["direct_epi"]) for _, _, w in _PLANNED} >= {("8ph", True), ("8ph", False)}


# --------------------------------------------------------------------------------------------------- segmented B

# S, seg_k, M, N, the splits the binding picks (one per segment; two where the launch would split that far by itself)
SEG_CASES = [(2, 64, 129, 130, 2), (3, 64, 127, 132, 3), (2, 128, 129, 132, 2), (3, 128, 257, 129, 3),
             (2, 1024, 129, 130, 4)]


@pytest.mark.parametrize("yout", ["f32", "bf16"])
@pytest.mark.parametrize("S,segk,M,N,splits", SEG_CASES, ids=[f"S{c[0]}_k{c[1]}_{c[2]}x{c[3]}" for c in SEG_CASES])
@pytest.mark.parametrize("dev", DEVS)
def test_gemm_segmented_exact(dev, S, segk, M, N, splits, yout):
    """B held as [S, N, seg_k] (segment s = columns s * seg_k .. of every row), walked in place."""
    K = S * segk
    A, B = _exact(M, N, K)
    Bg = B.view(N, S, segk).permute(1, 0, 2).contiguous()
    bias = _bias_for("col", M, N)
    e = Epi(mode="col", act="relu", dropout=0.5, seed=2 ** 32 + 9)
    if dev == "cuda":
        # the binding's request: S x d splits, d | seg_k / 64, S * d <= max(the launch's own choice, S)
        auto = ops.gemm_plan(M, N, K, out_dtype=DT[yout], bias_mode=ops.BIAS_COL)["splits"]
        d = max(c for c in range(1, segk // 64 + 1) if (segk // 64) % c == 0 and S * c <= max(auto, S))
        assert S * d == splits
        got = ops.gemm_plan(M, N, K, splits=splits, out_dtype=DT[yout], bias_mode=ops.BIAS_COL, seg_k=segk)
        want = dict(kernel="tile128", splits=splits, reducer="plain", direct_epi=False, kinter=False, packed=0)
        assert {k: got[k] for k in want} == want
    y = ops.gemm_nt_segmented(A.to(dev), Bg.to(dev), bias.to(dev), ops.BIAS_COL, ACTS[e.act], DT[yout],
                              dropout=e.dropout, seed=e.seed)
    _check_exact("segmented", y, _oracle(A, B, bias, e.mode, e.alpha, e.act, e.dropout, e.seed))


# ----------------------------------------------------------------------------------------------------- operand views

def _nan_parent(X, r0=2, aligned=True):
    """X as the view big[.., r0 : r0 + rows, :K] of a parent with 5 more rows and 24 more columns, NaN elsewhere."""
    rows, K = X.shape[-2:]
    big = torch.full(X.shape[:-2] + (rows + 5, K + 24), float("nan"), dtype=X.dtype)
    big[..., r0:r0 + rows, :K] = X
    # 16-B rows: every row of the view is 16-B aligned and the kernels read it in place
    assert (big.stride(-2) * big.element_size()) % 16 == 0 or not aligned
    return big, (lambda t: t[..., r0:r0 + rows, :K])


def _view_cases():
    table = []
    for form, M, N, K, splits, reducer in _per_form(((72, 1), (136, 2))):
        for batch in (0, 3):
            if batch and form not in BATCHABLE:
                continue
            cid = f"{form}-s{splits}-{M}x{N}x{K}" + (f"_b{batch}" if batch else "") + "-view"
            _register(table, cid, (form, M, N, K, splits, batch), _plan_args(form, M, N, K, batch, splits, "f32", COLB),
                      _want(form, N, splits, reducer), cpu_id=f"cpu-{M}x{N}x{K}_b{batch}")
    return table


_VIEW_CASES = _view_cases()


@pytest.mark.parametrize("dev,form,M,N,K,splits,batch,want", _VIEW_CASES)
def test_gemm_operand_views_surrounded_by_nan(dev, form, M, N, K, splits, batch, want):
    """A partial k-tile sits next to NaN in the same row, the rows before and past the view are NaN: any read the
    kernels do not clip with k < kend / row < rows_valid makes an output NaN."""
    A, B = _exact(M, N, K, batch)
    bias = _bias_for("col", M, N)
    bigA, va = _nan_parent(A)
    bigB, vb = _nan_parent(B, r0=3)
    Ad, Bd = va(bigA.to(dev)), vb(bigB.to(dev))
    assert torch.equal(Ad.cpu(), A) and not Ad.is_contiguous() and Ad.stride(-2) == K + 24
    ref = _oracle(A, B, bias, "col")
    assert ref.isfinite().all()
    for yout in ("f32", "bf16"):
        y = _gemm(dev, form, Ad, Bd, bias.to(dev), COLB, splits, yout, want)
        _check_exact(form, y, ref)


# ------------------------------------------------------------------------------------------------------ output views

SENTINEL = {"f32": (torch.int32, 0x7FC12345), "bf16": (torch.int16, 0x7FC5)}


def _out_cases():
    table = []
    for form, M, N, K, splits, reducer in _per_form(((136, 1), (136, 2))):
        for pad, c0, vec_c in ((12, 4, True), (13, 3, False), (12, 3, False)):
            for yout, acc in (("f32", False), ("bf16", False), ("f32", True)):
                case = (form, M, N, splits, reducer, pad, c0, vec_c, yout, acc)
                e = Epi(mode="row", alpha=0.5, dropout=0.5, seed=2 ** 32 + 21, acc=acc)   # the index has N, not ldc
                cid = f"{form}-s{splits}-{M}x{N}-ldc+{pad}_c{c0}-{yout}" + ("-acc" if acc else "")
                off = (2 * (N + pad) + c0) * (4 if yout == "f32" else 2)     # the view's byte offset in its buffer
                args = _plan_args(form, M, N, K, 0, splits, yout, e, N + pad, (off | 16) & -(off | 16))
                _register(table, cid, (case, e), args, _want(form, N, splits, reducer, staged_only=acc, vec_c=vec_c),
                          cpu_id=f"cpu-{M}x{N}-ldc+{pad}_c{c0}-{yout}" + ("-acc" if acc else ""))
    return table


_OUT_CASES = _out_cases()


@pytest.mark.parametrize("dev,case,e,want", _OUT_CASES)
def test_gemm_output_view_keeps_the_sentinel(dev, case, e, want):
    """out = wide[2 : 2 + M, c0 : c0 + N]: the view gets the exact result (alpha, row bias, dropout whose element
    index counts N columns per row while the rows of C are ldc apart; + C0 under accumulate), and every other
    element of the buffer keeps its bit pattern: rows below M, rows above, the columns on both sides, for aligned
    rows (4-column vector stores) and misaligned ones (odd row stride or a 3-element column offset)."""
    form, M, N, splits, reducer, pad, c0, vec_c, yout, acc = case
    K = 136
    A, B = _exact(M, N, K)
    bias = _bias_for("row", M, N)
    C0 = _halves(M, N, 3)[..., 0].contiguous() if acc else None
    ref = _oracle(A, B, bias, e.mode, e.alpha, e.act, e.dropout, e.seed, C0)
    ity, pattern = SENTINEL[yout]
    ldc = N + pad
    wide = torch.full((M + 4, ldc), pattern, dtype=ity).view(DT[yout]).to(dev)
    out = wide[2:2 + M, c0:c0 + N]
    if acc:
        out.copy_(C0)
    if dev == "cuda":
        assert (ldc % 4 == 0 and _align(out) % (16 if yout == "f32" else 8) == 0) == vec_c
    y = _gemm(dev, form, A.to(dev), B.to(dev), bias.to(dev), e, splits, yout, want, out)
    assert y.data_ptr() == out.data_ptr()
    _check_exact(form, out, ref)
    bits = wide.cpu().view(ity).clone()
    bits[2:2 + M, c0:c0 + N] = pattern
    bad = bits != pattern
    assert not bad.any(), (f"{form}: {int(bad.sum())} elements outside the output view were overwritten, first at "
                           f"{bad.nonzero()[0].tolist()} (the view is rows 2..{M + 1}, columns {c0}..{c0 + N - 1})")


# ------------------------------------------------------------------------------------------------ non-finite operands

def _nf_cases():
    table = []
    for form, M, N, K, splits, reducer in _per_form(((136, 1), (136, 2))):
        # (act, alpha, k0 of the NaN, k1 of the Inf): k0 = 130 lies in the ragged last k-tile of K = 136
        for act, alpha, k0, k1 in (("none", 1.0, 5, 70), ("none", -2.0, 130, 3), ("relu", -2.0, 130, 64)):
            case = (form, M, N, splits, reducer, act, alpha, k0, k1)
            args = _plan_args(form, M, N, K, 0, splits, "f32", Epi(mode="col", alpha=alpha, act=act))
            _register(table, f"{form}-s{splits}-{act}_a{alpha:g}_k{k0}", (case,), args, _want(form, N, splits, reducer),
                      cpu_id=f"cpu-{M}x{N}-{act}_a{alpha:g}_k{k0}")
    return table


_NF_CASES = _nf_cases()


@pytest.mark.parametrize("dev,case,want", _NF_CASES)
def test_gemm_nonfinite_operands(dev, case, want):
    form, M, N, splits, reducer, act, alpha, k0, k1 = case
    K = 136
    A0, B0 = _exact(M, N, K)
    i0, i1 = 3, M - 1                 # the first and the last row tile (the last row of C)
    A, B = A0.clone(), B0.clone()
    B[:, k1] = torch.where(B[:, k1] == 0, torch.full_like(B[:, k1], 0.25), B[:, k1])
    A[i0, k0] = float("nan")
    A[i1, k1] = float("inf")
    bias = _bias_for("col", M, N)
    e = Epi(mode="col", alpha=alpha, act=act)
    ref = _oracle(A, B, bias, e.mode, e.alpha, e.act)
    # the oracle has the shape the definition gives it
    fin = A.clone()
    fin[i0, k0] = 0
    fin[i1, k1] = 0
    clean = _oracle(fin, B, bias, e.mode, e.alpha, e.act)
    rows = torch.ones(M, dtype=torch.bool)
    rows[[i0, i1]] = False
    assert ref[i0].isnan().all() and torch.equal(ref[rows], clean[rows]) and clean.isfinite().all()
    inf_row = torch.sign(alpha * B[:, k1].double()) * float("inf")
    assert torch.equal(ref[i1], _act64(inf_row, act))
    if act == "relu":
        assert (ref[i1] == 0).any() and (ref[i1] == float("inf")).any()
    for yout in ("f32", "bf16"):
        y = _gemm(dev, form, A.to(dev), B.to(dev), bias.to(dev), e, splits, yout, want)
        _check_exact(form, y, ref)


# ------------------------------------------------------------------------------------------------------- rounded data

@functools.lru_cache(maxsize=None)
def _rounded(M, N, K):
    g = _gen("r", M, N, K)
    A = torch.randn(M, K, generator=g).to(BF16)
    B = (0.1 * torch.randn(N, K, generator=g)).to(BF16)
    bias = torch.randn(N, generator=g)
    return A, B, bias


def _dtype_cases(Ks, tag):
    """Every form on its ragged shape, each (K, splits) of ``Ks``, both output dtypes."""
    table = []
    for form, M, N, K, splits, reducer in _per_form(Ks):
        for yout in ("f32", "bf16"):
            _register(table, f"{form}-s{splits}-{M}x{N}x{K}-{yout}-{tag}", (form, M, N, K, splits, yout),
                      _plan_args(form, M, N, K, 0, splits, yout, COLB), _want(form, N, splits, reducer),
                      cpu_id=f"cpu-{M}x{N}x{K}-{yout}")
    return table


_ROUNDED_CASES = _dtype_cases(((520, 1), (520, 3)), "rounded")


@pytest.mark.parametrize("dev,form,M,N,K,splits,yout,want", _ROUNDED_CASES)
def test_gemm_rounded_data(dev, form, M, N, K, splits, yout, want):
    A, B, bias = _rounded(M, N, K)
    alpha = -2.0
    e = Epi(mode="col", alpha=alpha)
    ref = _oracle(A, B, bias, "col", alpha)
    S = _oracle(A.abs(), B.abs(), bias.abs(), "col", abs(alpha))
    bound = (K + splits + 4) * 2.0 ** -23 * S
    if yout == "bf16":
        bound = bound + 2.0 ** -8 * ref.abs()
    y = _gemm(dev, form, A.to(dev), B.to(dev), bias.to(dev), e, splits, yout, want)
    _check_bound(form, y, ref, bound, "rounded")


# -------------------------------------------------------------------------------------------------------- activations

_ACT_CASES = _dtype_cases(((72, 1), (72, 2)), "act")


@pytest.mark.parametrize("act", ["sigmoid", "exp", "tanh"])
@pytest.mark.parametrize("dev,form,M,N,K,splits,yout,want", _ACT_CASES)
def test_gemm_activation(dev, form, M, N, K, splits, yout, want, act):
    """An exact pre-activation (B scaled by 2**-3, |s| <= 31) through sigmoid / exp / tanh, under the bounds the
    module docstring derives from apply_act (LDS-staged unsplit epilogue) and apply_act_compact (reducers, direct
    epilogues)."""
    A, B = _exact(M, N, K, 0, 3)
    bias = _bias_for("col", M, N)
    s = _oracle(A, B, bias, "col")
    assert float(s.abs().max()) <= 31 and torch.equal(s.float().double(), s)
    ref = _act64(s, act)
    compact = dev == "cuda" and (splits > 1 or want["direct_epi"])
    rtol = BF16_RTOL if yout == "bf16" else 1e-5
    bound = rtol * ref.abs() + 1e-30
    if act == "tanh" and compact:
        bound = (BF16_RTOL if yout == "bf16" else 2.0 ** -23) * ref.abs() + 8 * 2.0 ** -24
    y = _gemm(dev, form, A.to(dev), B.to(dev), bias.to(dev), Epi(mode="col", act=act), splits, yout, want)
    _check_bound(form, y, ref, bound, act)


# ------------------------------------------------------------------------------------------------- the exact-f32 GEMM

@functools.lru_cache(maxsize=None)
def _exact_f32(M, N, K):
    """Integers in [-64, 64] and [-32, 32]: products below 2**11, every partial sum below K * 2**11 < 2**24."""
    assert K * 2 ** 11 < 2 ** 24
    g = _gen("f", M, N, K)
    return torch.randint(-64, 65, (M, K), generator=g).float(), torch.randint(-32, 33, (N, K), generator=g).float()


F32_SHAPES = [(1, 1, 4), (17, 33, 20), (129, 257, 516), (1500, 4, 8)]


@pytest.mark.parametrize("acc", [False, True], ids=["store", "acc"])
@pytest.mark.parametrize("alpha", [1.0, -2.0, 0.5])
@pytest.mark.parametrize("M,N,K", F32_SHAPES)
@pytest.mark.parametrize("dev", DEVS)
def test_gemm_f32_exact(dev, M, N, K, alpha, acc):
    A, B = _exact_f32(M, N, K)
    C0 = _halves(M, N, 5)[..., 0].contiguous() if acc else None
    ref = _oracle(A, B, alpha=alpha, C0=C0)
    assert torch.equal(ref.float().double(), ref)
    out = C0.clone().to(dev) if acc else None
    y = ops.gemm_nt_f32(A.to(dev), B.to(dev), alpha=alpha, out=out, accumulate=acc)
    assert y.dtype == F32 and y.device.type == dev
    _check_exact("gemm_f32", y, ref)


@pytest.mark.parametrize("acc", [False, True], ids=["store", "acc"])
@pytest.mark.parametrize("M,N,K", [(17, 33, 20), (129, 130, 36), (17, 33, 18), (130, 129, 37)])
@pytest.mark.parametrize("dev", DEVS)
def test_gemm_f32_views(dev, M, N, K, acc):
    """NaN-surrounded operand views and a sentinel-surrounded out view. K = 20 and 36 leave a tail of 4 after whole
    16-wide k steps and the kernel reads the views in place (16-B rows); K = 18 and 37 are no multiple of 4, the
    kernel's contract, so ``ops`` hands it zero-padded copies and must take nothing but the view into them."""
    A, B = _exact_f32(M, N, K)
    bigA, va = _nan_parent(A, aligned=K % 4 == 0)
    bigB, vb = _nan_parent(B, r0=1, aligned=K % 4 == 0)
    C0 = _halves(M, N, 7)[..., 0].contiguous() if acc else None
    ref = _oracle(A, B, alpha=-2.0, C0=C0)
    ity, pattern = SENTINEL["f32"]
    wide = torch.full((M + 4, N + 7), pattern, dtype=ity).view(F32).to(dev)
    out = wide[2:2 + M, 3:3 + N]
    if acc:
        out.copy_(C0)
    y = ops.gemm_nt_f32(va(bigA.to(dev)), vb(bigB.to(dev)), alpha=-2.0, out=out, accumulate=acc)
    assert y.data_ptr() == out.data_ptr()
    _check_exact("gemm_f32", out, ref)
    bits = wide.cpu().view(ity).clone()
    bits[2:2 + M, 3:3 + N] = pattern
    assert (bits == pattern).all(), f"overwritten outside the view, first at {(bits != pattern).nonzero()[0].tolist()}"
