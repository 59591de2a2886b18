"""conv2d and im2col (csrc/kernels/conv2d.hip) against a float64 oracle written from the definition.

Oracle. ``_oracle`` builds a zero-padded float64 copy of X and, for every filter tap (kh, kw), adds
``einsum('nchw,oc->nohw', Xpad[..., kh*dil : ... : stride, kw*dil : ... : stride], W[:, :, kh, kw])``; then the
bias. It never calls ``ops``, ``F.conv2d`` or ``unfold``. The NHWC matrix is ``permute(0, 2, 3, 1).reshape(-1, OC)``
of it. Each case runs twice against the same oracle: on the ``ops`` CPU fallback (unmarked) and on the HIP kernels
(``gpu`` mark). Every GPU case first asserts ``ops.conv2d_plan``, the dispatcher's own answer to "which kernel does
this call get", so a case can never test another kernel than its name says. Plans: ``igemm`` (generic gather
kernel), ``rows`` / ``rows_staged`` (two-pass row kernel with direct / LDS-staged stores), ``rowfull``, ``ws``.

Exact cases (no tolerance anywhere). X holds integers in [-4, 4], W integers in [-3, 3] times 0.25, the bias
half-integers in [-4, 4]: all exact in bf16. Every product is a multiple of 0.25 of magnitude <= 3, so every partial
sum, in any order, is a multiple of 0.25 below 3 K + 4 <= 2**11 (K <= 576 here): it has at most 13 significant bits
and f32 accumulation is exact. Hence an f32 output must EQUAL the oracle and a bf16 output must equal
``oracle.to(bfloat16)``, the round-to-nearest-even of an exact value (truncation differs whenever the dropped bits
are above half). The comparison is by value, so -0 and +0 are the same number; everything else is bit-equal.

Activations sigmoid / exp / tanh. W is scaled by a further 2**-2, the pre-activation s stays exact and |s| <=
3/16 * 4 * K + 4 <= 26.5 for the shapes used (K <= 30). The output is compared with the float64 activation of s
under the bounds tests/test_rowops.py derives for these same device functions (``__expf`` = ``v_exp_f32(x * log2e)``:
argument rounding |x| * 6e-8 plus 1 ulp, a division, a few ulp in all): f32 ``rtol 1e-5, atol 1e-30``; bf16
``(2**-8 + 2**-16) * |ref|`` (half a bf16 ulp for round to nearest even plus the f32 error).

Rounded data. X = randn and W = 0.1 * randn, both rounded to bf16 (the oracle reads the rounded values), f32 bias.
Products of two bf16 values are exact in f32, so only the additions round. With S the oracle evaluated on |X|, |W|,
|bias| (an upper bound of every partial sum's magnitude), each of the K accumulated terms and the bias may cost one
full f32 ulp of the running magnitude, 2**-23 * S, whether the matrix core rounds or truncates and in any order:
``|y - ref| <= (K + 4) * 2**-23 * S`` for f32 output (the 4 covers the bias add and the activation-free epilogue).
bf16 output adds the half ulp of the rounding: ``+ 2**-8 * |ref|``. Derived, not measured; the worst err / bound
seen is printed in the ``CONV_WORST`` line.

Non-finite pixels. One NaN and one +Inf pixel inside X. The oracle's non-finite outputs are exactly the pixel's
receptive set (all OC planes of its image, rows ``[h-KH+1, h]``, columns ``[c-KW+1, c]``; the test asserts this of
the oracle first). ``igemm`` gathers exactly the taps of the definition: its non-finite set must equal the
oracle's. The row kernels read 8 taps per filter row with zero weights past KW, and 0 * NaN = NaN: their non-finite
set must contain the oracle's and lie inside columns ``[c-7, c]`` of the same rows and planes; everything outside
that window is exact for every plan.

im2col. X is random 16-bit patterns viewed as bf16 (NaN, -0, Inf included); the result is compared as int16, bit
for bit, with ``out[p][k] = Xpad[n, c, oh*stride + kh*dil, ow*stride + kw*dil]`` (k = (c, kh, kw)), zero for k >= K.
"""
import functools
import json

import pytest
import torch

from netsdb_amd import ops

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DT = {"f32": F32, "bf16": BF16}
ACTS = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "sigmoid": ops.ACT_SIGMOID, "exp": ops.ACT_EXP,
        "tanh": ops.ACT_TANH}
BF16_RTOL = 2.0 ** -8 + 2.0 ** -16
EXP_TOL = (1e-5, 1e-30)
GPU_MARK = pytest.mark.gpu
DEVS = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=GPU_MARK)]

_WORST = {}                 # "<plan>/<out dtype>/<device>" -> worst err / bound seen in this run (exact cases: 0)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nCONV_WORST " + json.dumps({k: float(f"{v:.3g}") for k, v in sorted(_WORST.items())}))


def _note(plan, y, ratio):
    key = f"{plan}/{'f32' if y.dtype == F32 else 'bf16'}/{'gpu' if y.is_cuda else 'cpu'}"
    _WORST[key] = max(_WORST.get(key, 0.0), float(ratio))


# ---------------------------------------------------------------------------------------------------------- oracle

def _out_hw(H, W, KH, KW, s, p, d):
    return (H + 2 * p - d * (KH - 1) - 1) // s + 1, (W + 2 * p - d * (KW - 1) - 1) // s + 1


def _oracle(X, W4, bias, s, p, d):
    """float64 NCHW convolution from the definition: one einsum per filter tap over a zero-padded copy of X."""
    N, C, H, W = X.shape
    OC, _, KH, KW = W4.shape
    OH, OW = _out_hw(H, W, KH, KW, s, p, d)
    Xp = torch.zeros(N, C, H + 2 * p, W + 2 * p, dtype=F64)
    Xp[:, :, p:p + H, p:p + W] = X.double()
    Wd = W4.double()
    y = torch.zeros(N, OC, OH, OW, dtype=F64)
    for kh in range(KH):
        for kw in range(KW):
            win = Xp[:, :, kh * d: kh * d + (OH - 1) * s + 1: s, kw * d: kw * d + (OW - 1) * s + 1: s]
            y += torch.einsum("nchw,oc->nohw", win, Wd[:, :, kh, kw])
    if bias is not None:
        y += bias.double()[None, :, None, None]
    return y


def _act64(v, act):
    if act == "relu":
        return v.clamp(min=0)
    if act == "sigmoid":
        return 1 / (1 + torch.exp(-v))
    if act == "exp":
        return torch.exp(v)
    if act == "tanh":
        return torch.tanh(v)
    return v


def _layout(ref, nchw):
    return ref if nchw else ref.permute(0, 2, 3, 1).reshape(-1, ref.shape[1])


def _geom(*shape, s=1, p=0, d=1):
    """(N, C, H, W, OC, KH, KW), stride, pad, dil"""
    assert len(shape) == 7
    return (tuple(shape), s, p, d)


def _flat(W4, extra=0):
    """[OC, ldw] bf16 in (c, kh, kw) order, ldw = K rounded up to 8 (+ extra); the padding columns hold zero."""
    OC = W4.shape[0]
    K = W4[0].numel()
    ldw = (K + 7) // 8 * 8 + extra
    Wf = torch.zeros(OC, ldw, dtype=BF16)
    Wf[:, :K] = W4.reshape(OC, K).to(BF16)
    assert torch.equal(Wf[:, :K].double(), W4.reshape(OC, K).double())      # the filter values are exact in bf16
    return Wf


@functools.lru_cache(maxsize=None)
def _exact(geom, wshift=0):
    """Integer-valued case (see the module docstring): X bf16, W4 f64, bias f32, the bias-free pre-activation."""
    (N, C, H, W, OC, KH, KW), s, p, d = geom
    g = torch.Generator().manual_seed(hash((geom, wshift)) & 0xFFFFFF)
    X = torch.randint(-4, 5, (N, C, H, W), generator=g).to(BF16)
    W4 = torch.randint(-3, 4, (OC, C, KH, KW), generator=g).double() * (0.25 * 2.0 ** -wshift)
    bias = torch.randint(-8, 9, (OC,), generator=g).float() * 0.5
    return X, W4, bias, _oracle(X, W4, None, s, p, d)


def _pre(geom, has_bias, wshift=0):
    X, W4, bias, s0 = _exact(geom, wshift)
    return s0 + bias.double()[None, :, None, None] if has_bias else s0


def _conv(dev, geom, X, Wf, bias, act, yout, nchw, opts, plan):
    """ops.conv2d on ``dev`` under ``opts``; on the GPU the dispatcher must first confirm ``plan``."""
    (N, C, H, W, OC, KH, KW), s, p, d = geom
    with ops.kernel_options(**opts):
        if dev == "cuda":
            got = ops.conv2d_plan(N, C, H, W, OC, KH, KW, s, p, d, ldw=Wf.shape[1], nchw_out=nchw, out_dtype=DT[yout])
            assert got == plan, f"this case is meant for the {plan} kernel, the dispatcher picks {got}"
        y = ops.conv2d(X.to(dev), Wf.to(dev), None if bias is None else bias.to(dev), KH, KW, s, p, d, ACTS[act],
                       nchw_out=nchw, out_dtype=DT[yout])
    OH, OW = _out_hw(H, W, KH, KW, s, p, d)
    assert y.dtype == DT[yout] and y.device.type == dev
    assert tuple(y.shape) == ((N, OC, OH, OW) if nchw else (N * OH * OW, OC))
    return y


def _check_exact(plan, y, ref):
    """y == ref (f32 output) or y == ref.to(bf16) (bf16 output) at every element: no tolerance."""
    want = ref.to(y.dtype).double()
    got = y.detach().cpu().double()
    bad = got != want
    _note(plan if y.is_cuda else "cpu", y, float("inf") if bad.any() else 0.0)
    if bad.any():
        at = tuple(bad.nonzero()[0].tolist())
        worst = (got - want).abs().nan_to_num(nan=float("inf"))
        w = tuple((worst == worst.max()).nonzero()[0].tolist())
        raise AssertionError(
            f"{plan}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result; first at {at}: got "
            f"{float(got[at])!r}, oracle {float(ref[at])!r} (-> {float(want[at])!r}); worst at {w}: got "
            f"{float(got[w])!r}, expected {float(want[w])!r}")


def _check_bound(plan, y, ref, bound):
    """|y - ref| <= bound elementwise (finite oracle); reports the worst element."""
    got = y.detach().cpu().double()
    assert ref.isfinite().all()
    assert got.isfinite().all(), f"{plan}: non-finite output at {got.isfinite().logical_not().nonzero()[0].tolist()}"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    w = tuple((ratio == ratio.max()).nonzero()[0].tolist())
    _note(plan if y.is_cuda else "cpu", y, float(ratio[w]))
    assert float(ratio[w]) <= 1.0, (
        f"{plan}: worst element {w}: got {float(got[w])!r}, oracle {float(ref[w])!r}, err {float(err[w]):.3e} > "
        f"bound {float(bound[w]):.3e}")


# ------------------------------------------------------------------------------------------------- the exact cases

# (act, out dtype, NCHW output, bias given)
A_ = ("none", "f32", True, True)
B_ = ("relu", "f32", False, False)
C_ = ("relu", "bf16", False, True)
D_ = ("none", "bf16", False, False)
E_ = ("relu", "bf16", True, True)
F_ = ("none", "bf16", True, False)
G_ = ("relu", "bf16", True, False)
H_ = ("none", "bf16", True, True)
NOT_STAGED = (A_, B_, C_, D_)          # f32 NCHW, f32 NHWC, bf16 NHWC: every axis value at least once
BF16_NCHW = (E_, F_, G_, H_)
ANY_KERNEL = (A_, B_, C_, F_)          # the four dtype / layout pairs, both acts, bias and none

# bf16 NCHW -> rows_staged; any other output -> rows
STAGED_SHAPES = [
    _geom(2, 3, 12, 32, 70, 3, 3),     # OH 10, OW 30: last row group of 2 rows, second oc tile partial
    _geom(2, 2, 9, 64, 40, 5, 5),      # OH 5: last group of 1 row
    _geom(2, 3, 7, 24, 33, 1, 1),      # 1x1 filter
    _geom(1, 3, 9, 96, 64, 6, 1),      # OW 96: six pixel tiles
    _geom(1, 1, 4, 8, 1, 1, 1),        # the minimum
    _geom(2, 1, 10, 16, 17, 7, 7),     # OW 10
]
# bf16 NCHW where staging is refused -> rows
DIRECT_SHAPES = [
    _geom(2, 3, 11, 32, 8, 3, 3),      # OH*OW = 270
    _geom(1, 1, 11, 16, 5, 8, 8),      # OW 9 (odd), KW 8
    _geom(1, 3, 13, 112, 64, 7, 7),    # OH 7, OW 106: (OH % 4) * OW % 4 != 0
    _geom(1, 6, 10, 96, 16, 2, 3),     # C * rin = 30: the LDS row limit
]
# 7 pixel tiles, bf16 NCHW: ws (default), rowfull (conv_kernel=1), rows_staged (conv_kernel=0)
WIDE_SHAPES = [
    _geom(3, 3, 16, 104, 70, 7, 7),    # OW 98, OH 10: 3 row groups per image (last of 2 rows), 9 in all; OC 64 + 6
    _geom(2, 3, 12, 112, 64, 7, 1),    # OW 112
    _geom(2, 2, 14, 104, 16, 5, 3),    # OW 102
]
# row-path preconditions that fail -> igemm
NOT_ROW_SHAPES = [
    _geom(2, 3, 20, 18, 8, 7, 7),      # W % 8 != 0
    _geom(2, 3, 12, 120, 16, 7, 7),    # OW 114 > 112
    _geom(1, 4, 10, 96, 16, 7, 1),     # C * KH = 28 > 24
]
# geometry that is always igemm
GEOMETRY_SHAPES = [
    _geom(2, 5, 13, 17, 70, 3, 2, s=2, p=2, d=2),
    _geom(1, 64, 14, 14, 70, 3, 3, s=2, p=1),          # K = 576: three LDS K chunks
    _geom(3, 2, 19, 23, 15, 3, 3, s=3, p=3, d=3),
    _geom(1, 2, 6, 7, 5, 2, 2, p=3),                   # pad beyond the kernel's reach: border outputs = bias alone
    _geom(1, 2, 5, 6, 5, 2, 2, p=5, d=2),              # the same with dilation
    _geom(1, 256, 5, 6, 9, 1, 1),                      # K = 256: exactly one K chunk
    _geom(1, 257, 5, 6, 9, 1, 1),                      # K = 257: one element into the second chunk
    _geom(1, 8, 5, 6, 9, 1, 1),                        # K = 8
] + [_geom(1, 3, 6, 7, oc, 3, 3, p=1) for oc in (1, 15, 64, 65, 130)] + [
    _geom(1, 2, 1, 3, 5, 3, 3, p=1),                   # P = N*OH*OW = 3
    _geom(1, 2, 1, 127, 5, 3, 3, p=1),                 # P = 127
    _geom(2, 2, 8, 8, 5, 3, 3, p=1),                   # P = 128
    _geom(3, 2, 1, 43, 5, 3, 3, p=1),                  # P = 129
    _geom(3, 2, 3, 3, 7, 3, 3, p=1),                   # N = 3, OH*OW % 4 = 1: 4-pixel stores straddle images
    _geom(3, 2, 3, 2, 7, 3, 3, p=1),                   # OH*OW % 4 = 2
    _geom(3, 2, 1, 7, 7, 3, 3, p=1),                   # OH*OW % 4 = 3 (bf16: odd plane offsets)
]
STRADDLE = GEOMETRY_SHAPES[-3:]

_CASES = []        # (id, dev param, geom, combo, opts, plan, ldw extra)
_CPU_SEEN = set()


def _sid(geom):
    shape, s, p, d = geom
    return "x".join(map(str, shape)) + (f"_s{s}p{p}d{d}" if (s, p, d) != (1, 0, 1) else "")


def _oid(opts):
    short = {"conv_kernel": "k", "conv_blocks": "b", "conv_contig": "c", "conv_generic": "g"}
    return "".join(f"_{short[k]}{int(v)}" for k, v in opts.items())


def _add(plan, geom, combos, opts=None, extra=0):
    """One GPU case per combo under ``opts``; the CPU fallback (which has no options) once per (geom, combo, extra)."""
    opts = opts or {}
    for combo in combos:
        act, yout, nchw, has_bias = combo
        cid = (f"{_sid(geom)}{_oid(opts)}{'_ldw+8' if extra else ''}-{act}-{yout}-{'nchw' if nchw else 'nhwc'}-"
               f"{'bias' if has_bias else 'nobias'}")
        _CASES.append(pytest.param("cuda", geom, combo, opts, plan, extra, id=f"{plan}-{cid}-gpu", marks=GPU_MARK))
        if (geom, combo, extra) not in _CPU_SEEN:
            _CPU_SEEN.add((geom, combo, extra))
            _CASES.append(pytest.param("cpu", geom, combo, {}, "cpu", extra, id=f"cpu-{cid}"))


def _build_cases():
    for g in STAGED_SHAPES:
        _add("rows_staged", g, BF16_NCHW)
        _add("rows", g, NOT_STAGED)
    for g in DIRECT_SHAPES:
        _add("rows", g, BF16_NCHW)
    for g in WIDE_SHAPES:
        for kernel, plan in ((5, "ws"), (1, "rowfull")):
            # 9 row groups: 2 blocks walk 5 and 4 of them (both parities of the last-group flush), 1 block all 9,
            # 0 = one block per group, 512 = the default cap
            _add(plan, g, BF16_NCHW, {"conv_kernel": kernel, "conv_blocks": 512})
            for blocks, combos in ((0, (E_, F_)), (2, (G_, H_)), (1, (E_, F_))):
                _add(plan, g, combos, {"conv_kernel": kernel, "conv_blocks": blocks})
        # contiguous runs of row groups; with 4 blocks over 9 groups per = 3 and the fourth block owns none
        _add("rowfull", g, (E_,), {"conv_kernel": 1, "conv_contig": 1, "conv_blocks": 2})
        _add("rowfull", g, (F_,), {"conv_kernel": 1, "conv_contig": 1, "conv_blocks": 4})
        _add("rows_staged", g, BF16_NCHW, {"conv_kernel": 0})        # the two-pass kernel with 7 tiles
        _add("rows", g, NOT_STAGED)
    for g in STAGED_SHAPES + DIRECT_SHAPES + WIDE_SHAPES:            # fallthrough from the row path
        _add("igemm", g, ANY_KERNEL, {"conv_generic": True})
    for g in NOT_ROW_SHAPES + GEOMETRY_SHAPES:
        _add("igemm", g, ANY_KERNEL)
    for g in STRADDLE:
        _add("igemm", g, (E_, H_))
    # filter rows 8 columns longer than K rounded up (zero padding): one shape per plan
    _add("rows_staged", STAGED_SHAPES[0], (E_, F_), extra=8)
    _add("rows", STAGED_SHAPES[0], (A_, C_), extra=8)
    _add("ws", WIDE_SHAPES[0], (E_, F_), extra=8)
    _add("rowfull", WIDE_SHAPES[0], (E_, F_), {"conv_kernel": 1}, extra=8)
    _add("igemm", GEOMETRY_SHAPES[0], (A_, F_), extra=8)
    _add("igemm", GEOMETRY_SHAPES[6], (A_, F_), extra=8)


_build_cases()


@pytest.mark.parametrize("dev,geom,combo,opts,plan,extra", _CASES)
def test_conv2d_exact(dev, geom, combo, opts, plan, extra):
    act, yout, nchw, has_bias = combo
    X, W4, bias, _ = _exact(geom)
    ref = _layout(_act64(_pre(geom, has_bias), act), nchw)
    y = _conv(dev, geom, X, _flat(W4, extra), bias if has_bias else None, act, yout, nchw, opts, plan)
    _check_exact(plan, y, ref)


@pytest.mark.parametrize("geom", GEOMETRY_SHAPES[3:5], ids=_sid)
def test_pad_beyond_reach_case_has_bias_only_borders(geom):
    """The oracle of the two large-pad cases: the outermost ring of outputs sees padding only (= the bias)."""
    X, W4, bias, s0 = _exact(geom)
    assert (s0[:, :, 0] == 0).all() and (s0[:, :, -1] == 0).all() and (s0[..., 0] == 0).all() \
        and (s0[..., -1] == 0).all()
    assert (s0 != 0).any()


def test_case_table_reaches_every_plan_with_every_axis_value():
    """Each of the five plans sees both acts, bias and none, and every dtype / layout pair it supports."""
    seen = {}
    for c in _CASES:
        dev, geom, combo, opts, plan, extra = c.values
        if dev == "cuda":
            seen.setdefault(plan, set()).add(combo)
            (N, C, H, W, OC, KH, KW), s, p, d = geom
            with ops.kernel_options(**opts):       # the dispatcher is host arithmetic: no GPU needed to ask it
                got = ops.conv2d_plan(N, C, H, W, OC, KH, KW, s, p, d, ldw=(C * KH * KW + 7) // 8 * 8 + extra,
                                      nchw_out=combo[2], out_dtype=DT[combo[1]])
            assert got == plan, (c.id, got)
    assert set(seen) == {"igemm", "rows", "rows_staged", "rowfull", "ws"}
    for plan, combos in seen.items():
        pairs = {(c[1], c[2]) for c in combos}
        want = {("bf16", True)} if plan in ("rows_staged", "rowfull", "ws") else \
            {("f32", True), ("f32", False), ("bf16", True), ("bf16", False)}
        assert pairs == want, (plan, pairs)
        assert {c[0] for c in combos} == {"none", "relu"} and {c[3] for c in combos} == {True, False}, plan


# ---------------------------------------------------------------------------------- filter cache behind ops.derived

CACHE_CASES = [("ws", WIDE_SHAPES[0], {}), ("rowfull", WIDE_SHAPES[0], {"conv_kernel": 1}),
               ("rows_staged", STAGED_SHAPES[0], {}), ("rows", DIRECT_SHAPES[0], {})]


@pytest.mark.parametrize("plan,geom,opts", CACHE_CASES, ids=[c[0] for c in CACHE_CASES])
@pytest.mark.parametrize("dev", DEVS)
def test_filter_modified_in_place_between_calls(dev, plan, geom, opts):
    """Wflat.mul_(2) after a first call: the second call must use the new weights (the packed filter fragments
    are cached per filter tensor AND its in-place version)."""
    X, W4, bias, s0 = _exact(geom)
    (N, C, H, W, OC, KH, KW), s, p, d = geom
    b64 = bias.double()[None, :, None, None]
    Wf = _flat(W4).to(dev)
    Xd, bd = X.to(dev), bias.to(dev)
    with ops.kernel_options(**opts):
        if dev == "cuda":
            assert ops.conv2d_plan(N, C, H, W, OC, KH, KW, nchw_out=True) == plan
        y1 = ops.conv2d(Xd, Wf, bd, KH, KW, nchw_out=True)
        Wf.mul_(2)
        y2 = ops.conv2d(Xd, Wf, bd, KH, KW, nchw_out=True)
    _check_exact(plan, y1, s0 + b64)
    _check_exact(plan, y2, 2 * s0 + b64)


# ----------------------------------------------------------------------------------------------------- activations

ACT_CASES = [
    ("igemm", GEOMETRY_SHAPES[0], {}, [("f32", True), ("f32", False), ("bf16", True), ("bf16", False)]),
    ("rows", DIRECT_SHAPES[0], {}, [("f32", True), ("f32", False), ("bf16", True), ("bf16", False)]),
    ("rows_staged", STAGED_SHAPES[0], {}, [("bf16", True)]),
    ("rowfull", WIDE_SHAPES[1], {"conv_kernel": 1}, [("bf16", True)]),
    ("ws", WIDE_SHAPES[1], {}, [("bf16", True)]),
]
_ACT_PARAMS = [pytest.param(plan, geom, opts, yout, nchw, id=f"{plan}-{yout}-{'nchw' if nchw else 'nhwc'}")
               for plan, geom, opts, outs in ACT_CASES for yout, nchw in outs]


@pytest.mark.parametrize("act", ["sigmoid", "exp", "tanh"])
@pytest.mark.parametrize("plan,geom,opts,yout,nchw", _ACT_PARAMS)
@pytest.mark.parametrize("dev", DEVS)
def test_conv2d_activation(dev, plan, geom, opts, yout, nchw, act):
    X, W4, bias, _ = _exact(geom, 2)
    s = _pre(geom, True, 2)
    assert float(s.abs().max()) <= 27
    ref = _layout(_act64(s, act), nchw)
    y = _conv(dev, geom, X, _flat(W4), bias, act, yout, nchw, opts, plan)
    rtol, atol = (BF16_RTOL, EXP_TOL[1]) if yout == "bf16" else EXP_TOL
    _check_bound(plan, y, ref, rtol * ref.abs() + atol)


# ---------------------------------------------------------------------------------------------------- rounded data

ROUNDED_CASES = [
    ("igemm", GEOMETRY_SHAPES[1], {}, "f32", False), ("igemm", GEOMETRY_SHAPES[0], {}, "bf16", True),
    ("igemm", WIDE_SHAPES[0], {"conv_generic": True}, "f32", True),
    ("rows", DIRECT_SHAPES[2], {}, "f32", True), ("rows", DIRECT_SHAPES[2], {}, "bf16", True),
    ("rows_staged", STAGED_SHAPES[1], {}, "bf16", True),
    ("rowfull", WIDE_SHAPES[0], {"conv_kernel": 1}, "bf16", True),
    ("ws", WIDE_SHAPES[0], {}, "bf16", True),
]


@functools.lru_cache(maxsize=None)
def _rounded(geom):
    (N, C, H, W, OC, KH, KW), s, p, d = geom
    g = torch.Generator().manual_seed(7 + (hash(geom) & 0xFFFF))
    X = torch.randn(N, C, H, W, generator=g).to(BF16)
    W4 = (0.1 * torch.randn(OC, C, KH, KW, generator=g)).to(BF16)
    bias = torch.randn(OC, generator=g)
    ref = _oracle(X, W4, bias, s, p, d)
    S = _oracle(X.abs(), W4.abs(), bias.abs(), s, p, d)
    return X, W4, bias, ref, S


@pytest.mark.parametrize("plan,geom,opts,yout,nchw", ROUNDED_CASES,
                         ids=[f"{c[0]}-{_sid(c[1])}-{c[3]}" for c in ROUNDED_CASES])
@pytest.mark.parametrize("dev", DEVS)
def test_conv2d_rounded_data(dev, plan, geom, opts, yout, nchw):
    X, W4, bias, ref, S = _rounded(geom)
    K = W4[0].numel()
    bound = (K + 4) * 2.0 ** -23 * S
    if yout == "bf16":
        bound = bound + 2.0 ** -8 * ref.abs()
    y = _conv(dev, geom, X, _flat(W4), bias, "none", yout, nchw, opts, plan)
    _check_bound(plan, y, _layout(ref, nchw), _layout(bound, nchw))


# ----------------------------------------------------------------------------------------------- non-finite pixels

# plan, geom, opts, out dtype, the NaN pixel (n, c, h, w), the +Inf pixel
NONFINITE_CASES = [
    ("igemm", _geom(2, 3, 13, 24, 20, 3, 3, p=1), {}, "f32", (0, 1, 5, 12), (1, 2, 9, 20)),
    ("igemm", WIDE_SHAPES[0], {"conv_generic": True}, "bf16", (0, 1, 7, 50), (2, 0, 12, 90)),
    ("rows", _geom(2, 3, 13, 24, 20, 3, 3), {}, "f32", (0, 1, 5, 12), (1, 2, 9, 20)),
    ("rows_staged", _geom(2, 3, 14, 32, 20, 3, 3), {}, "bf16", (0, 1, 5, 12), (1, 2, 9, 20)),
    ("rowfull", WIDE_SHAPES[0], {"conv_kernel": 1}, "bf16", (0, 1, 7, 50), (2, 0, 12, 90)),
    ("ws", WIDE_SHAPES[0], {}, "bf16", (0, 1, 7, 50), (2, 0, 12, 90)),
]


@pytest.mark.parametrize("plan,geom,opts,yout,nan_at,inf_at", NONFINITE_CASES,
                         ids=[f"{c[0]}-{_sid(c[1])}" for c in NONFINITE_CASES])
@pytest.mark.parametrize("dev", DEVS)
def test_conv2d_nonfinite_pixels(dev, plan, geom, opts, yout, nan_at, inf_at):
    (N, C, H, W, OC, KH, KW), s, p, d = geom
    assert s == 1 and d == 1
    X0, W4, bias, _ = _exact(geom)
    X = X0.clone()
    X[nan_at] = float("nan")
    X[inf_at] = float("inf")
    ref = _oracle(X, W4, bias, s, p, d)
    OH, OW = ref.shape[2:]
    field = torch.zeros_like(ref, dtype=torch.bool)      # the receptive sets of the two pixels
    window = torch.zeros_like(ref, dtype=torch.bool)     # the row kernels' 8-tap window around them
    for n, _, h, w in (nan_at, inf_at):
        rows = slice(max(h + p - KH + 1, 0), min(h + p, OH - 1) + 1)
        field[n, :, rows, max(w + p - KW + 1, 0): min(w + p, OW - 1) + 1] = True
        window[n, :, rows, max(w + p - 7, 0): min(w + p, OW - 1) + 1] = True
    assert torch.equal(~ref.isfinite(), field), "the oracle's non-finite set is not the receptive set"
    y = _conv(dev, geom, X, _flat(W4), bias, "none", yout, True, opts, plan)
    got = y.detach().cpu().double()
    bad = ~got.isfinite()
    assert not (field & ~bad).any(), (
        f"{plan}: finite output where the oracle is not, first at {(field & ~bad).nonzero()[0].tolist()}")
    assert not (bad & ~window).any(), (
        f"{plan}: non-finite output outside the 8-tap window, first at {(bad & ~window).nonzero()[0].tolist()}")
    outside = ~window
    want = ref.to(y.dtype).double()
    assert torch.equal(got[outside], want[outside]), f"{plan}: finite outputs outside the window are not exact"
    if plan == "igemm" or dev == "cpu":
        assert torch.equal(bad, field), (
            f"{plan}: non-finite set differs from the oracle's, first at {(bad != field).nonzero()[0].tolist()}")
    else:
        print(f"\nCONV_NONFINITE {plan}: {int(bad.sum())} non-finite outputs, oracle {int(field.sum())}, "
              f"8-tap window {int(window.sum())}")


@pytest.mark.parametrize("plan,geom,opts,yout,nan_at,inf_at", NONFINITE_CASES,
                         ids=[f"{c[0]}-{_sid(c[1])}" for c in NONFINITE_CASES])
@pytest.mark.parametrize("dev", DEVS)
def test_conv2d_relu_of_nan(dev, plan, geom, opts, yout, nan_at, inf_at):
    """relu keeps NaN, as torch.relu and the CPU path do (``v > 0 ? v : 0`` gave 0): with one NaN pixel and relu,
    every output of the pixel's receptive set is NaN, and everything outside the row kernels' 8-tap window is the
    exact relu of the finite oracle (igemm and the CPU path: everything outside the receptive set)."""
    (N, C, H, W, OC, KH, KW), s, p, d = geom
    X0, W4, bias, _ = _exact(geom)
    X = X0.clone()
    X[nan_at] = float("nan")
    ref = _oracle(X, W4, bias, s, p, d)
    ref = torch.where(ref < 0, torch.zeros_like(ref), ref)               # relu that keeps NaN
    OH, OW = ref.shape[2:]
    n, _, h, w = nan_at
    rows = slice(max(h + p - KH + 1, 0), min(h + p, OH - 1) + 1)
    field = torch.zeros_like(ref, dtype=torch.bool)
    window = torch.zeros_like(ref, dtype=torch.bool)
    field[n, :, rows, max(w + p - KW + 1, 0): min(w + p, OW - 1) + 1] = True
    window[n, :, rows, max(w + p - 7, 0): min(w + p, OW - 1) + 1] = True
    assert torch.equal(ref.isnan(), field) and (ref[~field] == 0).any() and (ref[~field] > 0).any()
    y = _conv(dev, geom, X, _flat(W4), bias, "relu", yout, True, opts, plan)
    got = y.detach().cpu().double()
    assert got[field].isnan().all(), (
        f"{plan}: relu turned NaN into a number, first at {(field & ~got.isnan()).nonzero()[0].tolist()}")
    exact = ~field if plan == "igemm" or dev == "cpu" else ~window
    assert torch.equal(got[exact], ref.to(y.dtype).double()[exact]), f"{plan}: outputs away from the NaN are not exact"


# ------------------------------------------------------------------------------------------- the offset sentinel

@pytest.mark.parametrize("dev", DEVS)
def test_conv2d_refuses_images_reaching_the_masked_load_offset(dev):
    """A bf16 image set of 2 GiB + 512 KiB: the byte offset the kernels give a masked load (0x7ffffff0) would lie
    inside it and read a real pixel instead of zero. The call is refused before any launch."""
    X = torch.empty((1, 1, 32768, 32776), dtype=BF16, device=dev)
    assert X.numel() * 2 > 0x7FFFFFF0
    Wf = torch.zeros(4, 16, dtype=BF16, device=dev)
    for nchw in (True, False):
        with pytest.raises(RuntimeError):
            ops.conv2d(X, Wf, None, 3, 3, stride=1024, pad=1, nchw_out=nchw, out_dtype=F32)
    if dev == "cuda":
        with pytest.raises(RuntimeError):
            ops.conv2d_plan(1, 1, 32768, 32776, 4, 3, 3, 1024, 1, 1)
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------- im2col

def _im2col_oracle(X, KH, KW, s, p, d, ldk):
    """int16 gather from the definition: out[p][k] = Xpad[n, c, oh*s + kh*d, ow*s + kw*d], zero for k >= K."""
    N, C, H, W = X.shape
    OH, OW = _out_hw(H, W, KH, KW, s, p, d)
    K = C * KH * KW
    Xp = torch.zeros(N, C, H + 2 * p, W + 2 * p, dtype=torch.int16)
    Xp[:, :, p:p + H, p:p + W] = X
    pp = torch.arange(N * OH * OW)
    n, oh, ow = pp // (OH * OW), pp % (OH * OW) // OW, pp % OW
    k = torch.arange(K)
    c, kh, kw = k // (KH * KW), k % (KH * KW) // KW, k % KW
    out = torch.zeros(N * OH * OW, ldk, dtype=torch.int16)
    out[:, :K] = Xp[n[:, None], c[None, :], oh[:, None] * s + kh[None, :] * d, ow[:, None] * s + kw[None, :] * d]
    return out


def _im2col_case(dev, shape, KH, KW, s, p, d, ldk_mode):
    N, C, H, W = shape
    K = C * KH * KW
    ldk = {"default": None, "bias_col": (K + 1 + 7) // 8 * 8, "k+9": K + 9}[ldk_mode]
    g = torch.Generator().manual_seed(N * C * H * W + KH * 10 + KW)
    bits = torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16)
    flat = bits.view(-1)
    flat[:6] = torch.tensor([0x7FC0, -0x8000, 0x7F80, -0x80, 0x7F81, 1], dtype=torch.int16)   # NaN -0 Inf -Inf sNaN den
    ref = _im2col_oracle(bits, KH, KW, s, p, d, ldk or (K + 7) // 8 * 8)
    y = ops.im2col(bits.view(BF16).to(dev), KH, KW, s, p, d, ldk)
    assert y.dtype == BF16 and y.device.type == dev and tuple(y.shape) == tuple(ref.shape)
    got = y.cpu().view(torch.int16)
    bad = got != ref
    assert not bad.any(), (f"{int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}: "
                           f"got {int(got[bad][0]):#x}, expected {int(ref[bad][0]):#x}")


@pytest.mark.parametrize("ldk_mode", ["default", "bias_col", "k+9"])
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("p", [0, 1, 2])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("dev", DEVS)
def test_im2col_3x3(dev, s, p, d, ldk_mode):
    _im2col_case(dev, (2, 3, 12, 10), 3, 3, s, p, d, ldk_mode)


@pytest.mark.parametrize("ldk_mode", ["default", "bias_col", "k+9"])
@pytest.mark.parametrize("KH,KW,s,p,d", [(1, 1, 1, 0, 1), (1, 1, 2, 1, 1), (5, 2, 1, 0, 1), (5, 2, 2, 2, 2)])
@pytest.mark.parametrize("dev", DEVS)
def test_im2col_1x1_and_5x2(dev, KH, KW, s, p, d, ldk_mode):
    _im2col_case(dev, (2, 3, 12, 10), KH, KW, s, p, d, ldk_mode)


@pytest.mark.parametrize("dev", DEVS)
def test_im2col_past_the_grid_cap(dev):
    """4 x 64 x 64 pixels x 144 columns = 2 359 296 elements, more than the 8192 x 256 threads of the capped grid:
    the last 262 144 come from the second grid-stride pass."""
    _im2col_case(dev, (4, 16, 64, 64), 3, 3, 1, 1, 1, "default")
