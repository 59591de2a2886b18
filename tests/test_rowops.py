"""Row / elementwise kernels (csrc/kernels/rowops.hip) against a float64 oracle.

Every operation has a small plain-torch float64 function below, written from the operation's definition and
evaluated on the CPU; none of them calls ``ops``. (The one exception is dropout: the keep mask is the host
``ops.hash_uniform``, because that mask is the contract between host and kernel.) Each case runs twice against the
same oracle: on the ``ops`` CPU fallback (unmarked) and on the HIP kernel (``gpu`` mark).

The comparison is elementwise, ``|y - ref| <= rtol * |ref| + atol`` at every element, never normalised by a global
maximum. The bounds come from the code, not from measurements:

* f32 output of an exp-based kernel (softmax, sigmoid / exp / tanh activations): rtol 1e-5, atol 1e-30.
  ``__expf(x)`` is ``v_exp_f32(x * log2e)``: rounding the argument costs about ``|x| * 6e-8`` relative, the
  instruction 1 ulp. The inputs keep every exponent argument within about +-40 (<= 2.5e-6), the row-sum
  reduction adds a few ulp; 1e-5 is roughly 3x that.
* log-softmax, lstm_cell, lstm_ew: rtol 1e-5, atol 1e-6 for O(1) inputs (the atol covers the cancellation in
  ``f * c_prev + i * g``; the inputs keep every product below 4, whose half ulp is 2.4e-7).
* bias_act with act none / relu, embedding_bag in f32: rtol 2e-6, atol 1e-6. A bag has at most 64 terms; the tables
  and weights are positive, so the sequential f32 sum's error stays relative to the result (first-order worst case
  64 * 2**-24 = 3.8e-6 with every rounding in one direction; the rounding errors are independent, the expected
  error is near sqrt(64) * 2**-25 = 2.4e-7).
* row_normalize in f32: rtol 5e-6, atol 0. All terms are positive (rand + 0.1). A thread of the scalar kernel adds
  at most 65 elements in sequence (N = 16388 over 256 threads), the wave butterfly adds 6 levels, the cross-wave
  loop 7 more, then one correctly rounded division and one multiplication: first-order worst case
  (64 + 6 + 7 + 2) * 2**-24 = 4.7e-6.
* any bf16 output: ``|y - ref| <= (2**-8 + 2**-16) * |ref| + atol``. 2**-8 is half a bf16 ulp (round to nearest
  even), 2**-16 covers the f32 compute error; truncation (up to 2**-7) fails it. bf16 inputs are rounded to bf16
  first and the oracle reads the rounded values.
"""
import json

import numpy as np
import pytest
import torch

from netsdb_amd import ops

F32, BF16 = torch.float32, torch.bfloat16
DT = {"f32": F32, "bf16": BF16}
DEVS = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
GPU = [pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
BF16_RTOL = 2.0 ** -8 + 2.0 ** -16
EXP_TOL = (1e-5, 1e-30)
LOG_TOL = (1e-5, 1e-6)      # log-softmax, lstm_cell, lstm_ew
LIN_TOL = (2e-6, 1e-6)      # bias_act none / relu, embedding_bag
RN_TOL = (5e-6, 0.0)        # row_normalize

_WORST = {}                 # "<kernel>/<device>" -> worst err / bound seen in this run


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nROWOPS_WORST " + json.dumps({k: float(f"{v:.3g}") for k, v in sorted(_WORST.items())}))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dev(t, dev):
    return None if t is None else t.to(dev)


def _check(kernel, y, ref, tol):
    """|y - ref| <= rtol * |ref| + atol at every element (bf16 outputs: the half-ulp rtol); NaN and +-inf of the
    oracle must be met exactly. Reports the worst element."""
    rtol, atol = tol
    if y.dtype == BF16:
        rtol = BF16_RTOL
        kernel += "[bf16]"
    assert y.dtype in (F32, BF16) and ref.dtype == torch.float64
    assert tuple(y.shape) == tuple(ref.shape), f"{kernel}: shape {tuple(y.shape)} != {tuple(ref.shape)}"
    dev = y.device.type
    y = y.detach().cpu().double()
    nan = ref.isnan()
    assert torch.equal(y.isnan(), nan), (
        f"{kernel}: NaN pattern differs: {int(y.isnan().sum())} NaN in the output, {int(nan.sum())} in the oracle; "
        f"first at {(y.isnan() != nan).nonzero()[0].tolist()}")
    inf = ref.isinf()
    assert torch.equal(y[inf], ref[inf]), f"{kernel}: +-inf elements of the oracle are not met exactly"
    fin = ~(nan | inf)
    err = (y - ref).abs()[fin]
    if err.numel() == 0:
        return
    bound = (rtol * ref.abs() + atol)[fin]
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)   # err > 0 over a zero bound: inf
    w = int(ratio.argmax())
    key = f"{kernel}/{dev}"
    _WORST[key] = max(_WORST.get(key, 0.0), float(ratio[w]))
    at = fin.nonzero()[w].tolist()
    assert float(ratio[w]) <= 1.0, (
        f"{kernel}: worst element {at}: got {float(y[fin][w])!r}, oracle {float(ref[fin][w])!r}, "
        f"err {float(err[w]):.3e} > bound {float(bound[w]):.3e} (rtol {rtol:.3g}, atol {atol:.3g})")


# ---------------------------------------------------------------------------------------------------- softmax_rows

def _softmax_oracle(X, bias, log):
    v = X.double()
    if bias is not None:
        v = v + bias.double()
    return torch.log_softmax(v, dim=-1) if log else torch.softmax(v, dim=-1)


def _run_softmax(dev, X, bias, yout, log, name="softmax_rows"):
    ref = _softmax_oracle(X, bias, log)
    y = ops.softmax_rows(_dev(X, dev), _dev(bias, dev), out_dtype=DT[yout], log=log)
    assert y.dtype == DT[yout] and y.device.type == dev
    _check(name + ("_log" if log else ""), y, ref, LOG_TOL if log else EXP_TOL)
    return y.cpu(), ref


SM_SHAPES = [(1, 1), (3, 7), (2, 64), (5, 255), (5, 256), (4, 257), (3, 1000), (2, 5000)]


@pytest.mark.parametrize("log", [False, True], ids=["prob", "log"])
@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("yout", ["f32", "bf16"])
@pytest.mark.parametrize("xin", ["f32", "bf16"])
@pytest.mark.parametrize("R,N", SM_SHAPES)
@pytest.mark.parametrize("dev", DEVS)
def test_softmax_rows(dev, R, N, xin, yout, has_bias, log):
    """The four dtype pairs of softmax_rows_kernel, below / at / above one 256-thread pass, idle waves (N < 256)."""
    g = _gen(1000 * R + N)
    X = (torch.randn(R, N, generator=g) * 2).to(DT[xin])
    bias = torch.randn(N, generator=g) if has_bias else None
    y, _ = _run_softmax(dev, X, bias, yout, log)
    if not log and yout == "f32":
        s = y.double().sum(-1)
        assert ((s - 1).abs() <= N * 2.0 ** -23).all(), f"row sums {s.tolist()} not within N * 2**-23 of 1"


@pytest.mark.parametrize("log", [False, True], ids=["prob", "log"])
@pytest.mark.parametrize("xin", ["f32", "bf16"])
@pytest.mark.parametrize("dev", DEVS)
def test_softmax_rows_row_strided_input(dev, xin, log):
    """X = base[:, 3:3+N]: the row stride differs from N and the first element is not 16-B aligned."""
    R, N = 4, 300
    g = _gen(7)
    base = (torch.randn(R, N + 8, generator=g) * 2).to(DT[xin])
    bias = torch.randn(N, generator=g)
    ref = _softmax_oracle(base[:, 3:3 + N], bias, log)
    Xd = base.to(dev)[:, 3:3 + N]
    assert Xd.stride(0) == N + 8 and not Xd.is_contiguous()
    y = ops.softmax_rows(Xd, bias.to(dev), log=log)
    _check("softmax_rows_strided", y, ref, LOG_TOL if log else EXP_TOL)


@pytest.mark.parametrize("log", [False, True], ids=["prob", "log"])
@pytest.mark.parametrize("xin,yout", [("f32", "f32"), ("bf16", "f32"), ("f32", "bf16")])
@pytest.mark.parametrize("N", [7, 600])
@pytest.mark.parametrize("dev", DEVS)
def test_softmax_rows_wide_logit_spread(dev, N, xin, yout, log):
    """One column at +35 over logits in [-4.5, 4.5]: exponent arguments reach about -40, probabilities 1e-17, and
    the elementwise bound still holds for them (atol 1e-30 does not hide them)."""
    g = _gen(35 + N)
    X = torch.randn(3, N, generator=g).clamp(-4, 4)
    X[:, N // 2] = 35.0
    X = X.to(DT[xin])
    bias = torch.rand(N, generator=g) - 0.5
    _run_softmax(dev, X, bias, yout, log, "softmax_rows_spread")


def _mask_case(layout, g):
    R, N = 3, 600
    X = torch.randn(R, N, generator=g) * 2
    bias = torch.randn(N, generator=g)
    mask = torch.zeros(R, N, dtype=torch.bool)
    if layout in ("head", "bias"):
        mask[:, :300] = True        # every thread of the block reads -inf before its first finite element
    elif layout == "tail":
        mask[:, N - 100:] = True
    else:                           # scattered, different in every row; row 2 starts with one finite column
        mask[0, ::2] = True
        mask[1, 1::3] = True
        mask[2, 1:257] = True
    if layout == "bias":
        bias[:300] = float("-inf")
    else:
        X[mask] = float("-inf")
    return X, bias, mask


@pytest.mark.parametrize("log", [False, True], ids=["prob", "log"])
@pytest.mark.parametrize("xin,yout", [("f32", "f32"), ("bf16", "bf16")])
@pytest.mark.parametrize("layout", ["head", "tail", "bias", "scattered"])
@pytest.mark.parametrize("dev", DEVS)
def test_softmax_rows_masked_with_neg_inf(dev, layout, xin, yout, log):
    """-inf logits (ordinary masking): the float64 softmax of the same logits, exact zeros (log: -inf) at the masked
    positions, no NaN anywhere."""
    X, bias, mask = _mask_case(layout, _gen(600))
    X = X.to(DT[xin])
    y, ref = _run_softmax(dev, X, bias, yout, log, "softmax_rows_masked")
    assert not y.isnan().any()
    masked = y[mask].double()
    assert (masked == (float("-inf") if log else 0.0)).all()
    assert y[~mask].isfinite().all()
    assert ((ref[mask] == float("-inf")) if log else (ref[mask] == 0)).all()


@pytest.mark.parametrize("log", [False, True], ids=["prob", "log"])
@pytest.mark.parametrize("N,col", [(7, 2), (600, 0), (600, 300), (600, 599)])
@pytest.mark.parametrize("dev", DEVS)
def test_softmax_rows_nan_poisons_its_row_only(dev, N, col, log):
    g = _gen(N + col)
    X = torch.randn(3, N, generator=g)
    X[1, col] = float("nan")
    y, _ = _run_softmax(dev, X, None, "f32", log, "softmax_rows_nan")
    assert y[1].isnan().all() and not y[0].isnan().any() and not y[2].isnan().any()


# --------------------------------------------------------------------------------------------------- row_normalize

def _rownorm_oracle(X):
    v = X.double()
    return v / v.sum(-1, keepdim=True)


# N -> kernel on the GPU for an aligned f32 input: 4, 2048, 4096 vec NV=2; 4100, 8192 vec NV=4; 8196, 16384 vec NV=8;
# 16388 (too long for the registers), 130 and 7 (N % 4 != 0) the scalar two-pass kernel
RN_N = [4, 2048, 4096, 4100, 8192, 8196, 16384, 16388, 130, 7]
RN_DEV = [pytest.param("cpu", False, id="cpu"), pytest.param("cuda", False, id="gpu-nt", marks=pytest.mark.gpu),
          pytest.param("cuda", True, id="gpu-plain", marks=pytest.mark.gpu)]


def _run_rownorm(dev, plain, Xd, Xcpu, yout):
    ref = _rownorm_oracle(Xcpu)
    with ops.kernel_options(rownorm_plain_loads=plain):
        y = ops.row_normalize(Xd, out_dtype=DT[yout])
    assert y.dtype == DT[yout] and y.device.type == dev
    _check("row_normalize", y, ref, RN_TOL)


@pytest.mark.parametrize("yout", ["f32", "bf16"])
@pytest.mark.parametrize("N", RN_N)
@pytest.mark.parametrize("dev,plain", RN_DEV)
def test_row_normalize(dev, plain, N, yout):
    X = torch.rand(3, N, generator=_gen(N)) + 0.1
    _run_rownorm(dev, plain, X.to(dev), X, yout)


@pytest.mark.parametrize("yout", ["f32", "bf16"])
@pytest.mark.parametrize("N", [2048, 4100, 8196])
@pytest.mark.parametrize("dev,plain", RN_DEV)
def test_row_normalize_aligned_strided_view(dev, plain, N, yout):
    """base[:, 4:4+N] of a [3, N+8] f32 matrix: 16-B aligned rows with ldx != N, the vec kernel (NV = 2, 4, 8)."""
    base = torch.rand(3, N + 8, generator=_gen(N + 1)) + 0.1
    Xd = base.to(dev)[:, 4:4 + N]
    assert Xd.stride(0) == N + 8 and Xd.data_ptr() % 16 == 0
    _run_rownorm(dev, plain, Xd, base[:, 4:4 + N], yout)


@pytest.mark.parametrize("yout", ["f32", "bf16"])
@pytest.mark.parametrize("N,off,pad", [(2048, 1, 8), (4100, 1, 8), (2048, 4, 6)])
@pytest.mark.parametrize("dev,plain", RN_DEV)
def test_row_normalize_misaligned_view(dev, plain, N, off, pad, yout):
    """A first element off the 16-B grid (base[:, 1:1+N]) or a row stride that is no multiple of 4 floats: the
    16-B loads of the vec kernel do not apply, the scalar kernel must serve them."""
    base = torch.rand(3, N + pad, generator=_gen(N + off + pad)) + 0.1
    Xd = base.to(dev)[:, off:off + N]
    assert Xd.data_ptr() % 16 != 0 or Xd.stride(0) % 4 != 0
    _run_rownorm(dev, plain, Xd, base[:, off:off + N], yout)


@pytest.mark.parametrize("yout", ["f32", "bf16"])
@pytest.mark.parametrize("N", [7, 130, 4100])
@pytest.mark.parametrize("dev,plain", RN_DEV[:2])
def test_row_normalize_bf16_input(dev, plain, N, yout):
    X = (torch.rand(3, N, generator=_gen(N + 2)) + 0.1).to(BF16)
    _run_rownorm(dev, plain, X.to(dev), X, yout)


# -------------------------------------------------------------------------------------------------------- bias_act

ACTS = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "sigmoid": ops.ACT_SIGMOID, "exp": ops.ACT_EXP,
        "tanh": ops.ACT_TANH}
BIAS_MODES = {"nobias": ops.BIAS_NONE, "row": ops.BIAS_ROW, "col": ops.BIAS_COL}


def _bias_act_oracle(X, bias, mode, act):
    v = X.double()
    if bias is not None:
        v = v + (bias.double()[:, None] if mode == "row" else bias.double()[None, :])
    if act == "relu":
        v = v.clamp(min=0)
    elif act == "sigmoid":
        v = 1 / (1 + torch.exp(-v))
    elif act == "exp":
        v = torch.exp(v)
    elif act == "tanh":
        v = torch.tanh(v)
    return v


def _act_tol(act):
    return LIN_TOL if act in ("none", "relu") else EXP_TOL


def _run_bias_act(dev, X, bias, mode, act, yout):
    ref = _bias_act_oracle(X, bias, mode, act)
    y = ops.bias_act(X.to(dev), _dev(bias, dev), BIAS_MODES[mode], ACTS[act], out_dtype=DT[yout])
    assert y.dtype == DT[yout] and y.device.type == dev
    _check("bias_act_" + act, y, ref, _act_tol(act))


@pytest.mark.parametrize("yout", ["f32", "bf16"])
@pytest.mark.parametrize("xin", ["f32", "bf16"])
@pytest.mark.parametrize("mode", list(BIAS_MODES))
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("R,N", [(33, 65), (1, 1)])
@pytest.mark.parametrize("dev", DEVS)
def test_bias_act(dev, R, N, act, mode, xin, yout):
    g = _gen(R * N)
    X = (torch.randn(R, N, generator=g) * 3).to(DT[xin])
    bias = None if mode == "nobias" else torch.randn(R if mode == "row" else N, generator=g)
    _run_bias_act(dev, X, bias, mode, act, yout)


@pytest.mark.parametrize("yout", ["f32", "bf16"])
@pytest.mark.parametrize("mode", list(BIAS_MODES))
@pytest.mark.parametrize("dev", DEVS)
def test_bias_act_relu_of_nan(dev, mode, yout):
    """relu keeps NaN (as torch.relu and the CPU path do), sends -Inf to 0 and keeps +Inf; ``v > 0 ? v : 0`` and
    ``fmaxf(v, 0)`` both turn NaN into 0. ``_check`` requires the oracle's NaN pattern and its +-Inf exactly."""
    R, N = 5, 9
    g = _gen(95)
    X = torch.randn(R, N, generator=g) * 3
    X[0, 0], X[1, 3], X[2, 5], X[4, 8] = float("nan"), float("-inf"), float("inf"), float("nan")
    bias = None if mode == "nobias" else torch.randn(R if mode == "row" else N, generator=g)
    ref = _bias_act_oracle(X, bias, mode, "relu")
    assert int(ref.isnan().sum()) == 2 and float(ref[1, 3]) == 0.0 and float(ref[2, 5]) == float("inf")
    _run_bias_act(dev, X, bias, mode, "relu", yout)


@pytest.mark.parametrize("act", ["none", "tanh"])
@pytest.mark.parametrize("mode", ["row", "col"])
@pytest.mark.parametrize("dev", DEVS)
def test_bias_act_square_row_vs_col(dev, mode, act):
    """R == N with a different bias per index: a row / column (e / N vs e % N) mix-up changes every off-diagonal
    element and nothing else about the call."""
    n = 48
    g = _gen(48)
    X = torch.randn(n, n, generator=g)
    bias = torch.arange(n, dtype=F32) * 0.25 - 5.0
    _run_bias_act(dev, X, bias, mode, act, "f32")


@pytest.mark.parametrize("mode", ["row", "col"])
@pytest.mark.parametrize("dev", DEVS)
def test_bias_act_past_the_grid_cap(dev, mode):
    """1031 x 2039 = 2 102 209 elements, more than the 8192 x 256 threads of the capped grid: the last 5057
    elements come from the second grid-stride pass. Every row / column has its own bias value."""
    R, N = 1031, 2039
    g = _gen(1031)
    X = torch.randn(R, N, generator=g)
    n = R if mode == "row" else N
    bias = torch.arange(n, dtype=F32) * 0.5 - n / 4
    _run_bias_act(dev, X, bias, mode, "none", "f32")


@pytest.mark.parametrize("yout", ["f32", "bf16"])
@pytest.mark.parametrize("seed", [12345, 2 ** 40 + 7])
@pytest.mark.parametrize("p", [0.25, 0.5])
@pytest.mark.parametrize("R,N", [(33, 65), (1031, 2039)])
@pytest.mark.parametrize("dev", DEVS)
def test_bias_act_dropout(dev, R, N, p, seed, yout):
    """The zeroed set is exactly hash_uniform(seed, flat index) < p; the kept values are ref / (1 - p)."""
    g = _gen(R + N)
    X = (torch.rand(R, N, generator=g) + 0.5) * (torch.randint(0, 2, (R, N), generator=g) * 2 - 1)
    bias = torch.rand(N, generator=g) * 0.5 - 0.25
    ref = _bias_act_oracle(X, bias, "col", "none")
    assert (ref.abs() >= 0.25).all()        # a zero in the output is a dropped element, never a value
    drop = torch.from_numpy(ops.hash_uniform(seed, np.arange(R * N, dtype=np.uint64)) < np.float32(p)).reshape(R, N)
    assert 0 < int(drop.sum()) < R * N
    y = ops.bias_act(X.to(dev), bias.to(dev), ops.BIAS_COL, ops.ACT_NONE, dropout=p, seed=seed, out_dtype=DT[yout])
    y = y.cpu()
    diff = (y == 0) != drop
    assert not diff.any(), f"{int(diff.sum())} elements differ from the host mask, first {diff.nonzero()[0].tolist()}"
    _check("bias_act_dropout", y[~drop], (ref / (1 - p))[~drop], LIN_TOL)


# ------------------------------------------------------------------------------------------------------- lstm_cell

def _lstm_cell_oracle(gates, c_prev):
    g = gates.double()
    H = g.shape[1] // 4
    sig = lambda x: 1 / (1 + torch.exp(-x))  # noqa: E731
    i, f, gg, o = sig(g[:, :H]), sig(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), sig(g[:, 3 * H:])
    c = i * gg if c_prev is None else f * c_prev.double() + i * gg
    return o * torch.tanh(c), c


@pytest.mark.parametrize("with_c", [True, False], ids=["cprev", "nocprev"])
@pytest.mark.parametrize("hout", ["f32", "bf16"])
@pytest.mark.parametrize("gin", ["f32", "bf16"])
@pytest.mark.parametrize("B,H", [(1, 1), (16, 40), (3, 257)])
@pytest.mark.parametrize("dev", DEVS)
def test_lstm_cell(dev, B, H, gin, hout, with_c):
    g = _gen(B * H)
    gates = torch.randn(B, 4 * H, generator=g) * 2
    flat = gates.view(-1)
    flat[::7] = 30.0            # saturated gates, both signs, in all four gate blocks
    flat[3::11] = -30.0
    gates = gates.to(DT[gin])
    c_prev = torch.randn(B, H, generator=g).clamp(-3, 3) if with_c else None
    href, cref = _lstm_cell_oracle(gates, c_prev)
    h, c = ops.lstm_cell(gates.to(dev), _dev(c_prev, dev), h_dtype=DT[hout])
    assert h.dtype == DT[hout] and c.dtype == F32 and h.device.type == dev and c.device.type == dev
    _check("lstm_cell_c", c, cref, LOG_TOL)
    _check("lstm_cell_h", h, href, LOG_TOL)


@pytest.mark.parametrize("dev", DEVS)
def test_lstm_cell_past_the_grid_cap(dev):
    """B * H = 1031 * 2039 elements, more than the 8192 x 256 threads of the capped grid (second grid-stride pass)."""
    B, H = 1031, 2039
    g = _gen(2039)
    gates = torch.randn(B, 4 * H, generator=g) * 2
    c_prev = torch.randn(B, H, generator=g).clamp(-3, 3)
    href, cref = _lstm_cell_oracle(gates, c_prev)
    h, c = ops.lstm_cell(gates.to(dev), c_prev.to(dev))
    _check("lstm_cell_c", c, cref, LOG_TOL)
    _check("lstm_cell_h", h, href, LOG_TOL)


@pytest.mark.parametrize("dev", DEVS)
def test_empty_inputs(dev):
    """Zero rows / elements / bags: an empty result of the right shape and type, no launch over nothing."""
    z = torch.zeros(0, 8).to(dev)
    assert ops.softmax_rows(z).shape == (0, 8) and ops.row_normalize(z, out_dtype=BF16).dtype == BF16
    assert ops.bias_act(z, torch.zeros(8).to(dev), ops.BIAS_COL, ops.ACT_RELU, out_dtype=F32).shape == (0, 8)
    h, c = ops.lstm_cell(z)
    assert h.shape == (0, 2) and c.shape == (0, 2)
    e = torch.zeros(0).to(dev)
    assert ops.lstm_two_sum(e, e, e, e).numel() == 0 and ops.lstm_hidden(e, e).numel() == 0
    table = torch.ones(3, 5).to(dev)
    none = torch.zeros(0, dtype=torch.int64).to(dev)
    assert ops.embedding_bag(table, none, torch.zeros(1, dtype=torch.int64).to(dev)).shape == (0, 5)
    y = ops.embedding_bag(table, none, torch.zeros(3, dtype=torch.int64).to(dev), mode="mean")     # two empty bags
    assert y.shape == (2, 5) and (y == 0).all()
    if dev == "cuda":
        torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------- lstm_ew

# 4096 blocks x 256 threads x 4 floats is one full pass of the capped grid; the last size adds three more 256-thread
# rows of 16-B groups (a partial second pass) and a 3-element scalar tail
LSTM_EW_N = [1, 3, 4, 10010, 4096 * 256 * 4 + 4 * 256 * 3 + 3]


@pytest.mark.parametrize("n", LSTM_EW_N)
@pytest.mark.parametrize("dev", DEVS)
def test_lstm_two_sum(dev, n):
    g = _gen(n)
    f, i = torch.rand(n, generator=g), torch.rand(n, generator=g)           # gate values
    cp = torch.randn(n, generator=g).clamp(-3, 3)
    gg = torch.rand(n, generator=g) * 2 - 1
    ref = f.double() * cp.double() + i.double() * gg.double()
    y = ops.lstm_two_sum(f.to(dev), cp.to(dev), i.to(dev), gg.to(dev))
    assert y.dtype == F32 and y.device.type == dev
    _check("lstm_ew_two_sum", y, ref, LOG_TOL)


@pytest.mark.parametrize("n", LSTM_EW_N)
@pytest.mark.parametrize("dev", DEVS)
def test_lstm_hidden(dev, n):
    g = _gen(n + 1)
    o = torch.rand(n, generator=g)
    c = torch.randn(n, generator=g) * 2
    ref = o.double() * torch.tanh(c.double())
    y = ops.lstm_hidden(o.to(dev), c.to(dev))
    assert y.dtype == F32 and y.device.type == dev
    _check("lstm_ew_hidden", y, ref, LOG_TOL)


# --------------------------------------------------------------------------------------------------- embedding_bag

EB_V = 50
# 5 bags (not a multiple of the 4 waves of a block): empty first, one element, 64 elements, 5 with repeats, empty last
EB_OFFSETS = [0, 0, 1, 65, 70, 70]


def _bag_case(D, tdt, with_w):
    g = _gen(D)
    table = (torch.rand(EB_V, D, generator=g) + 0.5).to(DT[tdt])
    idx = torch.randint(0, EB_V, (70,), generator=g)
    idx[65:70] = torch.tensor([7, 7, 3, 7, 3])
    idx[1], idx[2] = EB_V - 1, 0          # the last and the first table row
    weights = torch.rand(70, generator=g) + 0.5 if with_w else None
    return table, idx, torch.tensor(EB_OFFSETS), weights


def _bag_oracle(table, idx, offsets, weights, mode):
    t = table.double()
    out = torch.zeros(offsets.numel() - 1, t.shape[1], dtype=torch.float64)
    for b in range(offsets.numel() - 1):
        s, e = int(offsets[b]), int(offsets[b + 1])
        for i in range(s, e):
            out[b] += (1.0 if weights is None else float(weights[i])) * t[int(idx[i])]
        if mode == "mean" and e > s:
            out[b] /= e - s
    return out


@pytest.mark.parametrize("with_w", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("tdt", ["f32", "bf16"])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 256, 257, 300, 515])
@pytest.mark.parametrize("dev", DEVS)
def test_embedding_bag(dev, D, tdt, mode, with_w):
    table, idx, offsets, weights = _bag_case(D, tdt, with_w)
    ref = _bag_oracle(table, idx, offsets, weights, mode)
    y = ops.embedding_bag(table.to(dev), idx.to(dev), offsets.to(dev), _dev(weights, dev), mode=mode)
    assert y.dtype == F32 and y.device.type == dev
    assert (y[0] == 0).all() and (y[4] == 0).all()      # empty bags are written, as zeros
    _check("embedding_bag", y, ref, LIN_TOL)


@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("dev", DEVS)
def test_embedding_bag_strided_weights(dev, mode):
    """weights[::2] of a longer vector: the correct result (or a refusal), never a read of it as if it were dense."""
    table, idx, offsets, _ = _bag_case(65, "f32", False)
    wide = torch.rand(140, generator=_gen(140)) + 0.5
    ref = _bag_oracle(table, idx, offsets, wide[::2], mode)
    wd = wide.to(dev)[::2]
    assert not wd.is_contiguous()
    try:
        y = ops.embedding_bag(table.to(dev), idx.to(dev), offsets.to(dev), wd, mode=mode)
    except RuntimeError:
        return
    _check("embedding_bag", y, ref, LIN_TOL)


# ------------------------------------------------------- optional operands must be on the main operand's device

@pytest.mark.parametrize("dev", GPU)
def test_host_operands_are_refused_before_any_launch(dev):
    """A CPU-resident optional operand next to a GPU main operand is an error of the call (RuntimeError), not a
    host pointer handed to a kernel."""
    g = _gen(1)
    X = torch.randn(4, 8, generator=g).to(dev)
    with pytest.raises(RuntimeError):
        ops.softmax_rows(X, torch.zeros(8))
    with pytest.raises(RuntimeError):
        ops.bias_act(X, torch.zeros(8), ops.BIAS_COL, ops.ACT_NONE, out_dtype=F32)
    with pytest.raises(RuntimeError):
        ops.bias_act(X, torch.zeros(4), ops.BIAS_ROW, ops.ACT_NONE, out_dtype=F32)
    with pytest.raises(RuntimeError):
        ops.lstm_cell(X, torch.zeros(4, 2))
    table, idx, offsets, weights = _bag_case(8, "f32", True)
    td, idd, od, wd = table.to(dev), idx.to(dev), offsets.to(dev), weights.to(dev)
    with pytest.raises(RuntimeError):
        ops.embedding_bag(td, idx, od, wd)
    with pytest.raises(RuntimeError):
        ops.embedding_bag(td, idd, offsets, wd)
    with pytest.raises(RuntimeError):
        ops.embedding_bag(td, idd, od, weights)
    torch.cuda.synchronize()
    # the same calls with every operand on the device still work
    _check("embedding_bag", ops.embedding_bag(td, idd, od, wd), _bag_oracle(table, idx, offsets, weights, "sum"),
           LIN_TOL)


@pytest.mark.parametrize("mode", ["row", "col"])
@pytest.mark.parametrize("dev", DEVS)
def test_bias_act_strided_bias(dev, mode):
    """A strided bias view is read through its strides."""
    R, N = 5, 9
    g = _gen(59)
    X = torch.randn(R, N, generator=g)
    wide = torch.randn(2 * (R if mode == "row" else N), generator=g)
    ref = _bias_act_oracle(X, wide[::2], mode, "none")
    y = ops.bias_act(X.to(dev), wide.to(dev)[::2], BIAS_MODES[mode], ops.ACT_NONE, out_dtype=F32)
    _check("bias_act_none", y, ref, LIN_TOL)
    sref = _softmax_oracle(X, wide[::2], False) if mode == "col" else None
    if sref is not None:
        _check("softmax_rows", ops.softmax_rows(X.to(dev), wide.to(dev)[::2]), sref, EXP_TOL)


# -------------------------------------------------------------------------------------------------------- prefetch

def _prefetch_sink(t):
    return ops._PREFETCH_SINK[t.device]


@pytest.mark.parametrize("nbytes", [1, 127, 128, 129, 100003])
@pytest.mark.parametrize("dev", GPU)
def test_prefetch_reads_only(dev, nbytes):
    """Whole 128-B lines only (the sizes straddle one line), nothing written: tensor bit-identical, sink still 0."""
    t = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=_gen(nbytes)).to(dev)
    before = t.clone()
    assert ops.prefetch([t]) is None
    torch.cuda.synchronize()
    assert torch.equal(t, before)
    assert int(_prefetch_sink(t).item()) == 0


@pytest.mark.parametrize("dev", GPU)
def test_prefetch_strided_view_and_several_tensors(dev):
    g = _gen(3)
    base = torch.randn(64, 48, generator=g).to(dev)
    view = base[:, ::2]
    other = torch.randn(1000, generator=g).to(BF16).to(dev)
    assert not view.is_contiguous()
    b0, o0 = base.clone(), other.clone()
    ops.prefetch([view, other, torch.empty(0, device=dev)], blocks=3)
    torch.cuda.synchronize()
    assert torch.equal(base, b0) and torch.equal(other, o0)
    assert int(_prefetch_sink(base).item()) == 0


def test_prefetch_is_a_no_op_on_cpu_tensors():
    t = torch.arange(300, dtype=F32)
    assert ops.prefetch([t, None]) is None
    assert torch.equal(t, torch.arange(300, dtype=F32))
