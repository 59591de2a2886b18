"""The packed-operand request of the block GEMM's launch plan (csrc/kernels/gemm_plan.h GemmCall::packed) on the CPU,
through a host driver of its own (tests/native/gemm_plan_packed.cpp: the plan with the request and the plan of the same
call without it). The request is honoured for the FF layer-1 call (kernel "8ph_pk", everything else as without it) and
dropped, leaving exactly the plan the call has today, for every launch the packed kernel form does not cover."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "netsdb_amd", "csrc", "kernels")
FIELDS = ("M", "N", "K", "batch", "splits", "cfg", "epi", "mfma", "fixup", "kinter", "out_f32", "accumulate",
          "bias_mode", "lda", "ldb", "ldc", "sC", "c_align", "seg_k", "has_ws", "packed")


@pytest.fixture(scope="module")
def plans_of(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gemm_plan_packed") / "gemm_plan_packed")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{KDIR}",
                    os.path.join(ROOT, "tests", "native", "gemm_plan_packed.cpp"), "-o", exe], check=True, timeout=120)

    def parse(text):
        kv = dict(t.split("=") for t in text.split())
        return {k: v if k in ("kernel", "reducer") else int(v) for k, v in kv.items()}

    def run(call):
        """(plan with the request, plan without it) of one call (a dict of GemmCall fields)."""
        d = dict(batch=1, splits=0, cfg=-1, epi=-1, mfma=0, fixup=0, kinter=0, out_f32=0, accumulate=0, bias_mode=0,
                 lda=call["K"], ldb=call["K"], ldc=call["N"], sC=0, c_align=16, seg_k=0, has_ws=1, packed=0)
        d.update(call)
        line = " ".join(str(int(d[f])) for f in FIELDS) + "\n"
        out = subprocess.run([exe], input=line, capture_output=True, text=True, check=True, timeout=120).stdout
        with_req, without = out.strip().split("|")
        return parse(with_req), parse(without)

    return run


LAYER1 = dict(M=1000, N=1000, K=597568)
L1 = dict(M=1000, N=1000, K=65536, cfg=2, splits=16)


@pytest.mark.parametrize("packed", [1, 2])
@pytest.mark.parametrize("call", [LAYER1, L1, dict(M=200, N=264, K=64, cfg=2), dict(L1, bias_mode=2, out_f32=1),
                                  dict(L1, N=1001), dict(L1, epi=0, splits=1)],
                         ids=["layer1", "l1_small_k", "one_tile", "bias_f32", "ragged_n", "lds_epilogue"])
def test_request_honoured(plans_of, call, packed):
    got, base = plans_of(dict(call, packed=packed))
    assert base["kernel"] == "8ph" and base["packed"] == 0 and base["rc"] == 0
    assert got == dict(base, kernel="8ph_pk", packed=packed)


def test_layer1_plan_is_todays(plans_of):
    """The headline call keeps its 16 tiles x 16 splits of 584 k-tiles, the plain reducer and the prefetch."""
    got, _ = plans_of(dict(LAYER1, packed=2))
    want = dict(cfg=2, splits=16, kchunk=584 * 64, kernel="8ph_pk", reducer="plain", reduce_blocks=977, wgs=256,
                direct_epi=1, prefetch_eligible=1, packed=2)
    assert {k: got[k] for k in want} == want


DROPPED = [
    ("mfma32", dict(L1, mfma=32), "8ph32"),
    ("mfma32_lds_epilogue", dict(L1, N=1001, mfma=32), "8ph"),       # the 16x16x32 loop runs, the request still goes
    ("fixup", dict(L1, fixup=1), "8ph_fixup"),
    ("seg_k", dict(L1, seg_k=8192, ldb=8192), "8ph"),
    ("batch2", dict(L1, batch=2, sC=1000 * 1000), "8ph"),
    ("cfg0", dict(L1, cfg=0), "tile128"),
    ("cfg3", dict(M=1000, N=128, K=65536, cfg=3), "stream256x128"),
    ("cfg4", dict(M=128, N=1000, K=65536, cfg=4), "stream128x256"),
    ("auto_small", dict(M=128, N=128, K=64), "tile128"),
    # 32768 k-tiles x 1024 padded rows x 128 B = 2^32 bytes: one 32-bit buffer cannot cover the copy
    ("oversized_k", dict(M=1000, N=1000, K=32768 * 64, cfg=2), "8ph"),
    ("unknown_request", dict(L1, packed=3), "8ph"),
]


@pytest.mark.parametrize("packed", [1, 2])
@pytest.mark.parametrize("name", [n for n, _, _ in DROPPED])
def test_request_dropped(plans_of, name, packed):
    call, kernel = next((c, k) for n, c, k in DROPPED if n == name)
    got, base = plans_of(dict(dict(packed=packed), **call))
    assert base["rc"] == 0 and base["kernel"] == kernel
    assert got == base and got["packed"] == 0


def test_size_bound_is_the_copy_of_the_packed_side(plans_of):
    """One k-tile less than the oversized case fits; the bound looks at the packed operand's own rows (256 rows of
    B at the oversized K are a quarter of the bytes)."""
    got, _ = plans_of(dict(M=1000, N=1000, K=32767 * 64, cfg=2, packed=1))
    assert got["kernel"] == "8ph_pk"
    big = dict(M=1000, N=256, K=32768 * 64, cfg=2)
    assert plans_of(dict(big, packed=1))[0]["packed"] == 0
    assert plans_of(dict(big, packed=2))[0]["packed"] == 2
