"""The block GEMM's launch plan (csrc/kernels/gemm_plan.h) on the CPU: the header is plain C++, so a ~30-line driver
(tests/native/gemm_plan_dump.cpp) built with the host compiler prints the plan of any call. Needs no GPU and no built
extension. Three checks: the plan reproduces what the three separate host functions it replaced answered
(tests/golden/gemm_plan_parent.json, recorded from the commit before the plan existed), a hand-checked table of named
plans, and one case per error code."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "netsdb_amd", "csrc", "kernels")
FIELDS = ("M", "N", "K", "batch", "splits", "cfg", "epi", "mfma", "fixup", "kinter", "out_f32", "accumulate",
          "bias_mode", "lda", "ldb", "ldc", "sC", "c_align", "seg_k", "has_ws")


@pytest.fixture(scope="module")
def plan_of(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{KDIR}",
                    os.path.join(ROOT, "tests", "native", "gemm_plan_dump.cpp"), "-o", exe], check=True, timeout=120)

    def run(calls):
        """Plans (dicts) of a list of calls (dicts of GemmCall fields; strides default to a contiguous call)."""
        lines = []
        for c in calls:
            d = dict(batch=1, splits=0, cfg=-1, epi=-1, mfma=0, fixup=0, kinter=0, out_f32=0, accumulate=0,
                     bias_mode=0, lda=c["K"], ldb=c["K"], ldc=c["N"], sC=0, c_align=16, seg_k=0, has_ws=1)
            d.update(c)
            lines.append(" ".join(str(int(d[f])) for f in FIELDS))
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True,
                             timeout=120).stdout.splitlines()
        assert len(out) == len(calls)
        plans = []
        for line in out:
            kv = dict(t.split("=") for t in line.split())
            plans.append({k: v if k in ("kernel", "reducer") else int(v) for k, v in kv.items()})
        return plans

    return run


def test_plan_reproduces_the_parents_host_functions(plan_of):
    """gemm_splits(M, N, K, batch, cfg), gemm_launch_wgs and gemm_prefetch_eligible(M, N, K, batch, splits, cfg) of the
    commit before gemm_plan.h, over a fixed sweep (every 43rd point of the product of the golden file's value sets):
    the plan gives every recorded value exactly."""
    with open(os.path.join(ROOT, "tests", "golden", "gemm_plan_parent.json")) as f:
        rows = json.load(f)["rows"]
    assert 1000 < len(rows) <= 2000
    auto = plan_of([dict(M=r[0], N=r[1], K=r[2], batch=r[3], cfg=r[4]) for r in rows])
    req = plan_of([dict(M=r[0], N=r[1], K=r[2], batch=r[3], cfg=r[4], splits=r[5]) for r in rows])
    bad = [(r, a["splits"], q["wgs"], q["prefetch_eligible"]) for r, a, q in zip(rows, auto, req)
           if (a["splits"], q["wgs"], q["prefetch_eligible"]) != tuple(r[6:9]) or a["rc"] or q["rc"]]
    assert not bad, (len(bad), bad[:5])


L1 = dict(M=1000, N=1000, K=65536, cfg=2, splits=16)      # the layer-1 shape class, K scaled down
EPI = dict(M=1000, N=1032, K=1024, cfg=2, splits=1)
NAMED = [
    # the headline FF layer 1: 16 tiles x 16 splits of 584 k-tiles fill the 256 CUs
    ("layer1", dict(M=1000, N=1000, K=597568),
     dict(cfg=2, splits=16, kchunk=584 * 64, kernel="8ph", reducer="plain", reduce_blocks=977, wgs=256,
          direct_epi=1, prefetch_eligible=1)),
    # the FF output layer: 228 tiles keep >= 3/4 of the chip busy, no split
    ("output_layer", dict(M=1000, N=14588, K=1000),
     dict(cfg=2, splits=1, kernel="8ph", reducer="none", wgs=228, direct_epi=1, prefetch_eligible=0)),
    ("dedup", dict(M=500, N=100, K=900000),
     dict(cfg=3, tbm=256, tbn=128, splits=128, kernel="stream256x128", reducer="wide", reduce_blocks=196, wgs=256)),
    ("dedup_t", dict(M=100, N=500, K=900000), dict(cfg=4, tbm=128, tbn=256, splits=128, kernel="stream128x256")),
    ("small", dict(M=128, N=128, K=64), dict(cfg=0, splits=1, kernel="tile128", reducer="none", wgs=1)),
    # ldc = 1030: C rows are not 16-B aligned, the register epilogue is off and with it the 32x32x16 loop
    ("mfma32_n1030", dict(EPI, N=1030, mfma=32), dict(vec_c=0, direct_epi=0, kernel="8ph")),
    ("mfma32_n1032", dict(EPI, mfma=32), dict(vec_c=1, direct_epi=1, kernel="8ph32")),
    ("mfma32_split_n1030", dict(EPI, N=1030, mfma=32, splits=4), dict(vec_ws=0, direct_epi=0, kernel="8ph")),
    ("mfma32_split_n1032", dict(EPI, mfma=32, splits=4), dict(direct_epi=1, kernel="8ph32", reducer="plain")),
    ("fixup", dict(L1, fixup=1), dict(splits=16, kernel="8ph_fixup", reducer="in_launch", reduce_blocks=0)),
    # 300 x 1028 at 32 splits: (308400 / 4 + 255) / 256 = 302 reducer blocks < 512, the wide reducer's case
    ("fixup_narrow", dict(M=300, N=1028, K=64000, cfg=2, splits=32, fixup=1),
     dict(splits=32, kernel="8ph", reducer="wide")),
    ("fixup_over_32", dict(M=1000, N=1000, K=65536, cfg=2, splits=40, fixup=1),
     dict(splits=40, kernel="8ph", reducer="plain")),
    ("fixup_mfma32", dict(L1, fixup=1, mfma=32), dict(kernel="8ph32", reducer="plain")),
    ("fixup_batched", dict(L1, fixup=1, batch=2), dict(kernel="8ph", reducer="plain", wgs=512)),
    ("fixup_ragged_n", dict(L1, N=1001, fixup=1), dict(vec_ws=0, direct_epi=0, kernel="8ph", reducer="plain")),
    ("epi_0", dict(EPI, epi=0), dict(direct_epi=0, kernel="8ph")),
    ("accumulate", dict(EPI, accumulate=1, out_f32=1), dict(direct_epi=0)),
    ("bias_matrix", dict(EPI, bias_mode=3), dict(direct_epi=0)),
    ("bf16_c_8B_aligned", dict(EPI, c_align=8), dict(vec_c=1, direct_epi=1)),
    ("f32_c_8B_aligned", dict(EPI, c_align=8, out_f32=1), dict(vec_c=0, direct_epi=0)),
    # stream tile, 8 splits of 128 k-tiles; on segmented B a split must stay inside one segment: kinter is dropped
    ("kinter", dict(M=500, N=100, K=65536, cfg=3, splits=8, kinter=1), dict(kinter=1, kchunk=8192)),
    ("kinter_segmented", dict(M=500, N=100, K=65536, cfg=3, splits=8, kinter=1, seg_k=8192), dict(rc=0, kinter=0)),
    ("kinter_8ph", dict(L1, kinter=1), dict(kinter=0)),
    # 25 k-tiles asked in 3: chunks of 9; 10 k-tiles asked in 7: chunks of 2, which 5 splits cover
    ("split_rounding", dict(M=256, N=256, K=1600, cfg=2, splits=3), dict(splits=3, kchunk=9 * 64)),
    ("split_dropped", dict(M=256, N=256, K=640, cfg=2, splits=7), dict(splits=5, kchunk=2 * 64)),
    ("empty", dict(M=0, N=100, K=64), dict(rc=0, wgs=0)),
]


@pytest.mark.parametrize("name", [n for n, _, _ in NAMED])
def test_named_plan(plan_of, name):
    call, want = next((c, w) for n, c, w in NAMED if n == name)
    plan = plan_of([call])[0]
    assert plan["rc"] == want.get("rc", 0)
    assert {k: plan[k] for k in want} == want


@pytest.mark.parametrize("rc,call", [
    (-1, dict(M=64, N=64, K=12)),                                        # K % 8
    (-1, dict(M=64, N=64, K=64, lda=68)),                                # rows not 16-B
    (-2, dict(M=64, N=64, K=64, ldb=4194304)),                           # 256 rows x ldb x 2 B past the buffer range
    (-3, dict(M=256, N=256, K=4096, splits=4, has_ws=0)),                # split-K without a workspace
    (-4, dict(M=64, N=64, K=64, accumulate=1, out_f32=0)),               # C += into bf16
    (-8, dict(M=64, N=64, K=64, cfg=1)),                                 # not a production config
    (-8, dict(M=64, N=64, K=64, cfg=7)),
    (-5, dict(M=256, N=256, K=1536, cfg=2, splits=4, seg_k=192)),        # kchunk 384 crosses the 192 segments
    (-1, dict(M=64, N=64, K=12, cfg=1, accumulate=1)),                   # the first failed check wins
])
def test_error_codes(plan_of, rc, call):
    assert plan_of([call])[0]["rc"] == rc
