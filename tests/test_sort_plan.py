"""The device ORDER BY's launch plan (csrc/kernels/sort_plan.h) on the CPU: the header is plain C++, so a small driver
(tests/native/sort_plan_dump.cpp) built with the host compiler prints the plan of any call. Needs no GPU and no built
extension. A hand-checked table of plans, one case per error code, and scratch_bytes = the sum of the listed buffers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "netsdb_amd", "csrc", "kernels")
I32, F32, I64, F64 = 0, 1, 2, 3
TILE = 4096                       # 256 threads x 16 rows
# state: hist[32][256] + base[32][256] + 3 words per slot + 4 key flags + 4 (total, padding), u32 each
STATE = 4 * (2 * 32 * 256 + 3 * 32 + 4 + 4)


@pytest.fixture(scope="module")
def plan_of(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("sort_plan") / "sort_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{KDIR}",
                    os.path.join(ROOT, "tests", "native", "sort_plan_dump.cpp"), "-o", exe], check=True, timeout=120)

    def run(dts, n):
        d = list(dts) + [0] * (4 - min(4, len(dts)))
        line = f"{len(dts)} {n} " + " ".join(str(x) for x in d[:4]) + "\n"
        out = subprocess.run([exe], input=line, capture_output=True, text=True, check=True, timeout=120).stdout
        return {k: int(v) for k, v in (t.split("=") for t in out.split())}

    return run


NAMED = [
    # one tile; 4 passes; hist + plan + 1 load + 3 x 4 + out = 16 launches; ceil(2049 / 1024) histogram workgroups
    ("i32_2049", [I32], 2049,
     dict(word_bits=32, tile=TILE, tiles=1, passes=4, launches=16, scan_step=256, hist_grid=3,
          counts_bytes=4 * 256 * 1, words_bytes=2 * 2049 * 4, ids_bytes=2 * 2049 * 4)),
    # one row past a tile: two tiles; 8 passes; 2 + 1 + 24 + 1 launches
    ("f64_tile_plus_1", [F64], TILE + 1,
     dict(word_bits=64, tiles=2, passes=8, launches=28, hist_grid=5,
          counts_bytes=4 * 256 * 2, words_bytes=2 * 4097 * 8, ids_bytes=2 * 4097 * 4)),
    # the largest call: 2^19 tiles, 32 passes, 2 + 4 + 96 + 1 launches, the histogram grid at its cap
    ("four_wide_keys_max_n", [I64, F64, I64, F64], 2 ** 31 - 1,
     dict(word_bits=64, tiles=2 ** 19, passes=32, launches=103, hist_grid=1024,
          counts_bytes=4 * 256 * 2 ** 19, words_bytes=16 * (2 ** 31 - 1), ids_bytes=8 * (2 ** 31 - 1))),
    # one 8-byte key among 4-byte ones widens every word; 4 + 8 + 4 passes; ceil(100000 / 4096) = 25 tiles
    ("mixed", [F32, I64, I32], 100000,
     dict(word_bits=64, tiles=25, passes=16, launches=54, hist_grid=98,
          counts_bytes=4 * 256 * 25, words_bytes=2 * 100000 * 8, ids_bytes=2 * 100000 * 4)),
    ("two_narrow_keys", [F32, I32], 5000, dict(word_bits=32, tiles=2, passes=8, launches=29)),
]


@pytest.mark.parametrize("name", [n for n, _, _, _ in NAMED])
def test_named_plan(plan_of, name):
    dts, n, want = next((d, n, w) for nm, d, n, w in NAMED if nm == name)
    plan = plan_of(dts, n)
    assert plan["rc"] == 0
    assert {k: plan[k] for k in want} == want
    assert plan["state_bytes"] == STATE
    assert plan["scratch_bytes"] == plan["state_bytes"] + plan["counts_bytes"] + plan["words_bytes"] + plan["ids_bytes"]


@pytest.mark.parametrize("rc,dts,n", [
    (-1, [], 100),                       # no key
    (-1, [I32] * 5, 100),                # five keys
    (-2, [I32, 4], 100),                 # no such dtype
    (-2, [-1], 100),
    (-3, [I32], 0),                      # n outside [1, 2^31)
    (-3, [I32], -5),
    (-3, [F64], 2 ** 31),
    (-1, [I32] * 5, 0),                  # the first failed check wins
    (-2, [7], 2 ** 31),
])
def test_error_codes(plan_of, rc, dts, n):
    assert plan_of(dts, n)["rc"] == rc


def test_tiles_cover_the_rows(plan_of):
    for n in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 200003):
        p = plan_of([I64], n)
        assert (p["tiles"] - 1) * p["tile"] < n <= p["tiles"] * p["tile"]
