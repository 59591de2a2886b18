"""The delimited-text parser's launch plan (csrc/kernels/textparse_plan.h) on the CPU: the header is plain C++, so a
small driver (tests/native/textparse_plan_dump.cpp) built with the host compiler prints the plan of any call. Needs no
GPU and no built extension. A hand-checked table of plans, one case per refusal code, and scratch_bytes = the sum of
the listed buffers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "netsdb_amd", "csrc", "kernels")
TILE = 16384                      # 256 threads x 4 loads x 16 bytes
STEP = 256                        # tiles per scan step
STATE = 8 * 4                     # rows | lowest bad row | flagged cells | spare, u64 each
BAR = 124


@pytest.fixture(scope="module")
def plan_of(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("textparse_plan") / "textparse_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{KDIR}",
                    os.path.join(ROOT, "tests", "native", "textparse_plan_dump.cpp"), "-o", exe], check=True, timeout=120)

    def run(nbytes, nfields, delim=BAR):
        out = subprocess.run([exe], input=f"{nbytes} {nfields} {delim}\n", capture_output=True, text=True, check=True,
                             timeout=120).stdout
        return {k: int(v) for k, v in (t.split("=") for t in out.split())}

    return run


NAMED = [
    ("one_byte", 1, 1, dict(tile=TILE, tiles=1, scan_step=STEP, launches=4, counts_bytes=4)),
    ("one_tile", TILE, 16, dict(tiles=1, counts_bytes=4)),
    ("one_tile_plus_1", TILE + 1, 16, dict(tiles=2, counts_bytes=8)),
    # one tile past a scan step: the scan takes two steps
    ("scan_step_tiles_plus_1", STEP * TILE + 1, 64, dict(tiles=STEP + 1, counts_bytes=4 * (STEP + 1))),
    # the largest accepted buffer: 2^31 - 1 bytes = 2^17 tiles
    ("largest", 2 ** 31 - 1, 3, dict(tiles=2 ** 17, counts_bytes=4 * 2 ** 17, launches=4)),
]


@pytest.mark.parametrize("name", [n for n, _, _, _ in NAMED])
def test_named_plan(plan_of, name):
    nbytes, nf, want = next((b, f, w) for nm, b, f, w in NAMED if nm == name)
    plan = plan_of(nbytes, nf)
    assert plan["rc"] == 0
    assert {k: plan[k] for k in want} == want
    assert plan["state_bytes"] == STATE
    assert plan["scratch_bytes"] == plan["counts_bytes"] + plan["state_bytes"]
    assert (plan["tiles"] - 1) * plan["tile"] < nbytes <= plan["tiles"] * plan["tile"]


@pytest.mark.parametrize("rc,nbytes,nf,delim", [
    (-1, 0, 3, BAR),                     # empty buffer
    (-1, -7, 3, BAR),
    (-2, 2 ** 31, 3, BAR),               # 2^31 bytes or more
    (-3, 100, 0, BAR),                   # fields outside 1..64
    (-3, 100, 65, BAR),
    (-4, 100, 3, 10),                    # the delimiter is a line end
    (-4, 100, 3, 13),
    (-4, 100, 3, 256),                   # not one byte
    (-1, 0, 0, 10),                      # the first failed check wins
    (-2, 2 ** 31, 65, 13),
])
def test_refusals(plan_of, rc, nbytes, nf, delim):
    assert plan_of(nbytes, nf, delim)["rc"] == rc


def test_data_dependent_buffers(plan_of):
    p = plan_of(100, 3)
    assert p["rows_bytes_1000"] == 4 * 1001       # u32 row starts, one past the end
    assert p["flags_bytes_10"] == 160             # two u64 per flagged cell


def test_any_single_byte_delimiter_but_line_ends(plan_of):
    assert all(plan_of(100, 3, d)["rc"] == (-4 if d in (10, 13) else 0) for d in (0, 9, 44, 124, 255, 10, 13))
