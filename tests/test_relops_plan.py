"""The relational operators' host plan (csrc/kernels/relops_plan.h) on the CPU: the header is plain C++, so a small
driver (tests/native/relops_plan_dump.cpp) built with the host compiler prints the plan of any call. Needs no GPU and
no built extension.

1. The plan reproduces the commit before it: tests/golden/relops_plan_parent.json holds that commit's work-buffer byte
   counts and tile counts (its relops.hip host functions, run over a fixed sweep) and its table capacities (_sizes of
   tests/test_groupby_oracle.py, to which the GPU suite holds the kernels). Every recorded value, exactly.
2. Every layout of the sweep is sound: offsets ascend, each region starts at its type's alignment (16 bytes for the
   partition key buffers; for the group-by's per-workgroup key ranges, which agg_hist_kernel reads 16 bytes at a time),
   the last region ends inside the total, a table has (cap + 1) * (4 + F) words.
3. One case per rejection; the first failed check wins.
The same sweep runs once more under -fsanitize=undefined,address where the host compiler has them."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "netsdb_amd", "csrc", "kernels")
SRC = os.path.join(ROOT, "tests", "native", "relops_plan_dump.cpp")
with open(os.path.join(ROOT, "tests", "golden", "relops_plan_parent.json")) as _f:
    GOLD = json.load(_f)
NS, FS, PBITS, PS, CAPB, THR = (GOLD[k] for k in ("n", "F", "pbits", "P", "cap_bits", "thr"))
JOIN_DEFAULTS = "1 4194304 4194304 1"      # filter on, 4 MiB / 4 MiB, partitioned build on


def _sweep_requests():
    req = []
    for n in NS:
        req.append(f"tiles {n}")
        for F in FS:
            req += [f"aggwork {n} {F} {pb}" for pb in PBITS]
            req += [f"agg {n} {F} {thr} 1 1 1" for thr in THR]
        req += [f"part {n} {P}" for P in PS]
        req += [f"jpart {n} {1 << cb} 0 -1" for cb in CAPB if 2 * n <= 1 << cb]
        if n < 2 ** 29:
            req.append(f"join {n} 0 {JOIN_DEFAULTS}")
    return req


def _build(cxx, exe, extra=()):
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *extra, f"-I{KDIR}", SRC, "-o", exe], check=True,
                   timeout=300)


def _ask(exe, requests):
    out = subprocess.run([exe], input="\n".join(requests) + "\n", capture_output=True, text=True, check=True,
                         timeout=300).stdout.splitlines()
    assert len(out) == len(requests)
    return [{k: int(v) for k, v in (t.split("=") for t in ln.split())} for ln in out]


@pytest.fixture(scope="module")
def cxx():
    c = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if c is None:
        pytest.skip("no host C++ compiler")
    return c


@pytest.fixture(scope="module")
def exe(cxx, tmp_path_factory):
    e = str(tmp_path_factory.mktemp("relops_plan") / "relops_plan_dump")
    _build(cxx, e)
    return e


@pytest.fixture(scope="module")
def sweep(exe):
    req = _sweep_requests()
    return dict(zip(req, _ask(exe, req)))


def test_constants(exe):
    c = _ask(exe, ["consts"])[0]
    assert c == dict(kSample=4096, kMetaStructWords=16, kMetaWords=16 + 4096, kMidPMax=3, kLdsLow=64 << 10,
                     kLdsPart=128 << 10, kLdsMid=160 << 10, kJRegionBits=12, kJRegion=4096, kJWholeWrap=1 << 22,
                     kJPartMaxRegions=8192, kJPartOneLevel=2048, kJPartCoarse=256, kJStageBins=1024, kJTile=4096,
                     kCompactTile=8192, kTakeCols=48)


def test_plan_reproduces_parent_bytes_and_tiles(sweep):
    for i, n in enumerate(NS):
        t = sweep[f"tiles {n}"]
        assert (t["join_tiles"], t["compact_tiles"]) == (GOLD["join_tiles"][i], GOLD["compact_tiles"][i]), n
        for j, F in enumerate(FS):
            for pb in PBITS:
                assert sweep[f"aggwork {n} {F} {pb}"]["total"] == GOLD["agg_work_bytes"][i][j][pb], (n, F, pb)
        for j, P in enumerate(PS):
            p = sweep[f"part {n} {P}"]
            assert p["rc"] == 0 and p["total"] == GOLD["part_work_bytes"][i][j], (n, P)
        for j, cb in enumerate(CAPB):
            want = GOLD["jpart_work_bytes"][i][j]
            assert (want is None) == (2 * n > 1 << cb)
            if want is not None:
                p = sweep[f"jpart {n} {1 << cb} 0 -1"]
                assert p["rc"] == (0 if cb <= 25 else -6) and p["total"] == want, (n, cb)      # at most 8192 regions


def test_plan_reproduces_parent_capacities(sweep):
    fields = GOLD["sizes_fields"]
    assert fields == ["lcap_low", "lcap_part", "lcap_mid", "gcap_low", "low_thr", "pbits"]
    for i, n in enumerate(NS):
        for j, F in enumerate(FS):
            for k, thr in enumerate(THR):
                p = sweep[f"agg {n} {F} {thr} 1 1 1"]
                got = [p["lcap_low"], p["lcap_part"], p["lcap_mid"], p["glow_cap"], p["low_thr"], p["pbits"]]
                assert p["rc"] == 0 and got == GOLD["sizes"][i][j][k], (n, F, thr)
                # the plan's own work buffer is the one of its pbits, and the reported bytes add up as the binding's did
                assert p["total"] == GOLD["agg_work_bytes"][i][j][p["pbits"]]
                assert p["gpart_cap"] == max(4096, min(1 << 17, 1 << (2 * n - 1).bit_length()))
                assert p["ocap_low"] == min(n, p["glow_cap"] + 1)
                assert p["phase1_bytes"] == 8 * (16 + 4096 + p["glow_words"] + n + p["ocap_low"] * (4 + F))
                assert p["part_bytes"] == 8 * (p["gpart_words"] + n * (4 + F)) + p["total"]


def _ascending(p, names, sizes, total_key="total"):
    """Regions `names` of byte sizes `sizes` lie in this order without overlap and end inside the total."""
    for a, b, sz in zip(names, names[1:], sizes):
        assert p[a] + sz <= p[b], (a, b, p)
    assert p[names[-1]] + sizes[-1] <= p["end"] <= p[total_key], p


def test_layouts_are_sound(sweep):
    for n in NS:
        for F in FS:
            for thr in THR:
                p = sweep[f"agg {n} {F} {thr} 1 1 1"]
                P, G = p["P"], p["G"]
                assert P == 1 << p["pbits"] and G == min(256, max(1, -(-n // 16384)))
                assert G * p["rpw"] >= n and (p["rpw"] * 8) % 16 == 0
                _ascending(p, ["hist", "tot", "bstart", "pkey", "pval", "prow", "qkey", "qval", "qrow"],
                           [4 * P * G, 8 * P, 8 * (P + 1), 8 * n, 8 * n * F, 4 * n, 8 * n, 8 * n * F, 4 * n])
                assert p["hist"] % 4 == 0 and p["prow"] % 4 == 0 and p["qrow"] % 4 == 0
                assert all(p[k] % 8 == 0 for k in ("tot", "bstart", "pval", "qval"))
                assert p["pkey"] % 16 == 0 and p["qkey"] % 16 == 0
                for t in ("glow", "gpart"):
                    s = p[f"{t}_cap"] + 1
                    assert p[f"{t}_words"] == s * (4 + F)
                    assert [p[f"{t}_{f}"] for f in ("key", "acc", "cnt", "rmin", "gid")] == \
                        [0, s, s + s * F, 2 * s + s * F, 3 * s + s * F]
                for o in ("out1", "out2"):
                    c = p[f"{o}_ocap"]
                    assert c == (p["ocap_low"] if o == "out1" else n) and p[f"{o}_words"] == c * (4 + F)
                    assert [p[f"{o}_{f}"] for f in ("reps", "aggs", "cnt", "slot_of_gid", "first")] == \
                        [0, c, c * (1 + F), c * (2 + F), c * (3 + F)]
                # LDS: every launch inside its budget
                assert p["lds_low"] == p["lcap_low"] * (20 + 8 * F) <= 64 << 10
                assert p["lds_mid"] == p["lcap_mid"] * (20 + 8 * F) <= 160 << 10
                assert p["lds_stage"] == p["T"] * (14 + 8 * F) <= 128 << 10 and p["lds_hist"] == 4 * P
                assert p["lds_bucket"] == max(p["T2"] * (14 + 8 * F), p["lcap_part"] * (20 + 8 * F)) <= 128 << 10
        for P in PS:
            p = sweep[f"part {n} {P}"]
            G = p["G"]
            assert G == min(256, max(1, -(-n // 16384))) and G * p["rpw"] >= n
            _ascending(p, ["hist", "tot", "bstart"], [4 * P * G, 8 * P, 8 * (P + 1)])
            assert p["tot"] % 8 == 0 and p["bstart"] % 8 == 0
            assert p["lds_hist"] == 4 * P and p["lds_scatter"] == 68 * P <= 160 << 10
        for cb in CAPB:
            if 2 * n > 1 << cb:
                continue
            p = sweep[f"jpart {n} {1 << cb} 0 -1"]
            P, G, Pc, sh = p["P"], p["G"], p["Pc"], p["sh"]
            assert P == 1 << (cb - 12) and Pc == P >> sh
            assert G == min(1024, max(1, -(-n // 16384))) and G * p["rpw"] >= n
            assert (sh == 0) == (P <= 2048) and (sh == 0 or Pc == 256) and p["staged"] == (sh > 0 and Pc + 1 <= 1024)
            names = ["hist", "btot", "cbase", "bbase", "ikey", "islot", "irank", "irow"]
            sizes = [4 * (Pc + 1) * G, 8 * (Pc + 1), 8 * (Pc + 2), 8 * (P + 2), 8 * n, 4 * n, 4 * n, 4 * n]
            if sh:
                names += ["ikey1", "irow1"]
                sizes += [8 * n, 4 * n]
            else:
                assert p["ikey1"] == p["ikey"] and p["irow1"] == p["irow"]
            _ascending(p, names, sizes)
            assert all(p[k] % 8 == 0 for k in ("btot", "cbase", "bbase"))
            assert all(p[k] % 4 == 0 for k in ("islot", "irank", "irow", "irow1"))
            assert p["ikey"] % 16 == 0 and p["ikey1"] % 16 == 0


def test_join_plan_steps(sweep, exe):
    """Load factor, table kind and filter at the sizes where each changes (default settings)."""
    want = {  # n: load, cap, regions, part, filter words, fold
        1: (8, 1024, 0, 0, 0, 0),
        2 ** 18: (8, 1 << 21, 0, 0, 1 << 16, 0),
        2 ** 18 + 1: (4, 1 << 21, 0, 0, 1 << 17, 0),
        2 ** 20 + 1: (4, 1 << 23, 1, 1, 1 << 19, 1),
        2 ** 21 + 1: (4, 1 << 24, 1, 1, 0, 0),
        2 ** 22: (4, 1 << 24, 1, 1, 0, 0),
        2 ** 22 + 1: (2, 1 << 24, 1, 1, 0, 0),
        2 ** 24: (2, 1 << 25, 1, 1, 0, 0),
    }
    for n, w in want.items():
        p = sweep[f"join {n} 0 {JOIN_DEFAULTS}"]
        assert (p["load"], p["cap"], p["regions"], p["part"], p["W"], p["fold"]) == w, (n, p)
        assert p["bshift"] == (p["cap"] // p["W"]).bit_length() - 1 if p["W"] else p["bshift"] == -1
        if p["part"]:
            assert p["rc"] == 0 and p["total"] == sweep[f"jpart {n} {p['cap']} 0 -1"]["total"]
    # more than kJPartMaxRegions regions, or the partitioned build switched off: the global insert; a rebuild's slots
    big, off, re = _ask(exe, [f"join {2 ** 25} 0 {JOIN_DEFAULTS}", f"join {2 ** 20 + 1} 0 1 4194304 4194304 0",
                              f"join {2 ** 20 + 1} {1 << 24} {JOIN_DEFAULTS}"])
    assert (big["cap"], big["regions"], big["part"]) == (1 << 26, 1, 0)
    assert (off["cap"], off["regions"], off["part"], off["fold"], off["W"]) == (1 << 23, 1, 0, 0, 1 << 19)
    assert (re["cap"], re["part"], re["W"], re["bshift"], re["fold"]) == (1 << 24, 1, 1 << 19, 5, 1)


@pytest.mark.parametrize("rc,request_line", [
    # agg_plan: agg n F low_threshold mid want_inv want_first
    (-2, "agg 0 2 0 1 0 1"),                    # n outside [1, 2^31)
    (-2, f"agg {2 ** 31} 2 0 1 0 1"),
    (-3, "agg 100 -1 0 1 0 1"),                 # F outside [0, 16]
    (-3, "agg 100 17 0 1 0 1"),
    (-1, "agg 100 100000 0 1 0 1"),             # an entry wider than the LDS: the MID table is checked first
    (-3, "agg 100 100000 1 1 0 1"),             # ... no MID path (explicit threshold): F is out of range
    (-2, f"agg {2 ** 31} 17 0 1 0 1"),          # the first failed check wins: n before F
    # agg_call_rc: call n F phase have_inv have_part_buffers vrs vcs (want_inv = 1)
    (0, "call 100 2 0 1 1 2 1"),
    (-7, "call 100 2 4 1 1 2 1"),               # no such phase
    (-7, "call 100 2 -1 0 0 -1 1"),
    (-8, "call 100 2 1 0 1 2 1"),               # want_inv without the buffer
    (-9, "call 100 2 2 1 0 2 1"),               # PART phases need the table and the work buffer
    (-9, "call 100 2 0 1 0 2 1"),
    (0, "call 100 2 1 1 0 2 1"),                # ... LOW phases do not
    (0, "call 100 2 3 1 0 2 1"),
    (-10, "call 100 2 1 1 1 -2 1"),             # negative strides
    (-10, "call 100 2 1 1 1 2 -1"),
    (0, "call 100 0 1 1 1 -2 -1"),              # ... which no column reads at F = 0
    (-3, "call 100 17 9 0 0 -1 -1"),            # a bad plan before any of these
    # join_part_plan: jpart n cap filter bshift
    (-1, f"jpart 0 {1 << 23} 0 -1"),
    (-2, f"jpart 1000 {1 << 22} 0 -1"),         # a whole-table probe order: not built by regions
    (-3, f"jpart 1000 {(1 << 23) + 4096} 0 -1"),
    (-4, f"jpart {(1 << 22) + 1} {1 << 23} 0 -1"),      # load above 1/2
    (-5, f"jpart 1000 {1 << 31} 0 -1"),
    (-6, f"jpart 1000 {1 << 26} 0 -1"),         # 16384 regions
    (-7, f"jpart 1000 {1 << 23} 1 1"),          # a folded filter word covers 4 .. 4096 slots
    (-7, f"jpart 1000 {1 << 23} 1 13"),
    (0, f"jpart 1000 {1 << 23} 1 2"),
    (0, f"jpart 1000 {1 << 23} 1 12"),
    (0, f"jpart 1000 {1 << 23} 0 13"),          # ... no filter: the shift is not looked at
    (-1, f"jpart 0 {1 << 22} 1 1"),             # the first failed check wins
    (-2, f"jpart 5 1000 1 1"),
    # part_plan: part n P
    (-1, "part 100 0"),
    (-1, "part 100 2049"),
    (-2, "part 0 16"),
    (-2, f"part {2 ** 31} 16"),
    (-1, f"part {2 ** 31} 0"),
])
def test_error_codes(exe, rc, request_line):
    assert _ask(exe, [request_line])[0]["rc"] == rc


def test_sweep_under_sanitizers(cxx, sweep, tmp_path):
    """The same sweep from a driver built with -fsanitize=undefined,address: same answers, no report."""
    e = str(tmp_path / "relops_plan_dump_san")
    san = ["-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g"]
    probe = subprocess.run([cxx, *san, "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}",
                           capture_output=True, text=True, timeout=120)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True,
                                               timeout=120).returncode != 0:
        pytest.skip("the host compiler has no undefined / address sanitizer, or its runtime does not start here")
    _build(cxx, e, san)
    req = list(sweep)
    assert _ask(e, req) == [sweep[r] for r in req]
