"""Device relational operators vs the PyTorch composites they replace, interleaved rounds in one process.

  * group-by + sum of 16 M rows (int64 key, one f64 value) at 8, 10 k and 10 M distinct keys:
    hash_aggregate (relops.hip) vs torch.unique(return_inverse) + index_add_;
  * hash join: build 2 M rows, probe 16 M rows (PK-FK, ~1 match per probe) via JoinTable vs sort + searchsorted;
    and a build-size sweep (2 / 16 / 64 M unique build keys, 16 M probes): build, probe, build + probe;
  * partition permutation of 16 M rows over 8 destinations: partition_perm vs argsort(stable) + bincount;
  * ORDER BY ... LIMIT k (K.order_limit, topk.hip) at --rows: one float64 key descending, k = 10 / 100 / 2048, vs
    torch.topk + a sort of the k values; three keys (float64 descending, int32, int64), k = 10, vs the chain of three
    stable argsorts;
  * ORDER BY without LIMIT (K.order_by) at --rows, path="device" (sort.hip) vs path="torch" (the stable-argsort chain):
    one int32 key in a date-like range of 2,500 values, one float64 key, three keys (float64 descending, int32, int64);
  * ORDER BY one string key (StringColumn.order_perm and K.order_by on the column) at --rows, every sort of the chain on
    path="device" vs path="torch": 25 distinct nation names, unique 'Supplier#%09d' names, random lowercase strings
    of 8 to 40 bytes; and once at 1 M rows against the host's sorted(col.tolist()).

    python scripts/bench_relops.py [--rows 16000000] [--rounds 5] [--json out.json]
                                   [--sections order_limit|order_by|order_by_str]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from netsdb_amd import _ext  # noqa: E402
from netsdb_amd.execution import kernels as K  # noqa: E402


def wall(fn, iters=3):
    """Host wall time per call incl. the call's own host syncs (the result sizes are read back)."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def run(fns, rounds):
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            res[k].append(wall(f))
    return {k: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
            for k, v in res.items()}


def bench_order_limit(a, out):
    """K.order_limit against the torch composites it replaces, both arms alternating in the same rounds."""
    dev = "cuda:0"
    n = a.rows
    g = torch.Generator(device=dev).manual_seed(1)
    out["order_limit"] = {}
    x = torch.rand(n, device=dev, dtype=torch.float64, generator=g)
    for k in (10, 100, 2048):
        def dev_ol():
            return K.order_limit([x], k, True)

        def torch_topk_sort():
            v, i = torch.topk(x, min(k, n), sorted=False)
            return i[torch.sort(v, descending=True, stable=True).indices]

        assert torch.equal(x[dev_ol()], x[torch_topk_sort()]), "order_limit differs from torch.topk"
        t = run({"order_limit": dev_ol, "torch_topk_sort": torch_topk_sort}, a.rounds)
        t["keys"], t["k"] = "f64 desc", k
        out["order_limit"][f"1key_k{k}"] = t
        print(json.dumps({"order_limit": f"1key_k{k}", **t}), flush=True)
    # three keys: about 16 rows share each value of key 0, so keys 1 and 2 decide inside its groups
    rev = torch.floor(x * (n / 16)) / (n / 16)
    od = torch.randint(0, 2500, (n,), device=dev, generator=g, dtype=torch.int32)
    ok = torch.randint(0, 1 << 40, (n,), device=dev, generator=g, dtype=torch.int64)
    del x

    def dev_ol3():
        return K.order_limit([rev, od, ok], 10, [True, False, False])

    def torch_argsort3():
        order = torch.argsort(ok, stable=True)
        order = order[torch.argsort(od[order], stable=True)]
        return order[torch.argsort(rev[order], descending=True, stable=True)][:10]

    assert torch.equal(dev_ol3(), torch_argsort3()), "order_limit differs from the argsort chain"
    t = run({"order_limit": dev_ol3, "torch_argsort_chain": torch_argsort3}, a.rounds)
    t["keys"], t["k"] = "f64 desc, i32, i64", 10
    out["order_limit"]["3key_k10"] = t
    print(json.dumps({"order_limit": "3key_k10", **t}), flush=True)


def bench_order_by(a, out):
    """K.order_by: the device radix sort against the argsort chain, both arms alternating in the same rounds."""
    dev = "cuda:0"
    n = a.rows
    g = torch.Generator(device=dev).manual_seed(2)
    out["order_by"] = {}
    x = torch.rand(n, device=dev, dtype=torch.float64, generator=g)
    od = torch.randint(0, 2500, (n,), device=dev, generator=g, dtype=torch.int32)
    ok = torch.randint(0, 1 << 40, (n,), device=dev, generator=g, dtype=torch.int64)
    rev = torch.floor(x * (n / 16)) / (n / 16)         # about 16 rows share each value: keys 1 and 2 decide inside
    shapes = (("1key_i32_dates", "i32 in [0, 2500)", [od], [False]),
              ("1key_f64", "f64", [x], [False]),
              ("3key", "f64 desc, i32, i64", [rev, od, ok], [True, False, False]))
    for name, what, keys, desc in shapes:
        def device_arm():
            return K.order_by(keys, desc, path="device")

        def torch_arm():
            return K.order_by(keys, desc, path="torch")

        assert torch.equal(device_arm(), torch_arm()), "order_by: the device arm differs from the argsort chain"
        t = run({"order_by_device": device_arm, "order_by_torch": torch_arm}, a.rounds)
        t["keys"], t["rows"] = what, n
        t["plan"] = K.order_by_plan([c.dtype for c in keys], n, True, "device")["path"]
        out["order_by"][name] = t
        print(json.dumps({"order_by": name, **t}), flush=True)


NATIONS = ["ALGERIA", "ARGENTINA", "BRAZIL", "CANADA", "EGYPT", "ETHIOPIA", "FRANCE", "GERMANY", "INDIA", "INDONESIA",
           "IRAN", "IRAQ", "JAPAN", "JORDAN", "KENYA", "MOROCCO", "MOZAMBIQUE", "PERU", "CHINA", "ROMANIA",
           "SAUDI ARABIA", "VIETNAM", "RUSSIA", "UNITED KINGDOM", "UNITED STATES OF AMERICA"]


def _string_shapes(n, dev, g):
    """The three string key columns of the order_by_str section, built on the device (no n-row host list)."""
    from netsdb_amd.objects.strings import StringColumn

    def packed(data, off, payload, maxlen):
        buf = torch.zeros(((payload + 16 + 3) // 4) * 4, dtype=torch.uint8, device=dev)
        buf[:payload] = data
        return StringColumn(buf, off, payload, maxlen=maxlen)

    nation = StringColumn.from_list(NATIONS, dev).take(torch.randint(0, len(NATIONS), (n,), device=dev, generator=g))
    ids = torch.randperm(n, device=dev, generator=g) + 1
    digits = (ids.unsqueeze(1) // (10 ** torch.arange(8, -1, -1, device=dev)).unsqueeze(0)) % 10 + ord("0")
    prefix = torch.tensor(list(b"Supplier#"), dtype=torch.uint8, device=dev).expand(n, 9)
    supp = packed(torch.cat([prefix, digits.to(torch.uint8)], 1).flatten(), torch.arange(n + 1, device=dev) * 18,
                  18 * n, 18)
    lens = torch.randint(8, 41, (n,), device=dev, generator=g)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=off[1:])
    total = int(off[-1])
    text = packed(torch.randint(ord("a"), ord("z") + 1, (total,), device=dev, generator=g, dtype=torch.uint8), off,
                  total, 40)
    return (("nation_25_distinct", "25 distinct names, L = 24", nation),
            ("supplier_unique", "'Supplier#%09d' unique, L = 18", supp),
            ("lowercase_8_40", "random lowercase, 8..40 bytes", text))


def bench_order_by_str(a, out):
    """ORDER BY one string key (StringColumn.order_perm: order words + the LSD chain over K.order_by; K.order_by on
    the column: that chain, the dense ranks, and the sort of the ranks): path="device" against path="torch" for every
    sort of the chain, both arms alternating in the same rounds; then once at 1 M rows against the host
    sorted(col.tolist()) that a caller had to do before. ``col[:]`` is a fresh column over the same buffers each call,
    so no call finds kept ranks."""
    from netsdb_amd.objects.strings import string_order_plan

    dev = "cuda:0"
    out["order_by_str"] = {}
    for n, host in ((a.rows, False), (1_000_000, True)):
        g = torch.Generator(device=dev).manual_seed(3)
        for name, what, col in _string_shapes(n, dev, g):
            fns = {f"{fn}_{path}": (lambda fn=fn, path=path: (
                col[:].order_perm(path=path) if fn == "order_perm" else K.order_by([col[:]], path=path)))
                for fn in ("order_perm", "order_by") for path in ("device", "torch")}
            ref = fns["order_perm_device"]()
            for k, f in fns.items():
                assert torch.equal(f(), ref), f"order_by_str: {k} differs"
            t = run(fns, a.rounds)
            t["keys"], t["rows"] = what, n
            t["groups"] = string_order_plan(col.max_len(), n)["groups"]
            if host:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                strs = col.tolist()
                t1 = time.perf_counter()
                ordered = sorted(strs)
                t2 = time.perf_counter()
                assert ordered == [strs[i] for i in ref.cpu().tolist()], "order_by_str: differs from the host sort"
                t["host_tolist_ms"], t["host_sorted_ms"] = round((t1 - t0) * 1e3, 1), round((t2 - t1) * 1e3, 1)
                t["default"] = run({"order_perm_default": lambda: col[:].order_perm()}, a.rounds)["order_perm_default"]
            key = f"{name}_{n}"
            out["order_by_str"][key] = t
            print(json.dumps({"order_by_str": key, **t}), flush=True)
            del col, fns, ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--sections", default="all",
                    help="all, or order_limit / order_by / order_by_str alone (the other sections run together)")
    a = ap.parse_args()
    out = {"rows": a.rows}
    alone = ("order_limit", "order_by", "order_by_str")
    if a.sections not in alone:
        bench_tables(a, out)
    if a.sections not in alone or a.sections == "order_limit":
        bench_order_limit(a, out)
    if a.sections not in alone or a.sections == "order_by":
        bench_order_by(a, out)
    if a.sections not in alone or a.sections == "order_by_str":
        bench_order_by_str(a, out)
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


def bench_tables(a, out):
    """The group-by, join and partition sections."""
    dev = "cuda:0"
    n = a.rows
    g = torch.Generator(device=dev).manual_seed(0)
    h = _ext.hip()
    out.update({"groupby": {}, "join": {}, "partition": {}})
    vals = torch.rand(n, device=dev, dtype=torch.float64, generator=g)
    for distinct in (8, 1000, 3000, 5000, 10_000, 10_000_000):
        keys = torch.randint(0, distinct, (n,), device=dev, generator=g) * 2654435761
        ref_u, ref_inv = torch.unique(keys, return_inverse=True)
        ref = torch.zeros(ref_u.numel(), device=dev, dtype=torch.float64).index_add_(0, ref_inv, vals)
        r = h.hash_aggregate(keys, vals, "sum", False, 0)
        order = torch.argsort(r[0])
        assert torch.equal(r[0][order], ref_u), "group keys differ"
        err = ((r[1][order, 0] - ref).abs().max() / ref.abs().max()).item()

        def dev_agg():
            return h.hash_aggregate(keys, vals, "sum", False, 0)

        def dev_agg_inv():
            return h.hash_aggregate(keys, vals, "sum", True, 0)

        def dev_agg_nofirst():   # the engine's numeric-key group-by: no representative rows needed
            return h.hash_aggregate(keys, vals, "sum", False, 0, False)

        r2 = dev_agg_nofirst()
        o2 = torch.argsort(r2[0])
        assert torch.equal(r2[0][o2], ref_u) and torch.allclose(r2[1][o2, 0], ref, rtol=1e-9), "no-first path differs"

        def torch_agg():
            u, inv = torch.unique(keys, return_inverse=True)
            return torch.zeros(u.numel(), device=dev, dtype=torch.float64).index_add_(0, inv, vals)

        def dev_agg_part():      # the same call with the MID path off (A/B: MID vs PART)
            h.agg_set_mid(False)
            try:
                return h.hash_aggregate(keys, vals, "sum", False, 0)
            finally:
                h.agg_set_mid(True)

        arms = {"hash_aggregate": dev_agg, "hash_aggregate_no_first": dev_agg_nofirst,
                "hash_aggregate_with_inverse": dev_agg_inv, "torch_unique_index_add": torch_agg}
        if 8 < distinct < 1_000_000:
            arms["hash_aggregate_mid_off"] = dev_agg_part
        t = run(arms, a.rounds)
        t["groups"] = int(ref_u.numel())
        t["path"] = ("LOW/MID", "PART")[int(r[5][1])]
        t["sample_distinct"] = int(r[5][3])
        t["max_rel_err"] = err
        out["groupby"][str(distinct)] = t
        print(json.dumps({"groupby": distinct, **t}), flush=True)
        del keys, ref_u, ref_inv, ref, r
    # join: build = 2M distinct keys (PK side), probe = 16M FK keys
    nb = max(1, n // 8)
    build = torch.randperm(nb, device=dev, generator=g) * 7 + 1
    probe = (torch.randint(0, nb, (n,), device=dev, generator=g) * 7 + 1)
    probe[::10] = -5   # 10 % without a match

    def dev_join():
        return K.JoinTable(build).probe(probe)

    def torch_join():
        sh, order = torch.sort(build)
        lo = torch.searchsorted(sh, probe)
        hi = torch.searchsorted(sh, probe, right=True)
        cnt = hi - lo
        pi = torch.repeat_interleave(torch.arange(n, device=dev), cnt)
        starts = torch.repeat_interleave(lo, cnt)
        csum = torch.cumsum(cnt, 0)
        offs = torch.arange(pi.numel(), device=dev) - torch.repeat_interleave(csum - cnt, cnt)
        return order[starts + offs], pi

    bi, pi = dev_join()
    assert torch.equal(build[bi], probe[pi]) and pi.numel() == int((probe > 0).sum())
    jt = K.JoinTable(build)
    t = run({"join_table_build_probe": dev_join, "join_probe_only": lambda: jt.probe(probe),
             "torch_sort_searchsorted": torch_join}, a.rounds)
    t["build_rows"], t["probe_rows"], t["matches"] = nb, n, int(pi.numel())
    out["join"] = t
    print(json.dumps({"join": t}), flush=True)
    del jt, bi, pi
    # build-size sweep: unique-key builds of 2 / 16 / 64 M rows, each probed by 16 M keys (~90 % matching)
    out["join_sweep"] = {}
    for nb2 in (2_000_000, 16_000_000, 64_000_000):
        b2 = torch.randperm(nb2, device=dev, generator=g) * 7 + 1
        p2 = torch.randint(0, nb2, (n,), device=dev, generator=g) * 7 + 1
        p2[::10] = -5
        jt2 = K.JoinTable(b2)
        bi2, pi2 = jt2.probe(p2)
        assert torch.equal(b2[bi2], p2[pi2]) and pi2.numel() == int((p2 > 0).sum())
        t = run({"build": lambda: K.JoinTable(b2), "probe": lambda: jt2.probe(p2),
                 "build_probe": lambda: K.JoinTable(b2).probe(p2)}, a.rounds)
        # the same probe against a table built without its probe filter (~90 % of the probes match: the filter
        # word is a second dependent read for most rows)
        _ext.hip().join_set_bloom(False)
        try:
            jt3 = K.JoinTable(b2)
        finally:
            _ext.hip().join_set_bloom(True)
        t.update({"probe_no_filter": run({"p": lambda: jt3.probe(p2)}, a.rounds)["p"]})
        del jt3
        t["build_rows"], t["probe_rows"], t["matches"] = nb2, n, int(pi2.numel())
        out["join_sweep"][str(nb2)] = t
        print(json.dumps({"join_sweep": nb2, **t}), flush=True)
        del b2, p2, jt2, bi2, pi2
    dest = torch.randint(0, 8, (n,), device=dev, generator=g)
    t = run({"partition_perm": lambda: K.partition_order(dest, 8),
             "torch_argsort_bincount": lambda: (torch.argsort(dest, stable=True),
                                                torch.bincount(dest, minlength=8).tolist())}, a.rounds)
    out["partition"] = t
    print(json.dumps({"partition": t}), flush=True)


if __name__ == "__main__":
    main()
