"""dbgen .tbl ingestion throughput (models/tpch_tbl.py): write generated TPC-H tables at scale factor SF in dbgen's
format, then time load_tbl (chunked read + device parse + dispatch into the sets) per table. One JSON line per run.

``--path torch|device`` picks the parser (a comma list interleaves them run by run over the same files); ``--runs``
repeats the timed load. Next to the end-to-end time every line carries a parse-only figure: HIP events around parse_tbl
over every chunk of every table, the chunks already resident on the device, after one warm-up pass."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_only_ms(tpch_tbl, T, d, dev, chunk_bytes, path):
    """Milliseconds of parse_tbl alone over every chunk of every table, by device events (GPU only)."""
    if not dev.startswith("cuda"):
        return None
    total = 0.0
    for name in T.TABLES:
        p = os.path.join(d, f"{name}.tbl")
        chunks = [torch.from_numpy(tpch_tbl.read_chunk(p, lo, hi)).to(dev) for lo, hi in tpch_tbl.chunk_bounds(p, chunk_bytes)]
        for buf in chunks:                                    # warm-up: code objects, allocator pools
            tpch_tbl.parse_tbl(buf, name, dev, path)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for buf in chunks:
            tpch_tbl.parse_tbl(buf, name, dev, path)
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1)
        del chunks
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=1.0)
    ap.add_argument("--chunk-mb", type=int, default=256)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--path", default=None, help="torch | device | a comma list to interleave (default: load_tbl's own)")
    ap.add_argument("--runs", type=int, default=1)
    a = ap.parse_args()
    from netsdb_amd.client import PDBClient
    from netsdb_amd.models import tpch as T
    from netsdb_amd.models import tpch_gen, tpch_tbl

    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    d = a.dir or tempfile.mkdtemp(prefix="tbl_")
    t0 = time.perf_counter()
    tables = tpch_gen.generate_fast(a.sf, seed=1)
    tpch_tbl.write_tbl(tables, d)
    t_write = time.perf_counter() - t0
    del tables
    paths = a.path.split(",") if a.path else [None]
    c = PDBClient(root=tempfile.mkdtemp(), device=dev)
    for i, p in enumerate(paths):                             # a warm-up load: first-launch costs out of the timing
        tpch_tbl.load_tbl(c, f"warm{i}", d, device=dev, chunk_bytes=a.chunk_mb << 20, path=p)
        c.remove_database(f"warm{i}")
    for run in range(a.runs):
        for p in paths:
            db = f"tpch_{run}_{p}"
            t1 = time.perf_counter()
            st = tpch_tbl.load_tbl(c, db, d, device=dev, chunk_bytes=a.chunk_mb << 20, path=p)
            total = time.perf_counter() - t1
            c.remove_database(db)
            nbytes = sum(v["bytes"] for v in st.values())
            rows = sum(v["rows"] for v in st.values())
            pm = parse_only_ms(tpch_tbl, T, d, dev, a.chunk_mb << 20, p)
            print(json.dumps({"sf": a.sf, "device": dev, "path": p or "default", "run": run, "bytes": nbytes,
                              "rows": rows, "seconds": round(total, 3), "GB_per_s": round(nbytes / total / 1e9, 3),
                              "Mrows_per_s": round(rows / total / 1e6, 2),
                              "parse_only_ms": None if pm is None else round(pm, 2),
                              "parse_only_GB_per_s": None if pm is None else round(nbytes / pm / 1e6, 2),
                              "write_seconds": round(t_write, 1),
                              "tables": {k: {"rows": v["rows"], "MB": round(v["bytes"] / 1e6, 1), "s": round(v["seconds"], 3)}
                                         for k, v in st.items()}}), flush=True)
    if a.dir is None:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
