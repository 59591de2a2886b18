"""Delimited-text ingestion for any flat schema: ``.tbl`` / CSV lines parsed into the columns of a ``PDBObject`` type.

Reference: the reference system loads text wherever it loads data: src/tpch/source/tpchDataLoader.cc (``:65`` splits a
line on '|', ``:480-653`` load the eight tables) and the CSV-reading FF / dedup / text-classifier drivers under
src/tests/source, each a per-line host tokenizer that builds one object per row.

MI355X-native design: a chunk of whole lines is parsed on the device by csrc/kernels/textparse.hip (newline counts per
16 KiB tile, a scan, the row starts in order, then one lane per row decoding every field in one walk). Nothing
proportional to rows x field width is built. Two paths share one contract:

* ``path="device"``: the kernels. A cell outside its kind's FAST GRAMMAR (below) is flagged, not failed: the loader
  decodes just those cells on the host with Python's ``int()`` / ``float()`` and reports how many (``host_cells``).
* ``path="host"``: split lines, split fields, Python's own ``int`` / ``float``. Deliberately plain: it is the oracle the
  device path is tested against.

Field kinds, from the schema annotation:

=============================  =================  ==========================================================
annotation                     stored as          fast grammar
=============================  =================  ==========================================================
``int``                        int64              ``-?[0-9]{1,18}``
``float``                      float64            ``-?[0-9]*(\\.[0-9]*)?``, 1..15 digits in all
``bool``                       torch.bool         ``0 1 true false True False``
``Date32`` / a class in dates  int32 yyyymmdd     ``[0-9]{4}-[0-9]{2}-[0-9]{2}`` (no fallback: else an error)
``str``                        StringColumn/list  any bytes
=============================  =================  ==========================================================

A float is ``(double)mantissa / 10**frac`` with the sign applied to the double: one IEEE division of two exactly
representable doubles, which equals ``float(text)`` for every string of the grammar, so ``-0.00`` is ``-0.0``.

Rows end at ``\\n`` (a ``\\r`` right before it is dropped; the last row may lack its ``\\n``) and must hold exactly the
expected number of delimiters: ``trailing=True`` means one after every field (dbgen), ``False`` between fields only
(CSV). A malformed row or a bad date raises ``ValueError`` naming the 1-based line of the LOWEST such line.

Known limits: no quoting or escapes, no NULLs, a single-byte delimiter, UTF-8 bytes passed through unexamined.
"""
from __future__ import annotations

import os
import re
import time
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _ext
from ..objects.record import RecordBatch
from ..objects.strings import StringColumn, use_device_strings

SKIP, INT, FLOAT, BOOL, DATE, STR = range(6)
ERR_ROW, ERR_DATE = 1, 2
NL, CR = 10, 13
MAX_CHUNK = (1 << 31) - (1 << 20)        # offsets are 32-bit: a chunk stays below 2^31 bytes

_INT_RE = re.compile(rb"-?[0-9]{1,18}")
_FLOAT_RE = re.compile(rb"-?([0-9]*)(?:\.([0-9]*))?")
_DATE_RE = re.compile(rb"[0-9]{4}-[0-9]{2}-[0-9]{2}")
_BOOLS = {b"0": False, b"1": True, b"true": True, b"false": False, b"True": True, b"False": False}
_DTYPE = {INT: torch.int64, FLOAT: torch.float64, BOOL: torch.bool, DATE: torch.int32}


# ------------------------------------------------------------------------------------------------ schema
def _delim_byte(delimiter) -> int:
    d = delimiter.encode() if isinstance(delimiter, str) else bytes(delimiter)
    if len(d) != 1 or d[0] in (NL, CR):
        raise ValueError(f"delimiter must be one byte other than a line end, got {delimiter!r}")
    return d[0]


def _kind_of(name: str, ft, dates) -> int:
    if ft is bool:
        return BOOL
    if ft is float:
        return FLOAT
    if ft is str:
        return STR
    if ft is int:
        return INT
    if isinstance(ft, type) and issubclass(ft, int):
        return DATE if ft.__name__ == "Date32" or ft in dates or ft.__name__ in dates else INT
    raise TypeError(f"field {name!r} of kind {ft!r} cannot be read from delimited text (flat int / float / bool / "
                    "date / str schemas only)")


def file_columns(type_, fields: Optional[Sequence[Optional[str]]] = None, dates=()) -> List[Tuple[Optional[str], int]]:
    """[(field name or None, kind)] per column of the file. Raises TypeError for a schema that is not flat, ValueError
    when ``fields`` does not name every schema field exactly once."""
    schema = type_.fields()
    dates = tuple(dates)
    kinds = {n: _kind_of(n, ft, dates) for n, ft in schema.items()}
    names = list(schema) if fields is None else list(fields)
    seen = [n for n in names if n is not None]
    unknown = [n for n in seen if n not in schema]
    if unknown:
        raise ValueError(f"unknown field name(s) {unknown} for {type_.type_name()}")
    missing = [n for n in schema if seen.count(n) != 1]
    if missing:
        raise ValueError(f"field(s) {missing} of {type_.type_name()} must appear exactly once in the file's columns")
    return [(n, SKIP if n is None else kinds[n]) for n in names]


def parse_plan(nbytes: int, nfields: int, delimiter="|") -> dict:
    """The device parser's launch plan (csrc/kernels/textparse_plan.h): rc, tile, tiles, scan_step, launches and the
    scratch bytes by buffer. Launches nothing."""
    d = delimiter.encode() if isinstance(delimiter, str) else bytes(delimiter)
    return dict(_ext.hip().text_parse_plan(int(nbytes), int(nfields), d[0] if len(d) == 1 else -1))


# ------------------------------------------------------------------------------------------------ cells
def in_fast_grammar(kind: int, cell: bytes) -> bool:
    if kind == INT:
        return _INT_RE.fullmatch(cell) is not None
    if kind == FLOAT:
        m = _FLOAT_RE.fullmatch(cell)
        return m is not None and 1 <= len(m.group(1)) + len(m.group(2) or b"") <= 15
    if kind == BOOL:
        return cell in _BOOLS
    return True


def _decode_cell(kind: int, cell: bytes, line: int, name: str):
    """Python's own reading of one numeric / bool cell; ValueError with the line and the field otherwise."""
    try:
        text = cell.decode()
        if kind == INT:
            v = int(text)
            if not -(1 << 63) <= v < (1 << 63):
                raise ValueError("outside int64")
            return v
        if kind == FLOAT:
            return float(text)
        t = text.strip().lower()
        if t in ("1", "true"):
            return True
        if t in ("0", "false"):
            return False
        raise ValueError("not a bool")
    except ValueError as e:
        what = {INT: "int", FLOAT: "float", BOOL: "bool"}[kind]
        raise ValueError(f"line {line}, field {name!r}: cannot read {cell!r} as {what} ({e})") from None


def _row_error(code: int, line: int, nfields: int, trailing: bool) -> ValueError:
    if code == ERR_DATE:
        return ValueError(f"line {line}: a date field is not YYYY-MM-DD")
    want = nfields if trailing else nfields - 1
    return ValueError(f"line {line}: malformed row, expected exactly {want} delimiters "
                      f"({'one after every field' if trailing else 'between fields only'})")


# ------------------------------------------------------------------------------------------------ host path
def _parse_host(data: bytes, cols, delim: int, trailing: bool, line0: int, stats: dict, device):
    d = bytes([delim])
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":                 # the text ended with its newline (or is empty)
        lines.pop()
    nf = len(cols)
    want = nf if trailing else nf - 1
    rows: List[List[bytes]] = []
    for i, ln in enumerate(lines):                 # structure and dates first: the lowest bad line wins
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        cells = ln.split(d)
        if ln.count(d) != want or (trailing and cells[-1] != b""):
            raise _row_error(ERR_ROW, line0 + i, nf, trailing)
        if trailing:
            cells.pop()
        for (name, kind), c in zip(cols, cells):
            if kind == DATE and _DATE_RE.fullmatch(c) is None:
                raise _row_error(ERR_DATE, line0 + i, nf, trailing)
        rows.append(cells)
    out: Dict[str, Any] = {}
    host_cells = 0
    for j, (name, kind) in enumerate(cols):
        if kind == SKIP:
            continue
        cells = [r[j] for r in rows]
        if kind == STR:
            out[name] = StringColumn.from_list(cells, device) if use_device_strings(device) else [c.decode() for c in cells]
        elif kind == DATE:
            out[name] = torch.tensor([int(c.replace(b"-", b"")) for c in cells], dtype=torch.int32)
        else:
            host_cells += sum(not in_fast_grammar(kind, c) for c in cells)
            vals = [_decode_cell(kind, c, line0 + i, name) for i, c in enumerate(cells)]
            out[name] = torch.tensor(vals, dtype=_DTYPE[kind])
    stats["host_cells"] = stats.get("host_cells", 0) + host_cells
    return out, len(rows)


# ------------------------------------------------------------------------------------------------ device path
def _string_buffer(buf: torch.Tensor) -> torch.Tensor:
    """The chunk as the string kernels want it (4-byte aligned, a multiple of 4 and at least 16 bytes): itself when it
    already is, otherwise a padded copy."""
    if buf.numel() % 4 == 0 and buf.numel() >= 16 and buf.data_ptr() % 4 == 0:
        return buf
    sbuf = torch.zeros(StringColumn._alloc_size(buf.numel()), dtype=torch.uint8, device=buf.device)
    sbuf[: buf.numel()] = buf
    return sbuf


def _parse_device(buf: torch.Tensor, nbytes: int, cols, delim: int, trailing: bool, line0: int, stats: dict):
    st, outs, flagged = _ext.hip().text_parse(buf, nbytes, [k for _, k in cols], delim, trailing)
    rows, code, bad, ncell = (int(x) for x in st.tolist())
    if code:
        raise _row_error(code, line0 + bad, len(cols), trailing)
    out: Dict[str, Any] = {}
    sbuf = None
    for (name, kind), t in zip(cols, outs):
        if kind == SKIP:
            continue
        if kind == STR:
            if sbuf is None:
                sbuf = _string_buffer(buf)
            out[name] = StringColumn.view(sbuf, t[0], t[1], nbytes, max(1, rows)).compact()
        else:
            out[name] = t
    if ncell:
        # the cells outside the fast grammar: their bytes in one gather, Python's reading, one scatter per column
        fl = flagged.cpu().numpy().astype(np.uint64)
        fl = fl[np.argsort(fl[:, 0], kind="stable")]              # by (row, field): the lowest line fails first
        r, f = (fl[:, 0] >> np.uint64(8)).astype(np.int64), (fl[:, 0] & np.uint64(0xFF)).astype(np.int64)
        s, e = (fl[:, 1] >> np.uint64(32)).astype(np.int64), (fl[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        off = np.zeros(len(s) + 1, dtype=np.int64)
        np.cumsum(e - s, out=off[1:])
        idx = np.repeat(s - off[:-1], e - s) + np.arange(off[-1])
        raw = buf[torch.from_numpy(idx).to(buf.device)].cpu().numpy().tobytes() if off[-1] else b""
        vals: Dict[int, Tuple[List[int], List[Any]]] = {}
        for k in range(len(s)):
            name, kind = cols[f[k]]
            v = _decode_cell(kind, raw[off[k]: off[k + 1]], line0 + int(r[k]), name)
            vals.setdefault(int(f[k]), ([], []))
            vals[int(f[k])][0].append(int(r[k]))
            vals[int(f[k])][1].append(v)
        for j, (ri, vs) in vals.items():
            name, kind = cols[j]
            out[name][torch.tensor(ri, dtype=torch.int64).to(buf.device)] = \
                torch.tensor(vs, dtype=_DTYPE[kind]).to(buf.device)
    stats["host_cells"] = stats.get("host_cells", 0) + ncell
    return out, rows


def parse_delimited(buf: torch.Tensor, type_, *, delimiter="|", trailing: bool = True,
                    fields: Optional[Sequence[Optional[str]]] = None, dates=(), path: Optional[str] = None,
                    stats: Optional[dict] = None, line0: int = 1, nbytes: Optional[int] = None) -> RecordBatch:
    """One chunk of whole lines (1-D uint8 tensor) -> a RecordBatch of ``type_``.

    ``fields``: the file's columns in order as field names, ``None`` for a column to skip (default: the schema's own
    order). ``dates``: int subclasses (or their names) to read as YYYY-MM-DD besides ``Date32``. ``path``: ``"device"``
    (the kernels; a CUDA buffer's default; raises on a CPU tensor) or ``"host"`` (the plain oracle; a CPU buffer's
    default). ``stats["host_cells"]`` gains the number of cells decoded by Python. ``line0``: the file line number of
    the chunk's first line, for error messages. ``nbytes``: the text's length when ``buf`` is a longer (padded)
    allocation; no load passes ``buf``'s end either way."""
    if buf.dtype != torch.uint8 or buf.dim() != 1:
        raise TypeError("parse_delimited: buf must be a 1-D uint8 tensor")
    cols = file_columns(type_, fields, dates)
    delim = _delim_byte(delimiter)
    if not 1 <= len(cols) <= 64:
        raise ValueError(f"{len(cols)} columns per row: the parser takes 1..64")
    if path is None:
        path = "device" if buf.is_cuda else "host"
    if path not in ("device", "host"):
        raise ValueError(f"path must be 'device' or 'host', got {path!r}")
    if path == "device" and not buf.is_cuda:
        raise ValueError("path='device' needs a GPU buffer")
    nb = buf.numel() if nbytes is None else int(nbytes)
    if not 0 <= nb <= buf.numel():
        raise ValueError("nbytes exceeds the buffer")
    stats = stats if stats is not None else {}
    stats["path"] = path
    if path == "host" or nb == 0:
        out, n = _parse_host(bytes(buf[:nb].cpu().numpy()), cols, delim, bool(trailing), line0, stats, buf.device)
        if buf.is_cuda:
            out = {k: (v.to(buf.device) if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    else:
        if nb >= 1 << 31:
            raise ValueError("a chunk must be smaller than 2^31 bytes (32-bit offsets): parse it in pieces")
        out, n = _parse_device(buf.contiguous(), nb, cols, delim, bool(trailing), line0, stats)
        if not use_device_strings(buf.device):
            out = {k: (v.tolist() if isinstance(v, StringColumn) else v) for k, v in out.items()}
    stats["rows"] = stats.get("rows", 0) + n
    return RecordBatch({name: out[name] for name in type_.fields()}, n, type_)


# ------------------------------------------------------------------------------------------------ files
def chunk_bounds(path: str, start: int = 0, chunk_bytes: int = 256 << 20) -> List[Tuple[int, int]]:
    """[(lo, hi)] byte ranges of line-aligned chunks of a file from ``start`` (each ends after a newline, or at EOF)."""
    size = os.path.getsize(path)
    if size <= start:
        return []
    mm = np.memmap(path, dtype=np.uint8, mode="r")
    out, lo = [], start
    while lo < size:
        hi = min(size, lo + max(1, chunk_bytes))
        while hi < size:
            win = mm[max(lo, hi - (1 << 20)): hi]
            k = np.flatnonzero(win == NL)
            if k.size:
                hi = hi - win.size + int(k[-1]) + 1
                break
            hi = min(size, hi + (1 << 20))            # a line longer than the window: widen
        out.append((lo, hi))
        lo = hi
    return out


def _first_lines(path: str, header: bool) -> Tuple[Optional[bytes], Optional[bytes], int]:
    """(header line or None, first data line or None, byte offset of the data), line ends dropped."""
    with open(path, "rb") as f:
        head = None
        if header:
            head = f.readline()
            if not head:
                return None, None, 0
        start = f.tell()
        first = f.readline()
    strip = lambda b: b.rstrip(b"\n").removesuffix(b"\r")      # noqa: E731
    return (strip(head) if head is not None else None), (strip(first) if first else None), start


def load_delimited(client, db: str, name: str, path: str, *, delimiter="|", trailing: Optional[bool] = None,
                   header: bool = False, fields: Optional[Sequence[Optional[str]]] = None, dates=(),
                   chunk_bytes: int = 256 << 20, policy=None) -> dict:
    """Ingest a delimited-text file into the existing set ``db.name``, whose type is the schema. Rank 0 reads
    line-aligned chunks (pinned, one H2D copy each), parses each on the client's device and dispatches it by the set's
    partition policy (send_data: a collective, so every rank takes part chunk by chunk). ``trailing=None`` decides
    from the first data line; ``header=True`` skips the first line (it still counts in error messages' line numbers).
    Returns {rows, bytes, seconds, chunks, host_cells}."""
    uset = client.storage.get_set(db, name)
    type_ = uset.type
    if type_ is None:
        raise ValueError(f"set {db}.{name} has no type: load_delimited needs the schema")
    cols = file_columns(type_, fields, dates)
    delim = _delim_byte(delimiter)
    dev = client.device
    chunk_bytes = max(1, min(int(chunk_bytes), MAX_CHUNK))
    t0 = time.perf_counter()
    bounds = None
    line0 = 2 if header else 1
    if client.ctx.rank == 0:
        _, first, start = _first_lines(path, header)
        if trailing is None and first is not None:
            k = first.count(bytes([delim]))
            if k not in (len(cols), len(cols) - 1):
                raise ValueError(f"line {line0}: {k} delimiters for {len(cols)} columns: cannot tell whether fields "
                                 "are followed or separated by the delimiter")
            trailing = k == len(cols)
        bounds = chunk_bounds(path, start, chunk_bytes)
    nchunks = len(bounds) if bounds is not None else 0
    if client.ctx.distributed:
        nchunks = int(client.ctx.all_reduce_scalar(float(nchunks), "max"))
    stats: dict = {"host_cells": 0}
    rows = nbytes = 0
    for i in range(nchunks):
        b = None
        if client.ctx.rank == 0:
            lo, hi = bounds[i]
            nb = hi - lo
            seg = np.zeros(StringColumn._alloc_size(nb), dtype=np.uint8)     # padded once, for the string kernels
            seg[:nb] = np.memmap(path, dtype=np.uint8, mode="r")[lo:hi]
            host = torch.from_numpy(seg)
            if dev.type == "cuda":
                buf = host.pin_memory().to(dev, non_blocking=True)
                b = parse_delimited(buf, type_, delimiter=delimiter, trailing=bool(trailing), fields=fields,
                                    dates=dates, stats=stats, line0=line0, nbytes=nb)
                del buf
            else:
                b = parse_delimited(host[:nb], type_, delimiter=delimiter, trailing=bool(trailing), fields=fields,
                                    dates=dates, stats=stats, line0=line0)
            rows += b.n
            line0 += b.n
            nbytes += nb
        client.send_data(db, name, b, policy=policy)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return {"rows": rows, "bytes": nbytes, "seconds": time.perf_counter() - t0, "chunks": nchunks,
            "host_cells": stats["host_cells"]}


def import_set(client, db: str, name: str, path: str, fmt: str = "csv") -> dict:
    """The inverse of ``PDBClient.export_set(fmt="csv")``: a header line of field names, then one comma-separated line
    per object. The header's names map the file's columns onto the set's schema; an unknown or a missing name raises
    ValueError. Objects that write their own value strings are out of scope."""
    if fmt != "csv":
        raise ValueError(f"import_set reads fmt='csv' only, got {fmt!r}")
    names = None
    if client.ctx.rank == 0:
        head, _, _ = _first_lines(path, True)
        if head is None:
            raise ValueError(f"{path}: no header line")
        names = head.decode().split(",")
    return load_delimited(client, db, name, path, delimiter=",", trailing=False, header=True, fields=names)


__all__ = ["parse_plan", "parse_delimited", "load_delimited", "import_set", "file_columns", "in_fast_grammar",
           "chunk_bounds"]
