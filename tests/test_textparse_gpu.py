"""The delimited-text kernels (csrc/kernels/textparse.hip) against the plain host path of storage/textload.py on the
same bytes, and against the whole-column torch parser of models/tpch_tbl.py where that one applies (the TPC-H tables).
Numbers compare by bit pattern, strings by bytes, and stats["host_cells"] against a count the test takes itself with
regular expressions over the cells. The shapes come from the plan (tile T, scan_step): buffers of one row, T and T + 1
bytes, newlines on either side of a tile boundary, a row and a number across it, a row longer than two tiles, one tile
more than a scan step, unpadded and unaligned buffers. Malformed text is reported through the status word; no case
reads out of range."""
import os
import re
import tempfile

import numpy as np
import pytest
import torch

from netsdb_amd.client import PDBClient
from netsdb_amd.models import tpch, tpch_gen, tpch_tbl
from netsdb_amd.models.tpch import Date32
from netsdb_amd.objects.record import PDBObject
from netsdb_amd.objects.strings import StringColumn
from netsdb_amd.storage import textload as TL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class GRow(PDBObject):
    k: int
    x: float
    ok: bool
    d: Date32
    s: str


class GNum(PDBObject):
    a: int
    b: float


class GStr(PDBObject):
    s: str


G64 = type("G64", (PDBObject,), {"__annotations__": {f"c{i:02d}": (int, float, str, bool)[i % 4] for i in range(64)}})

_FAST = {int: re.compile(rb"-?[0-9]{1,18}"), bool: re.compile(rb"0|1|true|false|True|False")}
_FLOAT = re.compile(rb"-?([0-9]*)(\.[0-9]*)?")


def expected_host_cells(text: bytes, typ, delimiter=b"|", fields=None):
    """Cells of int / float / bool columns outside the fast grammar, counted here with regular expressions."""
    schema = typ.fields()
    names = list(schema) if fields is None else fields
    n = 0
    for ln in text.split(b"\n"):
        if ln == b"" and len(names) > 1:
            continue
        ln = ln[:-1] if ln.endswith(b"\r") else ln
        for name, cell in zip(names, ln.split(delimiter)):
            ft = schema.get(name)
            if ft is float:
                m = _FLOAT.fullmatch(cell)
                n += not (m and 1 <= len(m.group(1)) + max(0, len(m.group(2) or b"") - 1) <= 15)
            elif ft in _FAST:
                n += _FAST[ft].fullmatch(cell) is None
    return n


def dev_buf(text: bytes) -> torch.Tensor:
    """An unpadded device tensor of exactly the text's bytes."""
    return torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(DEV)


def col_bytes(c):
    if isinstance(c, StringColumn):
        c = c.tolist()
    return [x.encode() if isinstance(x, str) else bytes(x) for x in c]


def assert_same(a, b):
    assert a.n == b.n and a.names() == b.names() and a.type is b.type
    for name in a.names():
        x, y = a[name], b[name]
        if isinstance(x, torch.Tensor):
            assert isinstance(y, torch.Tensor) and x.dtype == y.dtype, name
            x, y = x.cpu().contiguous(), y.cpu().contiguous()
            if x.dtype == torch.float64:
                x, y = x.view(torch.int64), y.view(torch.int64)          # bit patterns: -0.0 is not +0.0
            assert torch.equal(x, y), name
        else:
            assert col_bytes(x) == col_bytes(y), name


def check(text: bytes, typ, buf=None, **kw):
    """device == host on the same bytes, with the expected number of host-decoded cells; returns the device batch."""
    buf = dev_buf(text) if buf is None else buf
    sd, sh = {}, {}
    got = TL.parse_delimited(buf, typ, path="device", stats=sd, **kw)
    want = TL.parse_delimited(torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()), typ, path="host", stats=sh, **kw)
    assert_same(got, want)
    d = kw.get("delimiter", "|").encode()
    cells = expected_host_cells(text, typ, d, kw.get("fields"))
    assert sd["host_cells"] == cells == sh["host_cells"] and sd["path"] == "device" and sd["rows"] == want.n
    return got


def grow(i: int, pad: int = 0) -> bytes:
    return b"%d|%d.%02d|%d|19%02d-%02d-%02d|%s|\n" % (i * 37 - 500, i * 3 - 40, i % 100, i & 1, i % 100, 1 + i % 12,
                                                      1 + i % 28, b"s%d" % i + b"." * pad)


def text_of_length(total: int, first_pad: int = 0) -> bytes:
    """GRow lines of exactly `total` bytes: the first row's string is padded by first_pad, the last row's to fit."""
    rows = [grow(0, first_pad)]
    size, i, last = len(rows[0]), 1, (0, first_pad)
    while total - size >= 160:
        rows.append(grow(i))
        size, i, last = size + len(rows[-1]), i + 1, (i, 0)
    rest = total - size
    if rest >= len(grow(i)):
        rows.append(grow(i, rest - len(grow(i))))
    elif rest:
        rows[-1] = grow(last[0], last[1] + rest)
    out = b"".join(rows)
    assert len(out) == total
    return out


@pytest.fixture(scope="module")
def plan():
    p = TL.parse_plan(1 << 20, 5)
    assert p["rc"] == 0
    return p["tile"], p["scan_step"]


# ------------------------------------------------------------------------------------------------ sizes and boundaries
def test_one_row():
    b = check(b"7|-2.5|true|2024-02-29|x|\n", GRow)
    assert b["k"].tolist() == [7] and b["x"].tolist() == [-2.5] and b["d"].tolist() == [20240229]
    check(b"7|-2.5|true|2024-02-29|x|", GRow)
    check(b"\n", GStr, trailing=False)


def test_exactly_one_tile_and_one_byte_more(plan):
    T, _ = plan
    for total in (T, T + 1):
        assert TL.parse_plan(total, 5)["tiles"] == (1 if total == T else 2)
        check(text_of_length(total), GRow)


def test_newline_on_either_side_of_a_tile_boundary(plan):
    T, _ = plan
    base = len(grow(0))
    for end in (T, T + 1):                       # the first row's newline is the tile's last byte / the next one's first
        text = text_of_length(2 * T + 333, first_pad=end - base)
        assert text[end - 1] == 10 and text.index(b"\n") == end - 1
        check(text, GRow)


def test_row_and_number_across_a_tile_boundary(plan):
    T, _ = plan
    base = len(grow(0))
    for cut in (1, 3, 9):                        # the second row starts `cut` bytes before the boundary
        text = text_of_length(3 * T + 17, first_pad=T - cut - base)
        rows = text.split(b"\n")
        assert len(rows[0]) + 1 == T - cut and rows[1].startswith(b"-463|-37.01|")      # a number on the boundary
        b = check(text, GRow)
        assert b["k"][1].item() == -463 and b["x"][1].item() == -37.01


def test_one_row_longer_than_two_tiles(plan):
    T, _ = plan
    text = grow(1) + grow(2, 2 * T + 100) + grow(3)
    b = check(text, GRow)
    assert len(col_bytes(b["s"])[1]) == 2 * T + 102


def test_one_tile_more_than_a_scan_step(plan):
    T, step = plan
    total = step * T + 5
    assert TL.parse_plan(total, 5)["tiles"] == step + 1
    row = grow(12345, 180)
    n = total // len(row)
    text = row * (n - 1)
    text += grow(7, total - len(text) - len(grow(7)))
    assert len(text) == total
    b = check(text, GRow)
    assert b.n == n


def test_unpadded_tensor_ending_on_the_allocation(plan):
    T, _ = plan
    for total in (T + 7, 61, 2 * T - 1):
        text = text_of_length(total)
        buf = dev_buf(text)
        assert buf.numel() == total and buf.untyped_storage().nbytes() == total
        check(text, GRow, buf=buf)
        check(text[:-1], GRow, buf=dev_buf(text[:-1]))        # the last row without its newline


def test_view_at_an_unaligned_storage_offset():
    text = text_of_length(5000)
    for off in (1, 3, 8, 15):
        big = dev_buf(b"\n" * off + text)
        view = big[off:]
        assert view.data_ptr() % 16 == off
        check(text, GRow, buf=view)


def test_nbytes_of_a_longer_allocation():
    text = text_of_length(777)
    buf = dev_buf(text + b"9|9|\n" * 10)                       # bytes past the payload are never rows
    got = TL.parse_delimited(buf, GRow, path="device", nbytes=len(text))
    assert_same(got, TL.parse_delimited(dev_buf(text).cpu(), GRow, path="host"))


# ------------------------------------------------------------------------------------------------ values
def test_all_kinds_with_edge_values():
    rows = [
        b"-999999999999999999|-0.00|0|0001-01-01||",
        b"999999999999999999|.123456789012345|1|9999-12-31|\xc3\xa9t\xc3\xa9|",
        b"-0|-123456789012345|true|2000-02-29|a b|",
        b"000000000000000001|99999.9999999999|false|1970-01-01|-|",
        b"5|5.|True|1999-09-09|.|",
        b"-5|-.5|False|1999-09-09|5|",
        b"0|000000000000.000|1|1999-09-09|0|",
    ]
    text = b"\n".join(rows) + b"\n"
    b = check(text, GRow)
    assert b["k"].tolist()[:2] == [-999999999999999999, 999999999999999999]
    x = b["x"].cpu()
    assert x.view(torch.int64)[0].item() == torch.tensor([-0.0], dtype=torch.float64).view(torch.int64).item()
    assert x.tolist()[1:3] == [0.123456789012345, -123456789012345.0]


def test_cells_outside_the_grammar_are_decoded_by_python():
    rows = [b"1|1e-05|1|2000-01-01|a|", b" 2 |nan|0|2000-01-01|b|", b"1234567890123456789|1234567890.123456| true|2000-01-01|c|",
            b"+4|-inf|FALSE|2000-01-01|d|", b"5|0.30000000000000004|1|2000-01-01|e|", b"6|6|1|2000-01-01|f|"]
    text = b"\n".join(rows * 40) + b"\n"
    sd = {}
    TL.parse_delimited(dev_buf(text), GRow, path="device", stats=sd)
    assert sd["host_cells"] == 10 * 40
    check(text, GRow)
    for bad, name in ((b"7|x|1|2000-01-01|g|\n", "x"), (b"9223372036854775808|1|1|2000-01-01|g|\n", "k"),
                      (b"7|7|maybe|2000-01-01|g|\n", "ok")):
        for path in ("device", "host"):
            with pytest.raises(ValueError, match=rf"line 241, field '{name}'"):
                TL.parse_delimited(dev_buf(text + bad), GRow, path=path)


def test_crlf_final_newline_and_trailing_both_ways():
    check(b"1|2.5|\r\n-3|4.25|\r\n5|6|", GNum)
    check(b"1|2.5\r\n-3|4.25\r\n5|6", GNum, trailing=False)
    check(b"1,2.5\n-3,4.25\n", GNum, delimiter=",", trailing=False)
    check(b"a\n\nb\r\n\r\n", GStr, trailing=False)
    check(b"a\tb\t\n", type("GTab", (PDBObject,), {"__annotations__": {"p": str, "q": str}}), delimiter="\t")


def test_sixty_four_fields_and_a_skipped_column():
    def row(i):
        return b"|".join((b"%d" % (i - 3), b"%d.%d" % (i, i % 10), b"t%d" % i, b"%d" % (i & 1))[j % 4] for j in range(64))

    text = b"".join(row(i) + b"|\n" for i in range(300))
    b = check(text, G64)
    assert b["c00"].tolist()[:4] == [-3, -2, -1, 0] and b.n == 300
    check(b"".join(row(i) + b"\n" for i in range(300)), G64, trailing=False)
    check(b"2.5,junk,7\n-1,,8\n", GNum, delimiter=",", trailing=False, fields=["b", None, "a"])
    with pytest.raises(ValueError):
        TL.parse_delimited(dev_buf(b"1|" * 65 + b"\n"), G64, fields=list(G64.fields()) + [None])


# ------------------------------------------------------------------------------------------------ errors
def test_lowest_of_two_malformed_rows_in_different_tiles(plan):
    T, _ = plan
    rows = [grow(i) for i in range(2000)]
    assert sum(map(len, rows[:600])) > T and sum(map(len, rows[600:1500])) > T
    rows[1500] = b"1|2|\n"
    rows[600] = rows[600].replace(b"|\n", b"\n")
    for path in ("device", "host"):
        with pytest.raises(ValueError, match="line 601: malformed row"):
            TL.parse_delimited(dev_buf(b"".join(rows)), GRow, path=path)
        with pytest.raises(ValueError, match="line 1601: malformed row"):
            TL.parse_delimited(dev_buf(b"".join(rows)), GRow, path=path, line0=1001)
    for bad in (b"\n", b"1|2|3|2000-01-01|s|x\n", b"1|2|3|2000-01-01|s||\n", b"1|2|3|2000-01-01\n"):
        for path in ("device", "host"):
            with pytest.raises(ValueError, match="line 3: malformed row"):
                TL.parse_delimited(dev_buf(grow(1) + grow(2) + bad + grow(3)), GRow, path=path)
    with pytest.raises(ValueError, match="line 2: malformed row"):
        TL.parse_delimited(dev_buf(grow(1) + b"1|2|3"), GRow, path="device")


def test_bad_date():
    for cell in (b"1996-3-13", b"19960313", b"1996-03-1x", b"", b"1996/03/13", b"1996-03-130"):
        text = grow(1) + b"1|1|1|" + cell + b"|s|\n" + grow(2)
        for path in ("device", "host"):
            with pytest.raises(ValueError, match="line 2: a date field"):
                TL.parse_delimited(dev_buf(text), GRow, path=path)
    # a malformed row on a lower line wins over the date
    with pytest.raises(ValueError, match="line 1: malformed row"):
        TL.parse_delimited(dev_buf(b"1|2\n1|1|1|x|s|\n"), GRow, path="device")


# ------------------------------------------------------------------------------------------------ TPC-H and the client
@pytest.fixture(scope="module")
def lineitem_text():
    t = tpch_gen.generate_fast(0.033, seed=5)
    d = tempfile.mkdtemp()
    p = tpch_tbl.write_tbl(t, d, only=["lineitem", "orders"])
    return {k: open(v, "rb").read() for k, v in p.items()}


def test_lineitem_against_host_and_torch(lineitem_text):
    text = lineitem_text["lineitem"]
    typ = tpch.TABLES["lineitem"]
    assert 150_000 < text.count(b"\n") < 260_000
    buf = dev_buf(text)
    sd = {}
    got = TL.parse_delimited(buf, typ, path="device", stats=sd)
    assert sd["host_cells"] == 0                                # dbgen's text is wholly inside the fast grammar
    assert_same(got, tpch_tbl.parse_tbl(buf, "lineitem", path="torch"))
    assert_same(got, tpch_tbl.parse_tbl(buf, "lineitem", path="device"))
    # the host oracle reads cell by cell in Python (about 20 us a row): it takes a line-aligned eighth of the rows,
    # compared with the kernels on those same bytes; the whole buffer is held to the torch parser above
    cut = text.index(b"\n", len(text) // 8) + 1
    head = dev_buf(text[:cut])
    assert_same(TL.parse_delimited(head, typ, path="device"), TL.parse_delimited(head.cpu(), typ, path="host"))


def test_orders_against_torch(lineitem_text):
    buf = dev_buf(lineitem_text["orders"])
    assert_same(tpch_tbl.parse_tbl(buf, "orders", path="device"), tpch_tbl.parse_tbl(buf, "orders", path="torch"))


def test_load_delimited_into_a_set_in_small_chunks():
    text = b"".join(grow(i, i % 50) for i in range(3000))
    path = os.path.join(tempfile.mkdtemp(), "rows.tbl")
    with open(path, "wb") as f:
        f.write(text)
    c = PDBClient(root=tempfile.mkdtemp(), device=DEV)
    c.create_database("db")
    c.create_set("db", "rows", GRow)
    st = c.load_delimited("db", "rows", path, chunk_bytes=4096)
    assert st["rows"] == 3000 and st["bytes"] == len(text) and st["chunks"] > 20 and st["host_cells"] == 0
    got = c.get_set("db", "rows").all()
    want = TL.parse_delimited(torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()), GRow, path="host")
    for name in ("k", "x", "ok", "d"):
        assert torch.equal(got.columns[name].cpu(), want[name]), name
    assert col_bytes(got.columns["s"]) == col_bytes(want["s"])
