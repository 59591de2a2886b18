"""Delimited-text ingestion on the CPU (storage/textload.py): the host path, which is the oracle of the device path, and
the client methods. Hand-written expected values for each field kind, the fast grammar's edges with the exact number of
cells Python had to decode, line ends, column mapping, every kind of malformed input with its line number (with a header
and across chunk boundaries), and the export_set -> import_set round trip."""
import struct
import tempfile

import pytest
import torch

from netsdb_amd.client import PDBClient
from netsdb_amd.models.tpch import Date32
from netsdb_amd.objects.builtin import Employee
from netsdb_amd.objects.record import PDBObject, Tensor
from netsdb_amd.storage import textload as TL


class Day(int):
    pass


class TLRow(PDBObject):
    k: int
    x: float
    ok: bool
    d: Date32
    s: str


class TLPair(PDBObject):
    a: int
    b: float


class TLDays(PDBObject):
    k: int
    born: Day


class TLOne(PDBObject):
    s: str


class TLVec(PDBObject):
    k: int
    v: Tensor((4,))


def buf(b: bytes) -> torch.Tensor:
    return torch.frombuffer(bytearray(b), dtype=torch.uint8) if b else torch.empty(0, dtype=torch.uint8)


def bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", x))[0]


def parse(text: bytes, typ, **kw):
    st = {}
    b = TL.parse_delimited(buf(text), typ, stats=st, **kw)
    return b, st


# ------------------------------------------------------------------------------------------------ kinds
def test_every_kind_hand_checked():
    b, st = parse(b"1|2.50|1|1996-03-13|a b|\n-22|-0.125|false|2001-12-31||\n0|.5|True|0001-01-01|x|\n", TLRow)
    assert st == {"path": "host", "host_cells": 0, "rows": 3} and b.n == 3 and b.type is TLRow
    assert b["k"].dtype == torch.int64 and b["k"].tolist() == [1, -22, 0]
    assert b["x"].dtype == torch.float64 and b["x"].tolist() == [2.5, -0.125, 0.5]
    assert b["ok"].dtype == torch.bool and b["ok"].tolist() == [True, False, True]
    assert b["d"].dtype == torch.int32 and b["d"].tolist() == [19960313, 20011231, 10101]
    assert list(b["s"]) == ["a b", "", "x"]


def test_negative_zero_by_bit_pattern():
    b, st = parse(b"1|-0.00|\n2|0.00|\n3|-0|\n", TLPair)
    assert [bits(v) for v in b["b"].tolist()] == [bits(-0.0), bits(0.0), bits(-0.0)]
    assert bits(-0.0) != bits(0.0) and st["host_cells"] == 0


def test_fast_grammar_edges_and_host_cells():
    # 15 digits in all stay in the grammar, 16 leave it; so do 18 against 19 digits of an int
    b, st = parse(b"123456789012345678|123456789.012345|\n", TLPair)
    assert st["host_cells"] == 0 and b["a"].tolist() == [123456789012345678] and b["b"].tolist() == [123456789.012345]
    b, st = parse(b"1234567890123456789|1|\n", TLPair)
    assert st["host_cells"] == 1 and b["a"].tolist() == [1234567890123456789]
    b, st = parse(b"1|1234567890.123456|\n", TLPair)
    assert st["host_cells"] == 1 and b["b"].tolist() == [1234567890.123456]
    b, st = parse(b"-999999999999999999|-.000000000000001|\n", TLPair)
    assert st["host_cells"] == 0 and b["a"].tolist() == [-999999999999999999] and b["b"].tolist() == [-1e-15]
    # leading zeros count as digits
    b, st = parse(b"0000000000000000001|0000000000000001.5|\n", TLPair)
    assert st["host_cells"] == 2 and b["a"].tolist() == [1] and b["b"].tolist() == [1.5]


def test_cells_outside_the_grammar_go_to_python():
    b, st = parse(b"1|1e-05|\n 2 |nan|\n+3| 4.5 |\n4|inf|\n", TLPair)
    assert st["host_cells"] == 6
    assert b["a"].tolist() == [1, 2, 3, 4]
    x = b["b"].tolist()
    assert x[0] == 1e-05 and x[1] != x[1] and x[2] == 4.5 and x[3] == float("inf")
    b, st = parse(b"1|1| TRUE |2000-01-01|s|\n", TLRow)
    assert st["host_cells"] == 1 and b["ok"].tolist() == [True]


@pytest.mark.parametrize("text,line,field", [
    (b"1|2|\nx|3|\n", 2, "a"), (b"1|2|\n2|1.2.3|\n3||\n", 2, "b"), (b"9223372036854775808|1|\n", 1, "a"),
    (b"1|-|\n", 1, "b"), (b"|1|\n", 1, "a"),
])
def test_undecodable_cell_names_line_and_field(text, line, field):
    with pytest.raises(ValueError, match=rf"line {line}, field '{field}'"):
        parse(text, TLPair)
    with pytest.raises(ValueError, match=rf"line {line + 10}, field '{field}'"):
        parse(text, TLPair, line0=11)


def test_bool_outside_every_reading():
    with pytest.raises(ValueError, match="line 1, field 'ok'"):
        parse(b"1|1|yes|2000-01-01|s|\n", TLRow)


# ------------------------------------------------------------------------------------------------ rows
def test_crlf_and_missing_final_newline():
    b, _ = parse(b"1|2.5|\r\n3|4.5|\r\n5|6.5|", TLPair)
    assert b["a"].tolist() == [1, 3, 5] and b["b"].tolist() == [2.5, 4.5, 6.5]
    b, _ = parse(b"a,b\r\nc,d", TLTwoStr, delimiter=",", trailing=False)
    assert list(b["p"]) == ["a", "c"] and list(b["q"]) == ["b", "d"]


class TLTwoStr(PDBObject):
    p: str
    q: str


def test_trailing_both_ways_and_empty_strings():
    b, _ = parse(b"|\nx|\n", TLOne)
    assert list(b["s"]) == ["", "x"]
    b, _ = parse(b"\nx\n\n", TLOne, trailing=False)           # one column, separators only: an empty line is a row
    assert list(b["s"]) == ["", "x", ""]
    b, _ = parse(b",\n,x\n", TLTwoStr, delimiter=",", trailing=False)
    assert list(b["p"]) == ["", ""] and list(b["q"]) == ["", "x"]
    assert parse(b"", TLOne)[0].n == 0


def test_fields_with_a_skipped_column_and_another_order():
    b, st = parse(b"2.5,junk,7\n-1,,8\n", TLPair, delimiter=",", trailing=False, fields=["b", None, "a"])
    assert b["a"].tolist() == [7, 8] and b["b"].tolist() == [2.5, -1.0] and st["host_cells"] == 0
    assert b.names() == ["a", "b"]
    for bad in (["a"], ["a", "a", "b"], ["a", "b", "c"], ["a", None]):
        with pytest.raises(ValueError):
            parse(b"1,2\n", TLPair, delimiter=",", trailing=False, fields=bad)


def test_dates_names_other_int_subclasses():
    b, _ = parse(b"1|1999-12-31|\n", TLDays, dates=(Day,))
    assert b["born"].dtype == torch.int32 and b["born"].tolist() == [19991231]
    b, _ = parse(b"1|19991231|\n", TLDays)                     # not named: an int like any other
    assert b["born"].dtype == torch.int64 and b["born"].tolist() == [19991231]
    assert parse(b"1|1999-12-31|\n", TLDays, dates=("Day",))[0]["born"].tolist() == [19991231]


def test_schema_that_is_not_flat():
    with pytest.raises(TypeError, match="'v'"):
        parse(b"1|2|\n", TLVec)
    c = PDBClient(root=tempfile.mkdtemp(), device="cpu")
    c.create_database("db")
    c.create_set("db", "v", TLVec)
    with pytest.raises(TypeError):
        c.load_delimited("db", "v", "/nonexistent/file/is/never/opened")


def test_arguments():
    with pytest.raises(ValueError):
        TL.parse_delimited(buf(b"1|2|\n"), TLPair, path="device")        # a CPU tensor
    with pytest.raises(ValueError):
        TL.parse_delimited(buf(b"1|2|\n"), TLPair, path="torch")
    for d in ("\n", "\r", "||", ""):
        with pytest.raises(ValueError):
            TL.parse_delimited(buf(b"1|2|\n"), TLPair, delimiter=d)


# ------------------------------------------------------------------------------------------------ malformed input
@pytest.mark.parametrize("text,kw,line", [
    (b"1|2|\n3|4\n5|6|\n", {}, 2),                             # a delimiter short
    (b"1|2|\n3|4|5|\n", {}, 2),                                # one too many
    (b"1|2|\n3|4|x\n", {}, 2),                                 # bytes after the last delimiter
    (b"1|2|\n\n3|4|\n", {}, 2),                                # an empty line
    (b"1|2|\n3|4|\n5", {}, 3),                                 # a torn last line
    (b"1,2\n3,4,\n", dict(delimiter=",", trailing=False), 2),
    (b"1,2\n3\n4\n", dict(delimiter=",", trailing=False), 2),  # the lowest of two
    (b"1|2|\n3|4\n", dict(line0=100), 101),
])
def test_malformed_row_line_number(text, kw, line):
    with pytest.raises(ValueError, match=rf"line {line}: malformed row"):
        parse(text, TLPair, **kw)


@pytest.mark.parametrize("cell", [b"1996-3-13", b"19960313", b"1996-03-1x", b"", b"1996/03/13", b"1996-03-130", b" 1996-03-13"])
def test_bad_date_is_an_error(cell):
    with pytest.raises(ValueError, match="line 2: a date field"):
        parse(b"1|1|1|2000-01-01|s|\n1|1|1|" + cell + b"|s|\n", TLRow)


def test_lowest_bad_line_wins_over_kinds_and_cells():
    # line 2 has an undecodable cell, line 3 a bad date, line 4 is malformed: structure and dates are settled first
    with pytest.raises(ValueError, match="line 3: a date field"):
        parse(b"1|1|1|2000-01-01|s|\nx|1|1|2000-01-01|s|\n1|1|1|2000|s|\n1|1|\n", TLRow)


# ------------------------------------------------------------------------------------------------ files and the client
def _client(typ, name="t"):
    c = PDBClient(root=tempfile.mkdtemp(), device="cpu")
    c.create_database("db")
    c.create_set("db", name, typ)
    return c


def _write(text: bytes) -> str:
    f = tempfile.NamedTemporaryFile(suffix=".txt", delete=False)
    f.write(text)
    f.close()
    return f.name


def test_load_delimited_many_chunks():
    n = 500
    text = b"".join(b"%d|%d.%02d|\n" % (i, i * 7, i % 100) for i in range(n))
    c = _client(TLPair)
    st = c.load_delimited("db", "t", _write(text), chunk_bytes=64)
    assert st["rows"] == n and st["bytes"] == len(text) and st["chunks"] > 50 and st["host_cells"] == 0
    assert set(st) == {"rows", "bytes", "seconds", "chunks", "host_cells"}
    got = c.get_set("db", "t").all()
    assert got.columns["a"].tolist() == list(range(n))
    assert got.columns["b"].tolist() == [float("%d.%02d" % (i * 7, i % 100)) for i in range(n)]


def test_trailing_is_detected_from_the_first_data_line():
    for text, kw in ((b"1|2|\n3|4|\n", {}), (b"1|2\n3|4\n", {}), (b"a,b\n1,2\n3,4", dict(delimiter=",", header=True))):
        c = _client(TLPair)
        assert c.load_delimited("db", "t", _write(text), **kw)["rows"] == 2
        assert c.get_set("db", "t").all().columns["a"].tolist() == [1, 3]
    with pytest.raises(ValueError, match="line 1"):
        _client(TLPair).load_delimited("db", "t", _write(b"1|2|3|\n"))
    with pytest.raises(ValueError, match="line 2"):
        _client(TLPair).load_delimited("db", "t", _write(b"a|b\n1\n"), header=True)
    assert _client(TLPair).load_delimited("db", "t", _write(b""))["rows"] == 0


def test_line_numbers_with_a_header_and_across_chunks():
    rows = [b"%d|%d.5|\n" % (i, i) for i in range(40)]
    rows[30] = b"30|30.5\n"                                     # file line 32 with the header
    rows[35] = b"35\n"
    with pytest.raises(ValueError, match="line 32: malformed row"):
        _client(TLPair).load_delimited("db", "t", _write(b"a|b|\n" + b"".join(rows)), header=True, chunk_bytes=64)
    rows[30] = b"30|3x.5|\n"
    rows[35] = b"35|35.5|\n"
    with pytest.raises(ValueError, match="line 31, field 'b'"):
        _client(TLPair).load_delimited("db", "t", _write(b"".join(rows)), chunk_bytes=64)


def test_export_import_round_trip():
    emps = [Employee("ann", 45, "eng", 0.1 + 0.2), Employee("bob", 30, "ops", 1e-05), Employee("", -1, "r d", -0.0),
            Employee("dee", 10 ** 18, "x", 2.5)]
    c = _client(Employee, "emps")
    c.send_data("db", "emps", emps)
    path = tempfile.mktemp(suffix=".csv")
    assert c.export_set("db", "emps", path)
    c.create_set("db", "back", Employee)
    st = c.import_set("db", "back", path)
    # 0.30000000000000004 has 17 digits, 1e-05 an exponent, 10**18 has 19 digits: three cells for Python
    assert st["rows"] == 4 and st["host_cells"] == 3
    back = list(c.get_set_iterator("db", "back"))
    assert back == emps and [bits(o.salary) for o in back] == [bits(e.salary) for e in emps]


def test_import_set_checks_the_header():
    for head in (b"name,age,department\n", b"name,age,department,salary,extra\n", b"name,age,dept,salary\n"):
        c = _client(Employee, "e")
        with pytest.raises(ValueError):
            c.import_set("db", "e", _write(head + b"a,1,b,2.0\n"))
    with pytest.raises(ValueError):
        _client(Employee, "e").import_set("db", "e", _write(b"name,age,department,salary\n"), fmt="json")
    # the header decides the mapping, whatever the order
    c = _client(Employee, "e")
    assert c.import_set("db", "e", _write(b"salary,name,department,age\n2.5,a,d,7\n"))["rows"] == 1
    assert list(c.get_set_iterator("db", "e")) == [Employee("a", 7, "d", 2.5)]
