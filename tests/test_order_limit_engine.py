"""K.order_limit behind the engine: TopKComp (rows tied at the k-th score are kept lowest row first, integer scores
compare exactly, 1 rank == 2 ranks) and the ORDER BY ... LIMIT tails of TPC-H Q03 / Q02."""
import math
import os
import socket
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from netsdb_amd.client import PDBClient
from netsdb_amd.computations import ScanSet, TopKComp, WriteSet
from netsdb_amd.lambdas import make_lambda_from_member
from netsdb_amd.models import tpch
from netsdb_amd.objects import PDBObject
from netsdb_amd.objects.builtin import Employee


class Scored(PDBObject):
    name: str
    score: int


class TopSalary(TopKComp):
    def get_value_projection(self, e):
        return make_lambda_from_member(e, "salary")


class TopScore(TopKComp):
    def get_value_projection(self, e):
        return make_lambda_from_member(e, "score")


N_EMPS, K_TIES = 40, 13


def _tied_emps():
    """Salaries 1000 + 10 * (i % 4): ten rows share each salary. The top 13 are the ten rows of 1030 and then the three
    LOWEST rows of 1020. (A salary's rows are all even or all odd, so the record-wise round-robin placement of a
    2-rank run keeps each tie group on one rank in row order.)"""
    return [Employee(f"e{i:02d}", 30, "eng", 1000.0 + 10 * (i % 4)) for i in range(N_EMPS)]


def _expected_ties():
    return [f"e{i:02d}" for i in range(N_EMPS) if i % 4 == 3] + ["e02", "e06", "e10"]


def _top_names(c, comp, cls, out="top"):
    if c.storage.has_set("db", out):
        c.remove_set("db", out)
    c.create_set("db", out, cls)
    c.execute_computations(WriteSet("db", out).set_input(comp.set_input(ScanSet("db", "rows", cls))))
    return [o.name for o in c.get_set_iterator("db", out, gather=True)]


def _tie_client(root, device=None, ctx=None):
    kw = {"device": device} if device else {}
    if ctx is not None:
        kw["ctx"] = ctx
    c = PDBClient(root=root, page_size=1 << 12, **kw)
    c.create_database("db")
    c.create_set("db", "rows", Employee)
    c.send_data("db", "rows", _tied_emps() if ctx is None or ctx.rank == 0 else None)
    return c


def test_topk_ties_keep_lowest_rows_cpu(tmp_path):
    c = _tie_client(str(tmp_path))
    first = _top_names(c, TopSalary(K_TIES), Employee)
    assert sorted(first) == sorted(_expected_ties())
    assert _top_names(c, TopSalary(K_TIES), Employee) == first
    assert "device_order_limit" not in c.engine.pipeline_stats


def _int_scores(dev, tmp_path):
    big = 2 ** 53
    rows = [Scored(f"r{i}", big) for i in range(6)] + [Scored("r6", big + 1)] + [Scored(f"r{i}", i) for i in range(7, 30)]
    kw = {"device": dev} if dev != "cpu" else {}
    c = PDBClient(root=str(tmp_path), page_size=1 << 12, **kw)
    c.create_database("db")
    c.create_set("db", "rows", Scored)
    c.send_data("db", "rows", rows)
    assert _top_names(c, TopScore(1), Scored) == ["r6"]
    assert sorted(_top_names(c, TopScore(3), Scored)) == ["r0", "r1", "r6"]
    return c


def test_topk_integer_scores_compare_exactly_cpu(tmp_path):
    _int_scores("cpu", tmp_path)


# ------------------------------------------------------------------------------------------------ 2 ranks (gloo)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, ws, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(ws),
                      LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        from netsdb_amd.parallel.comm import ClusterContext

        ctx = ClusterContext(rank, ws, torch.device("cpu"), "gloo")
        c = _tie_client(tempfile.mkdtemp(), ctx=ctx)
        res = {"names": _top_names(c, TopSalary(K_TIES), Employee), "local": c.get_set("db", "rows").num_records()}
        torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_topk_two_ranks_keep_the_rows_of_one_rank(tmp_path):
    one = _top_names(_tie_client(str(tmp_path)), TopSalary(K_TIES), Employee)
    out = tempfile.mkdtemp()
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    res = [torch.load(os.path.join(out, f"r{r}.pt"), weights_only=False) for r in range(2)]
    assert all(0 < r["local"] < N_EMPS for r in res) and sum(r["local"] for r in res) == N_EMPS
    for r in res:
        assert sorted(r["names"]) == sorted(one) == sorted(_expected_ties())


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_topk_ties_keep_lowest_rows_gpu(tmp_path):
    c = _tie_client(str(tmp_path), device="cuda:0")
    first = _top_names(c, TopSalary(K_TIES), Employee)
    assert sorted(first) == sorted(_expected_ties())
    assert _top_names(c, TopSalary(K_TIES), Employee) == first
    assert c.engine.pipeline_stats["device_order_limit"] >= 1


@pytest.mark.gpu
def test_topk_integer_scores_compare_exactly_gpu(tmp_path):
    c = _int_scores("cuda:0", tmp_path)
    assert c.engine.pipeline_stats["device_order_limit"] >= 1


def _close_rows(got, ref, keys):
    assert len(got) == len(ref), (got[:3], ref[:3])
    for g, r in zip(got, ref):
        for k in keys:
            if isinstance(r[k], float):
                assert math.isclose(g[k], r[k], rel_tol=1e-9, abs_tol=1e-6), (k, g, r)
            else:
                assert g[k] == r[k], (k, g, r)


@pytest.mark.gpu
def test_tpch_q03_q02_order_by_limit_gpu(tmp_path):
    t = tpch.generate(0.004, seed=7)
    c = PDBClient(root=str(tmp_path), device="cuda:0")
    tpch.load(c, "tpch", t, device="cuda:0")
    st = c.engine.pipeline_stats
    ref = tpch.reference("q03", t)
    assert ref
    _close_rows(tpch.q03(c, "tpch"), ref, list(ref[0]))
    n3 = st.get("device_order_limit", 0)
    assert n3 >= 1
    size = int(t["part"]["p_size"][5])
    suffix = t["part"]["p_type"][5].split()[-1]
    for region in tpch.REGIONS:
        ref = tpch.reference("q02", t, size=size, type_suffix=suffix, region=region)
        if ref:
            break
    assert ref
    # k below the number of qualifying rows, so the k-th balance is looked up on the device
    k = max(1, len(ref) // 2)
    ref = tpch.reference("q02", t, size=size, type_suffix=suffix, region=region)[:k]
    got = tpch.q02(c, "tpch", size=size, type_suffix=suffix, region=region, k=k)
    _close_rows(got, ref, ["s_acctbal", "s_name", "n_name", "p_partkey", "p_mfgr"])
    assert st.get("device_order_limit", 0) > n3
