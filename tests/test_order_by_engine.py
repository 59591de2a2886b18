"""K.order_by behind the engine: a TopKComp whose k is above K.ORDER_LIMIT_MAX_K keeps the k best rows in order (rows
tied at the k-th score lowest row first) through the full ORDER BY with a limit instead of order_limit."""
import pytest
import torch

from netsdb_amd.client import PDBClient
from netsdb_amd.computations import ScanSet, TopKComp, WriteSet
from netsdb_amd.execution import kernels as K
from netsdb_amd.lambdas import make_lambda_from_member
from netsdb_amd.objects import PDBObject

N_ROWS, K_TOP = 5000, 3000


class Scored(PDBObject):
    name: str
    score: int


class TopScore(TopKComp):
    def get_value_projection(self, e):
        return make_lambda_from_member(e, "score")


def _scores():
    """700 distinct scores over 5000 rows: about seven rows tie on each, and the 3000-th row is inside a tie group."""
    g = torch.Generator().manual_seed(21)
    return torch.randint(0, 700, (N_ROWS,), generator=g).tolist()


def _expected(scores):
    rows = sorted(range(N_ROWS), key=lambda i: (-scores[i], i))[:K_TOP]
    return [f"r{i:04d}" for i in rows]


def _run(root, device=None):
    scores = _scores()
    kw = {"device": device} if device else {}
    c = PDBClient(root=root, page_size=1 << 16, **kw)
    c.create_database("db")
    c.create_set("db", "rows", Scored)
    c.send_data("db", "rows", [Scored(f"r{i:04d}", s) for i, s in enumerate(scores)])
    c.create_set("db", "top", Scored)
    c.execute_computations(WriteSet("db", "top").set_input(TopScore(K_TOP).set_input(ScanSet("db", "rows", Scored))))
    got = [o.name for o in c.get_set_iterator("db", "top", gather=True)]
    assert K_TOP > K.ORDER_LIMIT_MAX_K
    assert got == _expected(scores)
    return c


def test_topk_above_the_order_limit_cap_cpu(tmp_path):
    c = _run(str(tmp_path))
    assert "device_order_by" not in c.engine.pipeline_stats
    assert "device_order_limit" not in c.engine.pipeline_stats


@pytest.mark.gpu
def test_topk_above_the_order_limit_cap_gpu(tmp_path):
    c = _run(str(tmp_path), device="cuda:0")
    # the score column reaches the engine as int64 or float64: the same plan either way at this size
    plan = K.order_by_plan([torch.int64], N_ROWS, True)
    assert plan["path"] in ("radix", "torch")
    assert plan["path"] == K.order_by_plan([torch.float64], N_ROWS, True)["path"]
    if plan["path"] == "radix":
        assert c.engine.pipeline_stats["device_order_by"] >= 1
    else:
        assert "device_order_by" not in c.engine.pipeline_stats
    # the arm the default dispatch leaves out gives the same rows
    sc = torch.tensor(_scores(), device="cuda:0")
    dev = K.order_by([sc], True, limit=K_TOP, path="device")
    assert torch.equal(dev, K.order_by([sc], True, limit=K_TOP, path="torch"))
