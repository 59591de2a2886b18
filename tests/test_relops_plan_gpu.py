"""What hash_aggregate and join_build allocate is what their plans say (hash_aggregate_plan / join_build_plan, i.e.
csrc/kernels/relops_plan.h) and what the commit before the plan allocated: tests/golden/relops_plan_parent.json holds
the status words and tensor sizes of one run of that commit over these same inputs ("gpu"). Each group-by case first
asserts the path it is about."""
import json
import os

import numpy as np
import pytest
import torch

from netsdb_amd import _ext

DEV = "cuda:0"
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relops_plan_parent.json")) as _f:
    GOLD = json.load(_f)["gpu"]


def _keys(kind, n):
    g = np.random.default_rng(12345)
    if kind == "low":                                   # 8 keys
        return (np.arange(n, dtype=np.int64) % 8) * 1000003 + 7
    if kind == "mid":                                   # 3000 keys, uniform
        return g.integers(0, 3000, n).astype(np.int64) * 7919 + 1
    return g.permutation(n).astype(np.int64) * 3 + 1    # all distinct


GROUPBY = [("low", 4096, 2, False), ("mid", 65536, 2, False)] + [("part", 65536, F, inv) for F in (0, 2, 16)
                                                                  for inv in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,F,inv", GROUPBY, ids=[f"{k}-n{n}-F{F}-inv{int(i)}" for k, n, F, i in GROUPBY])
def test_hash_aggregate_allocates_its_plan(kind, n, F, inv):
    h = _ext.hip()
    k = torch.from_numpy(_keys(kind, n)).to(DEV)
    v = torch.ones((n, F), dtype=torch.float64, device=DEV) if F else None
    plan = h.hash_aggregate_plan(n, F, 0, want_inv=inv, want_first=True)
    assert plan["rc"] == 0
    groups, path, ok, est, scratch = h.hash_aggregate(k, v, "sum", inv, 0, True)[5].tolist()
    assert ok == 1
    mid_parts = -(-est // (plan["lcap_mid"] // 2))     # MID key partitions the estimate asks for (at most 3 run)
    if kind == "low":
        assert path == 0 and est <= plan["low_thr"] and groups == 8
    elif kind == "mid":
        assert path == 0 and est > plan["low_thr"] and mid_parts <= 3 and groups == 3000
    else:
        assert path == 1 and est > plan["low_thr"] and mid_parts > 3 and groups == n
    want = GOLD["groupby"][f"{kind}-n{n}-F{F}-inv{int(inv)}"]
    assert [groups, path, ok, est] == [want[f] for f in ("groups", "path", "ok", "est")]
    assert scratch == plan["scratch_part" if path else "scratch_low"] == want["scratch_bytes"]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1000, 2 ** 18, 2 ** 18 + 1, 2 ** 20 + 1, 2 ** 21 + 1])
def test_join_build_allocates_its_plan(n):
    """Both load-factor steps, whole-table against region tables, the one- and two-level partition, the filter on
    (separate pass and folded into the region pass) and off."""
    h = _ext.hip()
    k = torch.arange(n, dtype=torch.int64, device=DEV) * 2654435761 + 11
    plan = h.join_build_plan(n)
    tab, perm, bloom, stat = h.join_build(k)
    assert stat.numel() == 0 or int(stat[0]) == 0                       # built at the planned size, not rebuilt larger
    got = {"cap": tab.shape[0] - 1, "bloom": bloom.numel(), "stat": stat.numel(), "fail": 0}
    assert got == {"cap": plan["cap"], "bloom": plan["bloom_words"], "stat": plan["stat_words"], "fail": 0}
    assert got == GOLD["join"][str(n)]
    assert plan["rc"] == 0 and perm.numel() == n
    shape = (plan["load"], plan["regions"], plan["part"], plan["fold"], plan["sh"] > 0)
    assert shape == {1000: (8, 0, 0, 0, False), 2 ** 18: (8, 0, 0, 0, False), 2 ** 18 + 1: (4, 0, 0, 0, False),
                     2 ** 20 + 1: (4, 1, 1, 1, False), 2 ** 21 + 1: (4, 1, 1, 0, True)}[n]
