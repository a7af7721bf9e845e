"""The queueing rules of branch.GradBranch on CPU tensors, its fork replaced by a stub that logs enter / exit and carries a fresh
completion token: when a deferred launch runs, what a flush returns, how parked work goes out (one product each or ONE grouped launch,
the tile threshold, the table caches and their keys, the LayerNorm finish table) and what begin() / drop() reset -- never the tables."""
import os
import subprocess
import sys

import pytest
import torch

from aozora_sdxl_training_amd import ops
from aozora_sdxl_training_amd.activations import ActivationStore
from aozora_sdxl_training_amd.branch import GradBranch

BF16, F32 = torch.bfloat16, torch.float32


class _Fork:
    done = None

    def __init__(self, log):
        self.log = log

    def __enter__(self):
        self.log.append("enter")
        return self

    def __exit__(self, *a):
        self.done = object()
        self.log.append("exit")
        return False


class _Branch(GradBranch):
    def fork(self):
        self.forks.append(_Fork(self.log))
        return self.forks[-1]


@pytest.fixture
def make(monkeypatch):
    """make(concurrent, **policy) -> a branch on "cpu" without streams; branch.log takes "enter" / "exit" of every fork and one entry per
    ops launch: ("gemm", dy, x, dW, keywords), ("grouped", record), ("ln", table, njobs, nblocks).  ops.tn_group_table (it refuses CPU
    tensors) returns a tuple around a new record [jobs, device] per call, so identity shows a cache hit; branch.tables holds the records."""
    from aozora_sdxl_training_amd.unet import ExecPolicy
    log, tables = [], []
    monkeypatch.setattr(ops, "gemm", lambda a, b, out, **kw: log.append(("gemm", a, b, out, kw)))
    monkeypatch.setattr(ops, "gemm_tn_grouped", lambda rec: log.append(("grouped", rec)))
    monkeypatch.setattr(ops, "ln_param_finish_multi", lambda t, n, blocks: log.append(("ln", t, n, blocks)))

    def table(jobs, device):
        tables.append([list(jobs), device])
        return (tables[-1],)
    monkeypatch.setattr(ops, "tn_group_table", table)

    def make(concurrent, **policy):
        b = _Branch(ExecPolicy(**policy), ActivationStore("cpu"), [], "cpu")
        b.concurrent, b.log, b.forks, b.tables = concurrent, log, [], tables
        return b
    return make


def _job(K, N, M, bias=True):
    """(dY [K][N], X [K][M], dW [N][M], bias gradient [N] or None): ceil(N / 128) * ceil(M / 128) tiles."""
    return (torch.zeros(K, N, dtype=BF16), torch.zeros(K, M, dtype=BF16), torch.zeros(N, M, dtype=BF16),
            torch.zeros(N, dtype=BF16) if bias else None)


def _is_product_of(entry, job):
    kind, dy, x, dW, kw = entry
    return (kind == "gemm" and dy is job[0] and x is job[1] and dW is job[2] and set(kw) == {"trans_a", "trans_b", "accumulate", "split_k", "bias_grad"}
            and (kw["trans_a"], kw["trans_b"], kw["accumulate"], kw["split_k"]) == (True, False, True, 0) and kw["bias_grad"] is job[3])


def test_the_module_stands_without_the_executor():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, types, aozora_sdxl_training_amd.branch as b; "
            "assert 'aozora_sdxl_training_amd.unet' not in sys.modules; "
            "b.GradBranch(types.SimpleNamespace(), None, [], 'cpu')")
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0


def test_a_serial_branch_runs_at_once_and_never_forks(make):
    b = make(False, side_batch=3)
    ran = []
    b.defer(lambda: ran.append(1))
    assert ran == [1] and b.q == []
    b.defer(lambda: ran.append(2))
    assert ran == [1, 2] and b.q == []
    assert b.flush() is None and b.forks == [] and b.log == [] and not b.used


def test_a_batch_goes_out_in_order_inside_one_fork_and_an_empty_flush_returns_the_last_event(make):
    b = make(True, side_batch=3)
    b.defer(lambda: b.log.append(1))
    b.defer(lambda: b.log.append(2))
    assert b.log == [] and len(b.q) == 2 and b.forks == []
    b.defer(lambda: b.log.append(3))
    assert b.log == ["enter", 1, 2, 3, "exit"] and b.q == [] and len(b.forks) == 1
    first = b.forks[0].done
    assert first is not None and b.done is first
    assert b.flush() is first and b.flush() is first and len(b.forks) == 1        # nothing queued: the previous flush's event
    b.defer(lambda: b.log.append(4))
    second = b.flush()
    assert second is not first and second is b.forks[1].done and b.done is second and len(b.forks) == 2
    assert b.log == ["enter", 1, 2, 3, "exit", "enter", 4, "exit"]
    assert b.flush() is second


def test_below_the_threshold_every_parked_product_goes_out_on_its_own_in_park_order(make):
    """(The threshold is one the 13 tiles never reach.  With tn_group = 0 linear() parks nothing, and the rule `tiles >= tn_group`
    would call anything parked a full group: there is no per-product case to check at 0.)"""
    b = make(False, tn_group=100)
    jobs = [_job(64, 256, 128), _job(32, 128, 128, bias=False), _job(64, 384, 256), _job(64, 256, 256)]
    for j in jobs:
        b.park_tn(j)
    assert b.log == [] and b.tn_jobs == jobs
    b.finish_tn()
    assert len(b.log) == 4 and all(_is_product_of(e, j) for e, j in zip(b.log, jobs))
    assert b.tn_jobs == [] and b.tables == [] and b.tn_tables == {}
    b.finish_tn()                 # nothing parked: nothing goes out
    assert len(b.log) == 4


def test_parked_products_go_out_as_one_grouped_launch_when_their_tiles_reach_the_threshold(make):
    b = make(False, tn_group=4)
    j2, j1a, j1b = _job(64, 256, 128), _job(64, 128, 128), _job(64, 100, 70, bias=False)       # 2, 1 and 1 tiles
    b.park_tn(j2)
    assert b.log == [] and b.tn_jobs == [j2]                 # 2 tiles
    b.park_tn(j1a)
    assert b.log == [] and b.tn_jobs == [j2, j1a]            # 3 tiles
    b.park_tn(j1b)                                           # 4 tiles: out
    assert b.tn_jobs == [] and len(b.log) == 1 and len(b.tables) == 1
    tab = b.tables[0]
    assert b.log[0][0] == "grouped" and b.log[0][1] is tab and tab == [[j2, j1a, j1b], torch.device("cpu")]
    assert [t[0] for t in b.tn_tables.values()] == [tab] and list(b.tn_tables.values())[0][0] is tab
    for j in (j2, j1a, j1b):                                 # the same operand set again: the same table object
        b.park_tn(j)
    assert len(b.log) == 2 and b.log[1][1] is tab and len(b.tables) == 1 and len(b.tn_tables) == 1
    k2 = _job(64, 256, 128)                                  # other addresses: another table
    b.park_tn(k2); b.park_tn(j2)
    assert len(b.log) == 3 and b.log[2][1] is b.tables[1] and b.tables[1][0] == [k2, j2] and len(b.tn_tables) == 2
    # a block that ends below the threshold: one product each
    b.park_tn(j2); b.park_tn(j1a)
    b.finish_tn()
    assert len(b.log) == 5 and _is_product_of(b.log[3], j2) and _is_product_of(b.log[4], j1a) and len(b.tables) == 2


def test_context_projection_gradients_go_out_alone_or_grouped_under_their_own_table_key(make):
    b = make(False, tn_group=4)
    j, k = _job(308, 256, 128), _job(308, 256, 128)
    b.park_xkv(j)
    b.finish_xkv()
    assert len(b.log) == 1 and _is_product_of(b.log[0], j) and b.tables == [] and b.xkv_jobs == []
    b.park_xkv(j); b.park_xkv(k)
    assert len(b.log) == 1
    b.finish_xkv()
    assert len(b.log) == 2 and b.log[1][0] == "grouped" and b.log[1][1] is b.tables[0] and b.tables[0][0] == [j, k] and b.xkv_jobs == []
    b.park_xkv(j); b.park_xkv(k)
    b.finish_xkv()
    assert b.log[2][1] is b.tables[0] and len(b.tables) == 1
    b.park_tn(j); b.park_tn(k)            # the same operands through finish_tn: a table of its own
    assert len(b.log) == 4 and b.log[3][1] is b.tables[1] and b.tables[1] is not b.tables[0] and len(b.tn_tables) == 2
    assert sorted(key[0] == "xkv" for key in b.tn_tables) == [False, True]
    b.finish_xkv()                        # nothing parked
    assert len(b.log) == 4


def test_layernorm_partial_sums_are_finished_by_one_launch_over_a_cached_table(make):
    b = make(False)
    p1, p2, p3 = (torch.zeros(n, dtype=F32) for n in (4 * 70 * 2, 2 * 64 * 2, 3 * 33 * 2))
    gw1, gb1, gw2, gb3 = (torch.zeros(n, dtype=BF16) for n in (70, 70, 64, 33))
    recs = [(p1, gw1, gb1, 4, 70), (p2, gw2, None, 2, 64), (p3, None, gb3, 3, 33)]
    for r in recs:
        b.park_ln(r)
    assert b.log == []
    b.finish_ln()
    assert len(b.log) == 1 and b.ln_jobs == []
    kind, tab, n, blocks = b.log[0]
    assert kind == "ln" and n == 3 and blocks == 3 + 2 + 2           # ceil(70 / 32) + ceil(64 / 32) + ceil(33 / 32)
    assert tab.dtype == torch.int64 and tab.device.type == "cpu"
    assert tab.tolist() == [[p1.data_ptr(), gw1.data_ptr(), gb1.data_ptr(), 4, 70, 0],
                            [p2.data_ptr(), gw2.data_ptr(), 0, 2, 64, 3],
                            [p3.data_ptr(), 0, gb3.data_ptr(), 3, 33, 5]]
    for r in recs:                                                   # the same records again: the same table
        b.park_ln(r)
    b.finish_ln()
    assert len(b.log) == 2 and b.log[1][1] is tab and b.log[1][2:] == (3, 7) and len(b.ln_tables) == 1
    b.park_ln(recs[0]); b.park_ln(recs[1])                           # two of them: another table
    b.finish_ln()
    assert len(b.log) == 3 and b.log[2][1] is not tab and b.log[2][2:] == (2, 5) and len(b.ln_tables) == 2
    b.finish_ln()                                                    # nothing parked
    assert len(b.log) == 3


def test_a_region_end_sends_ln_then_tn_then_xkv_and_flushes_and_a_block_end_tn_alone(make):
    b = make(True, side_batch=100, tn_group=100)
    jt, jx = _job(64, 256, 128), _job(308, 256, 128)
    rec = (torch.zeros(2 * 64 * 2, dtype=F32), torch.zeros(64, dtype=BF16), None, 2, 64)
    b.park_xkv(jx); b.park_tn(jt); b.park_ln(rec)
    assert b.log == []
    b.block_end()
    assert [e if isinstance(e, str) else e[0] for e in b.log] == ["enter", "gemm", "exit"] and _is_product_of(b.log[1], jt)
    assert b.tn_jobs == [] and b.ln_jobs == [rec] and b.xkv_jobs == [jx] and b.done is b.forks[0].done
    del b.log[:]
    b.park_tn(jt)
    b.region_end()
    assert [e if isinstance(e, str) else e[0] for e in b.log] == ["enter", "ln", "gemm", "gemm", "exit"]
    assert _is_product_of(b.log[2], jt) and _is_product_of(b.log[3], jx)
    assert (b.q, b.ln_jobs, b.tn_jobs, b.xkv_jobs) == ([], [], [], []) and len(b.forks) == 2 and b.done is b.forks[1].done
    b.region_end()                # nothing parked, nothing queued: no fork
    assert len(b.forks) == 2


def test_begin_and_drop_empty_the_queue_and_the_parked_lists_and_keep_the_tables(make):
    b = make(True, side_batch=100)
    table = torch.zeros(4, dtype=torch.int64)
    lnt, tnt, events = b.ln_tables, b.tn_tables, b.events
    lnt["k"], tnt["k"] = table, table

    def fill():
        b.q, b.ln_jobs, b.tn_jobs, b.xkv_jobs = [1], [1], [1], [1]
        b.ev_cursor, b.rr, b.used, b.done = 5, 3, True, "ev"
    fill()
    b.drop()
    assert (b.q, b.ln_jobs, b.tn_jobs, b.xkv_jobs) == ([], [], [], [])
    assert (b.ev_cursor, b.rr, b.used, b.done) == (5, 3, True, "ev")          # the step goes on: its events stay handed out
    fill()
    b.begin()
    assert (b.q, b.ln_jobs, b.tn_jobs, b.xkv_jobs) == ([], [], [], [])
    assert (b.ev_cursor, b.rr, b.used, b.done) == (0, 0, False, None)
    assert b.ln_tables is lnt and b.tn_tables is tnt and lnt == {"k": table} and tnt == {"k": table} and b.events is events


def test_the_event_pool_hands_out_the_same_events_every_step_and_enter_notes_how_the_backward_ends(make):
    b = make(True, fork_events=False)
    b.events.extend(["e0", "e1"])         # (a new one would be a device event: the pool is pre-filled)
    assert [b.event(), b.event()] == ["e0", "e1"] and b.ev_cursor == 2
    b.begin()
    assert b.event() == "e0"
    events = b.events
    b.reset_events()
    assert b.events is events and events == [] and b.ev_cursor == 0
    assert (b.defer_join, b.parity) == (False, 0)
    b.enter(1, 1)
    assert (b.defer_join, b.parity) == (True, 1)
