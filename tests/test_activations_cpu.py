"""The gradient-buffer rules and the deferred-reader bookkeeping of activations.ActivationStore on CPU tensors: when a contribution to an
activation's gradient is written in place, out of place or aliases a layer's dY (the rule that lets the parameter-gradient branch read
any dY at any later time without a wait), that the pool's allocation order never depends on need_grad flags, and which readers a
micro-step waits for."""
import itertools

import pytest
import torch

from aozora_sdxl_training_amd import activations, ops
from aozora_sdxl_training_amd._lib import AozoraError
from aozora_sdxl_training_amd.activations import ActivationStore

BF16, F32 = torch.bfloat16, torch.float32
KEY = (1, 8, 8, 77, 0)


@pytest.fixture
def store():
    s = ActivationStore("cpu")
    s.begin(KEY, recording=False)
    return s


@pytest.fixture
def adds(monkeypatch):
    """ops.add_rows replaced by a logger of (a, b, out): nothing is launched."""
    log = []
    monkeypatch.setattr(ops, "add_rows", lambda a, b, out: log.append((a, b, out)))
    return log


def test_the_module_stands_without_the_executor():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, aozora_sdxl_training_amd.activations as a; "
            "assert 'aozora_sdxl_training_amd.unet' not in sys.modules; a.ActivationStore('cpu')")
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0
    from aozora_sdxl_training_amd import unet
    for name in ("Act", "POOL_ALIGN", "_Arena", "_Pool"):
        assert getattr(unet, name) is getattr(activations, name)


def test_new_takes_one_pool_buffer_whatever_the_flag_and_dtype(store):
    a = store.new(6, 10)
    b = store.new(6, 10, need_grad=False)
    c = store.new(3, 4, need_grad=False, dtype=F32)
    assert all(x.t is buf for x, buf in zip((a, b, c), store.pool.bufs)) and len(store.pool.bufs) == 3
    assert store.pool.cursor == 3
    assert [(tuple(x.t.shape), x.t.dtype, x.need_grad) for x in (a, b, c)] == [((6, 10), BF16, True), ((6, 10), BF16, False), ((3, 4), F32, False)]
    assert all(x.g is None and x.ready is None and not x.g_alias for x in (a, b, c))


def test_gbuf_no_gradient_yet_takes_a_buffer_and_overwrites(store):
    a = store.new(6, 10)
    cur = store.pool.cursor
    dst, add = store.gbuf(a)
    assert add is None and dst is a.g and dst is store.pool.bufs[cur] and not a.g_alias
    assert store.pool.cursor == cur + 1 and tuple(dst.shape) == (6, 10) and dst.dtype == BF16


def test_gbuf_owned_gradient_accumulates_in_place_without_a_buffer(store):
    a = store.new(6, 10)
    first, _ = store.gbuf(a)
    cur = store.pool.cursor
    for _ in range(3):
        dst, add = store.gbuf(a)
        assert dst is first and add is first and a.g is first and not a.g_alias
    assert store.pool.cursor == cur


def test_gbuf_aliased_gradient_goes_out_of_place_and_the_dy_is_never_a_destination_again(store, adds):
    a = store.new(6, 10)
    dy = torch.zeros(6, 10, dtype=BF16)
    store.give_grad(a, dy)                         # alias=True: dy is some layer's dY
    assert a.g is dy and a.g_alias
    cur = store.pool.cursor
    dst, add = store.gbuf(a)
    assert add is dy and dst is not dy and dst is a.g and dst is store.pool.bufs[cur] and not a.g_alias
    assert store.pool.cursor == cur + 1
    for _ in range(3):                             # owned from here on: in place, and never dy
        d2, a2 = store.gbuf(a)
        assert d2 is dst and a2 is dst and d2.data_ptr() != dy.data_ptr()
    assert store.pool.cursor == cur + 1 and adds == []


def test_a_gradient_given_without_alias_is_owned(store, adds):
    """concat hands slices of its own gradient on (alias=False unless that gradient is itself a dY): they may be written in place."""
    a = store.new(6, 10)
    sl = torch.zeros(6, 10, dtype=BF16)
    cur = store.pool.cursor
    store.give_grad(a, sl, alias=False)
    assert a.g is sl and not a.g_alias
    assert store.gbuf(a) == (sl, sl) and store.pool.cursor == cur and adds == []


def test_gbuf_single_raises_on_a_second_consumer(store, adds):
    a = store.new(6, 10)
    dst = store.gbuf_single(a, "attention projections")
    assert dst is a.g
    with pytest.raises(AozoraError, match="attention projections must have a single consumer"):
        store.gbuf_single(a, "attention projections")
    b = store.new(6, 10)
    store.give_grad(b, torch.zeros(6, 10, dtype=BF16))
    with pytest.raises(AozoraError, match="GEGLU projection must have a single consumer"):
        store.gbuf_single(b, "GEGLU projection")


def test_give_grad_aliases_then_adds_out_of_place_then_in_place(store, adds):
    a = store.new(6, 10)
    dy1, dy2, dy3 = (torch.zeros(6, 10, dtype=BF16) for _ in range(3))
    cur = store.pool.cursor
    store.give_grad(a, dy1)                        # no gradient yet: aliases, no buffer, no launch
    assert a.g is dy1 and a.g_alias and store.pool.cursor == cur and adds == []
    store.give_grad(a, dy2)                        # aliased: a fresh buffer = dy1 + dy2, dy1 untouched
    fresh = store.pool.bufs[cur]
    assert a.g is fresh and not a.g_alias and store.pool.cursor == cur + 1
    assert len(adds) == 1 and adds[0][0] is dy1 and adds[0][1] is dy2 and adds[0][2] is fresh
    store.give_grad(a, dy3)                        # owned: in place
    assert a.g is fresh and store.pool.cursor == cur + 1
    assert len(adds) == 2 and adds[1][0] is fresh and adds[1][1] is dy3 and adds[1][2] is fresh


def test_give_grad_ignores_an_activation_that_needs_no_gradient(store, adds):
    a = store.new(6, 10, need_grad=False)
    cur = store.pool.cursor
    for _ in range(2):
        store.give_grad(a, torch.zeros(6, 10, dtype=BF16))
    assert a.g is None and not a.g_alias and store.pool.cursor == cur and adds == []


def _sequence(store, flags):
    """A fixed call sequence over one activation under test (t) and three others whose need_grad flags vary.  The others go through
    everything that may not look at the flag: new, gbuf (no gradient yet, owned), gbuf_single, and a first contribution through
    give_grad (which takes no buffer either way).  -> the pool index of every buffer handed out, in call order."""
    got = []

    def idx(tensor):
        got.append(next(i for i, b in enumerate(store.pool.bufs) if b is tensor))
    o = [store.new(5, 12, need_grad=flags[0]), store.new(7, 3, need_grad=flags[1], dtype=F32), store.new(5, 12, need_grad=flags[2])]
    t = store.new(5, 12)
    for a in o + [t]:
        idx(a.t)
    idx(store.gbuf(o[0])[0])
    store.give_grad(t, torch.zeros(5, 12, dtype=BF16))
    store.give_grad(o[2], torch.zeros(5, 12, dtype=BF16))
    idx(store.gbuf(t)[0])
    idx(store.gbuf(o[0])[0])
    idx(store.gbuf_single(o[1], "other"))
    idx(store.pool.get((9,), F32))
    store.give_grad(t, torch.zeros(5, 12, dtype=BF16))
    idx(t.g)
    idx(store.new(2, 2).t)
    return got


def test_allocation_order_does_not_depend_on_the_flags_of_other_activations(adds, monkeypatch):
    """The freeze-mask independence the adapters rely on: one launch tape per bucket serves every mask only if the n-th buffer of a step is
    the same buffer under each."""
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    tables, orders, ptrs = [], [], []
    for flags in itertools.product((True, False), repeat=3):
        s = ActivationStore("cpu")
        s.begin(KEY, recording=False)
        orders.append(_sequence(s, flags))
        tables.append([(tuple(b.shape), b.dtype) for b in s.pool.bufs])
        s.begin(KEY, recording=False)              # the arena is taken here; the replay hands out the same table again
        assert _sequence(s, flags[::-1]) == orders[-1]
        ptrs.append([b.data_ptr() - s.arena_of(0).buf.data_ptr() for b in s.pool.bufs])
        assert ptrs[-1] == s.pool.offsets
    assert orders[0] == [0, 1, 2, 3, 4, 5, 4, 6, 7, 5, 8]
    assert all(o == orders[0] for o in orders) and all(t == tables[0] for t in tables) and all(p == ptrs[0] for p in ptrs)


class _Stream:
    def __init__(self, log):
        self.log = log

    def wait_event(self, ev):
        self.log.append(ev)


def test_wait_free_pops_the_readers_of_that_parity_only(monkeypatch):
    log = []
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: _Stream(log))
    s = ActivationStore("cpu")
    assert not s.has_deferred()
    s.wait_free(0)
    assert log == []
    s.leave_readers(0, ["e0a", "e0b"])
    s.leave_readers(1, ["e1"])
    assert s.has_deferred()
    s.wait_free(0)
    assert log == ["e0a", "e0b"] and s.deferred == {1: ["e1"]} and s.has_deferred()
    s.wait_free(0)
    assert log == ["e0a", "e0b"]
    s.wait_free(1)
    assert log == ["e0a", "e0b", "e1"] and not s.has_deferred()
    s.leave_readers(1, ["e1"])
    s.clear_readers()
    assert not s.has_deferred() and log == ["e0a", "e0b", "e1"]


def test_settle_clears_the_readers_of_every_parity(monkeypatch):
    log = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: log.append("sync"))
    s = ActivationStore("cpu", on_replace=lambda arena: log.append(("replace", dict(s.deferred), s.pool, arena.capacity)))
    s.begin(KEY, recording=False)
    s.pool.get((4, 4), BF16)
    s.leave_readers(0, ["e0"])
    s.leave_readers(1, ["e1"])
    s.settle(s.arena_of(1))                        # nothing pending on parity 1: nothing happens
    assert log == [] and s.has_deferred() and s.generation == 0
    s.settle(s.arena_of(0))
    # synchronised first; by the time the executor is told, the readers are gone, no pool is current and the old arena still stands
    assert log == ["sync", ("replace", {}, None, 0)]
    assert not s.has_deferred() and s.generation == 1 and s.arena_of(0).capacity == 256
