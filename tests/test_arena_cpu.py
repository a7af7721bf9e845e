"""The activation arena, its pools and the store that replaces arenas (activations._Arena / _Pool / ActivationStore) are pure
bookkeeping and run on the CPU: offsets, replay, growth, generations and the memory bound
arena <= max need + 256 B x (buffers of the largest bucket)."""
import itertools

import pytest
import torch

from aozora_sdxl_training_amd._lib import AozoraError
from aozora_sdxl_training_amd.activations import POOL_ALIGN, ActivationStore, _Arena, _Pool

BF16, F32 = torch.bfloat16, torch.float32
SMALL = [((3, 5), BF16), ((7,), F32), ((2, 4, 4, 8), BF16), ((129,), BF16), ((64, 2), F32)]
MID = [((40, 33), BF16), ((1000,), F32), ((3, 5), BF16)]
LARGE = [((64, 64), BF16), ((5000,), F32), ((17, 19), BF16), ((1,), F32), ((300, 7), BF16), ((128,), BF16)]


def _up(n):
    return (n + POOL_ALIGN - 1) // POOL_ALIGN * POOL_ALIGN


def _need(shapes):
    total = 0
    for shape, dtype in shapes:
        n = 1
        for d in shape:
            n *= d
        total += _up(n * (2 if dtype == BF16 else 4))
    return total


def _settle(arena):
    """What ActivationStore.settle does to the arena between micro-steps, without the device."""
    if arena.pending():
        arena.grow()
        return True
    return False


def _run(pool, shapes):
    pool.reset()
    return [pool.get(shape, dtype) for shape, dtype in shapes]


def _visit(arena, pools, name, shapes, times=3):
    for _ in range(times):
        _settle(arena)
        if name not in pools:
            pools[name] = _Pool("cpu", arena)
        bufs = _run(pools[name], shapes)
    return bufs


def test_alignment_is_256_bytes():
    assert POOL_ALIGN == 256


def test_nbytes_is_the_sum_of_the_rounded_buffers():
    # 3*5*2 = 30 -> 256 ; 7*4 = 28 -> 256 ; 2*4*4*8*2 = 512 -> 512 ; 129*2 = 258 -> 512 ; 64*2*4 = 512 -> 512
    assert _need(SMALL) == 256 + 256 + 512 + 512 + 512
    pool = _Pool("cpu")
    _run(pool, SMALL)
    assert pool.nbytes() == 2048
    assert pool.arena.wanted == 2048         # ... and that is what the arena is asked for


def test_offsets_are_deterministic_and_aligned():
    tables = []
    for _ in range(2):
        arena = _Arena("cpu")
        pool = _Pool("cpu", arena)
        _run(pool, LARGE)
        assert _settle(arena)
        bufs = _run(pool, LARGE)
        assert all(o % POOL_ALIGN == 0 for o in pool.offsets)
        assert pool.offsets == list(itertools.accumulate([0] + [_up(b.numel() * b.element_size()) for b in bufs[:-1]]))
        base = arena.buf.data_ptr()
        assert [b.data_ptr() - base for b in bufs] == pool.offsets          # the buffers ARE views of the arena at those offsets
        assert [(tuple(b.shape), b.dtype) for b in bufs] == [(s, d) for s, d in LARGE]
        tables.append(list(pool.offsets))
    assert tables[0] == tables[1]


def test_same_address_on_every_pass_after_reset():
    arena, pools = _Arena("cpu"), {}
    _visit(arena, pools, "a", LARGE, times=2)
    first = [b.data_ptr() for b in _run(pools["a"], LARGE)]
    for _ in range(3):
        assert [b.data_ptr() for b in _run(pools["a"], LARGE)] == first
    # another bucket in between uses the same memory and moves nothing
    _visit(arena, pools, "b", SMALL)
    assert [b.data_ptr() for b in _run(pools["a"], LARGE)] == first
    assert arena.generation == 1


def test_buffers_do_not_overlap_and_hold_data():
    arena, pools = _Arena("cpu"), {}
    bufs = _visit(arena, pools, "a", LARGE)
    for i, b in enumerate(bufs):
        b.fill_(i + 1)
    for i, b in enumerate(bufs):
        assert bool((b.float() == i + 1).all())
    spans = sorted((b.data_ptr(), b.data_ptr() + b.numel() * b.element_size()) for b in bufs)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert spans[0][0] >= arena.buf.data_ptr() and spans[-1][1] <= arena.buf.data_ptr() + arena.capacity


def test_replay_mismatch_is_an_error():
    arena, pools = _Arena("cpu"), {}
    _visit(arena, pools, "a", SMALL)
    pool = pools["a"]
    pool.reset()
    pool.get((3, 5), BF16)
    with pytest.raises(AozoraError, match="replay mismatch"):
        pool.get((8,), F32)                  # the table says (7,) fp32
    pool.reset()
    with pytest.raises(AozoraError, match="replay mismatch"):
        pool.get((3, 5), F32)                # same shape, other dtype


def test_clearing_the_pools_restarts_at_offset_zero_of_the_arena_still_held():
    arena, pools = _Arena("cpu"), {}
    _visit(arena, pools, "a", LARGE)
    base, gen = arena.buf.data_ptr(), arena.generation
    pools.clear()
    bufs = _visit(arena, pools, "a", MID)      # another allocation sequence under the same key
    assert arena.buf.data_ptr() == base and arena.generation == gen
    assert pools["a"].offsets[0] == 0 and bufs[0].data_ptr() == base
    assert pools["a"].nbytes() == _need(MID)


def test_growth_bumps_the_generation_and_old_pools_reassign_their_offsets():
    arena, pools = _Arena("cpu"), {}
    small = _visit(arena, pools, "s", SMALL)
    assert arena.generation == 1 and arena.capacity == _need(SMALL)
    offsets_before = list(pools["s"].offsets)
    # a larger bucket: its first run spills into buffers of its own, the arena is replaced before the next run
    _settle(arena)
    pools["l"] = _Pool("cpu", arena)
    spilled = _run(pools["l"], LARGE)
    assert arena.generation == 1 and arena.pending() and arena.wanted == _need(LARGE)
    lo, hi = arena.buf.data_ptr(), arena.buf.data_ptr() + arena.capacity
    assert any(not (lo <= b.data_ptr() < hi) for b in spilled)
    del spilled, small
    assert _settle(arena)
    assert arena.generation == 2 and arena.capacity == _need(LARGE)
    assert pools["s"].bufs and pools["s"]._gen == 1          # stale until its next visit ...
    bufs = _run(pools["s"], SMALL)
    assert pools["s"]._gen == 2 and pools["s"].offsets == offsets_before
    base = arena.buf.data_ptr()
    assert [b.data_ptr() - base for b in bufs] == offsets_before            # ... then inside the NEW arena
    large = _run(pools["l"], LARGE)
    assert [b.data_ptr() - base for b in large] == pools["l"].offsets
    assert pools["s"].nbytes() == _need(SMALL) and pools["l"].nbytes() == _need(LARGE)
    assert not _settle(arena) and arena.generation == 2


ORDERS = {
    "ascending": ["s", "m", "l"],
    "descending": ["l", "m", "s"],
    "mixed": ["m", "s", "l", "s", "m", "l", "s"],
}
SHAPES = {"s": SMALL, "m": MID, "l": LARGE}


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_arena_is_bounded_by_the_largest_bucket(order):
    arena, pools = _Arena("cpu"), {}
    seen = []
    for name in ORDERS[order]:
        _visit(arena, pools, name, SHAPES[name])
        seen.append(name)
        largest = max(seen, key=lambda n: _need(SHAPES[n]))
        need = {n: pools[n].nbytes() for n in pools}
        assert need == {n: _need(SHAPES[n]) for n in pools}
        assert max(need.values()) <= arena.capacity <= need[largest] + POOL_ALIGN * len(SHAPES[largest])
    # growth happened once per new largest bucket and never otherwise
    records, best = 0, 0
    for name in ORDERS[order]:
        if _need(SHAPES[name]) > best:
            best, records = _need(SHAPES[name]), records + 1
    assert arena.generation == records


def test_replacing_an_arena_keeps_what_other_parities_recorded(monkeypatch):
    """ActivationStore.settle with no device, its on_replace the executor's own hook (AozoraUNet._arena_replaced on a bare object
    that has only the fields the hook touches, its parameter-gradient branch a real GradBranch): the device is synchronised BEFORE anything is released, the TrainStep objects let
    go before the old arena does, only pools of the replaced arena are dropped -- and the pointer tables stay: launch tapes of the
    other parity hold their raw addresses (they were once cleared here, and a double-buffered run replayed a tape over freed
    tables)."""
    from aozora_sdxl_training_amd.branch import GradBranch
    from aozora_sdxl_training_amd.unet import AozoraUNet, ExecPolicy
    log = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: log.append("sync"))
    u = object.__new__(AozoraUNet)
    s = u.acts = ActivationStore("cpu", on_replace=u._arena_replaced)
    assert (s.pools, s.pool, s.arenas, s.generation, s.deferred) == ({}, None, {}, 0, {})
    s.leave_readers(0, ["ev"])
    b = u.branch = GradBranch(ExecPolicy(), s, [], "cpu")
    u._tape, b.q, b.ln_jobs, b.tn_jobs, b.xkv_jobs, u._hoisted = [1], [1], [1], [1], [1], {"a": 1}
    table = torch.zeros(4, dtype=torch.int64)
    b.ln_tables["k"], b.tn_tables["k"], u._group_tables = table, table, {"k": table}

    class Client:
        def _arena_replaced(self, arena):
            log.append(("client", arena.capacity))
    client = Client()
    s.add_client(client)
    a0, a1 = s.arena_of(0), s.arena_of(1)
    assert s.arena_of("call") is a0 and a0 is not a1
    for key, arena, shapes in (((2, 16, 16, 77, 0), a0, SMALL), ((2, 16, 16, 77, 1), a1, MID)):
        s.pools[key] = _Pool("cpu", arena)
        _run(s.pools[key], shapes)
    assert s.prepare(0) == 1 and log == ["sync", ("client", 0)]
    assert not s.has_deferred()
    assert (u._tape, b.q, b.ln_jobs, b.tn_jobs, b.xkv_jobs, u._hoisted) == ([], [], [], [], [], {})
    assert s.prepare(1) == 1 and s.generation == 2
    p0, p1 = s.pools[(2, 16, 16, 77, 0)], s.pools[(2, 16, 16, 77, 1)]
    _run(p0, SMALL); _run(p1, MID)
    addr1 = [b.data_ptr() for b in p1.bufs]
    # a larger bucket on parity 0
    s.pools[(2, 24, 24, 77, 0)] = _Pool("cpu", a0)
    _run(s.pools[(2, 24, 24, 77, 0)], LARGE)
    del log[:]
    assert s.prepare(1) == 1 and log == []                      # nothing pending there
    assert s.prepare(0) == 2 and log == ["sync", ("client", _need(SMALL))]
    assert s.generation == 3 and a0.capacity == _need(LARGE) and a1.generation == 1
    assert not p0.bufs and [b.data_ptr() for b in p1.bufs] == addr1   # parity 1 keeps its views
    assert b.ln_tables == {"k": table} and b.tn_tables == {"k": table} and u._group_tables == {"k": table}
    assert s.activation_bytes() == {"arena": {0: _need(LARGE), 1: _need(MID)}, "generation": 3,
                                    "need": {(2, 16, 16, 77, 0): _need(SMALL), (2, 16, 16, 77, 1): _need(MID), (2, 24, 24, 77, 0): _need(LARGE)}}
    # ... and the UNet's forwarders and properties read the same store
    assert u.activation_bytes() == s.activation_bytes() and u.generation == 3 and u._pool is s.pool and u._arena_of(1) is a1
    assert u.prepare_pool(0) == 2 and not u.has_deferred()


def test_begin_settles_makes_and_rewinds_the_pool_but_never_settles_under_a_recording(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    s = ActivationStore("cpu")
    key = (2, 16, 16, 77, 1)
    s.begin(key, recording=False)
    assert s.pool is s.pools[key] and s.pool.arena is s.arena_of(1) and s.generation == 0
    [s.pool.get(shape, dtype) for shape, dtype in SMALL]
    s.begin(key, recording=True)                 # pending, but a recording is running: the arena stays as it is
    assert s.generation == 0 and s.pool is s.pools[key] and s.pool.cursor == 0 and s.pool.bufs
    s.begin(key, recording=False)
    assert s.generation == 1 and s.arena_of(1).capacity == _need(SMALL) and s.pool is s.pools[key] and not s.pool.bufs
    s.begin((2, 16, 16, 77, "call"), recording=False)
    assert s.pool.arena is s.arena_of(0)
