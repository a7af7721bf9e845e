"""params.ParamStore on the CPU, without a device or the library: the slot layout, the region cuts, the transposed-copy (W^T) jobs and their
per-region tables, the state dicts and the region-event protocol, at the mini configuration without adapters and with
LoraSpec(4, 8.0, "", "unet", 8, 4.0).  The counts and offsets are the ones AozoraUNet laid out before the store was split from it."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aozora_sdxl_training_amd import params as P                                                  # noqa: E402
from aozora_sdxl_training_amd.unet_spec import LoraSpec, lora_table, mini_config, param_table     # noqa: E402

CUTS = (1904640, 9400320)
STRADDLERS = ((1902720, 1), (9396864, 2))        # (offset of a weight that lies across a cut, the later region)
#             parameters, flat_numel, linear jobs, 3x3 jobs, trainable end, table jobs per region, loose jobs per region
GOLDEN = {"plain": (620, 31883264, 173, 38, 31880640, (117, 71, 327), (0, 0, 0)),
          "lora": (1094, 32890880, 562, 72, 32890304, (117, 71, 684), (0, 0, 338))}


def make(kind, cls=P.ParamStore):
    cfg = mini_config()
    base = param_table(cfg)
    return cls(cfg, base + (lora_table(cfg, LoraSpec(4, 8.0, "", "unet", 8, 4.0)) if kind == "lora" else []), len(base), "cpu")


@pytest.fixture(scope="module")
def stores():
    """Read-only: the tests that change a store make their own."""
    return {kind: make(kind) for kind in GOLDEN}


@pytest.mark.parametrize("kind", list(GOLDEN))
def test_golden_layout(stores, kind):
    s = stores[kind]
    n, numel, lin, conv, tend, _, _ = GOLDEN[kind]
    assert len(s._table) == len(s._slots) == len(s._params) == len(list(s.parameters())) == n
    assert [k for k, _ in s.named_parameters()] == [k for k, _ in s._table]
    assert s.flat_numel == numel == s.pflat.numel() == s.gflat.numel() == s.wtflat.numel()
    assert (len(s._wt_jobs), len(s._wt_conv_jobs)) == (lin, conv)
    assert s.region_bounds() == [(0, CUTS[0]), (CUTS[0], CUTS[1]), (CUTS[1], numel)] and s.tail_offset() == CUTS[1]
    assert s.trainable_ranges() == [(0, tend)]


def test_adapters_leave_the_base_slots_where_they_are(stores):
    plain, lora = stores["plain"], stores["lora"]
    assert list(lora._slots)[:len(plain._slots)] == list(plain._slots)
    assert all(lora._slots[k] == v for k, v in plain._slots.items())
    assert lora._wt_jobs[:len(plain._wt_jobs)] == plain._wt_jobs                     # adapter linear jobs behind the base ones
    assert lora._wt_conv_jobs[-len(plain._wt_conv_jobs):] == plain._wt_conv_jobs     # adapter 3x3 jobs in front of the base ones


def table_offsets(s, k):
    """Source offsets (elements) of the jobs in region k's table and of its loose jobs."""
    tab, njobs, tiles, loose = s._refresh_table(*s.region_bounds()[k])
    rows = tab.tolist() if tab is not None else []
    assert njobs == len(rows) and tiles == sum((r[3] + 63) // 64 * ((r[2] + 63) // 64) for r in rows)
    return [(r[0] - s.pflat.data_ptr()) // 2 for r in rows], [j[0] for j in loose]


@pytest.mark.parametrize("kind", list(GOLDEN))
def test_region_tables_partition_the_jobs(stores, kind):
    s = stores[kind]
    per = [table_offsets(s, k) for k in range(3)]
    assert tuple(len(t) for t, _ in per) == GOLDEN[kind][5] and tuple(len(l) for _, l in per) == GOLDEN[kind][6]
    want = sorted([o for o, _, _ in s._wt_jobs] + [o + tap * ci for o, _, ci in s._wt_conv_jobs for tap in range(9)])
    assert len(want) == len(s._wt_jobs) + 9 * len(s._wt_conv_jobs) == {"plain": 515, "lora": 1210}[kind]
    assert sorted(o for t, l in per for o in t + l) == want          # every job in exactly one region
    assert s._refresh_table(*s.region_bounds()[0]) is s._refresh_table(*s.region_bounds()[0])      # built once
    jobs = {o: r * c for o, r, c in s._wt_jobs} | {o: co * 9 * ci for o, co, ci in s._wt_conv_jobs}
    for o, later in STRADDLERS:
        cut = CUTS[later - 1]
        assert o < cut < o + jobs[o]
        assert [k for k in range(3) if o in per[k][0] + per[k][1]] == [later]


@pytest.mark.parametrize("kind", list(GOLDEN))
def test_structural_invariants(stores, kind):
    s = stores[kind]
    assert P.ALIGN == 64 and all(o % 64 == 0 for o, _, _ in s._slots.values())
    assert all(v % 4096 == 0 for lo, hi in s.region_bounds() for v in (lo, hi)) and s.flat_numel % 4096 == 0
    jobs = {o: (r, c) for o, r, c in s._wt_jobs}
    q = [n for n in s._slots if n.endswith("attn1.to_q.weight")]
    k2 = [n for n in s._slots if n.endswith("attn2.to_k.weight")]
    assert q and k2
    for n in q:
        o, st, _ = s._slots[n]
        assert jobs[o] == (3 * st[0], st[1])
        assert s._slots[n.replace("to_q", "to_k")][0] not in jobs and s._slots[n.replace("to_q", "to_v")][0] not in jobs
    for n in k2:
        o, st, _ = s._slots[n]
        assert jobs[o] == (2 * st[0], st[1]) and s._slots[n.replace("to_k", "to_v")][0] not in jobs
    o, st, shape = s._slots["conv_in.weight"]
    assert st[3] == 8 and shape[1] == 4 and s._w["conv_in.weight"].shape[3] == 8 and s._params["conv_in.weight"].shape[1] == 4
    for name, (o, st, shape) in s._slots.items():
        p, g = s._params[name], s._gviews[name]
        assert tuple(p.shape) == tuple(g.shape) == shape and p._az_owner is s and p._az_name == name
        assert p.data_ptr() == s.pflat.data_ptr() + 2 * o == s._w[name].data_ptr()
        assert g.data_ptr() == s.gflat.data_ptr() + 2 * o == s._gw[name].data_ptr()
    W = s._w[q[0]]
    assert s._wt(W).data_ptr() == s.wtflat.data_ptr() + 2 * s._slots[q[0]][0] and s._wt(W).shape == (W.shape[1], W.shape[0])
    Wf, Gf, tr = s._fused_w([q[0], q[0].replace("to_q", "to_k"), q[0].replace("to_q", "to_v")])
    assert Wf.shape == jobs[s._slots[q[0]][0]] and Wf.data_ptr() == W.data_ptr() and Gf.data_ptr() == s._gw[q[0]].data_ptr() and tr


def test_state_dict_round_trip_and_freeze():
    s = make("plain")
    s._wt_dirty = False
    noise = torch.randn(s.flat_numel, generator=torch.Generator().manual_seed(3)).bfloat16()
    sd = {n: noise[s._slots[n][0]:][:math.prod(shape)].view(shape) for n, shape in s._base_table}
    assert s.load_state_dict(sd) is s and s._wt_dirty
    out = s.state_dict()
    assert list(out) == [n for n, _ in s._base_table] and all(torch.equal(out[n], sd[n]) for n in sd)
    assert not s._w["conv_in.weight"][..., 4:].any()                # the padding channels stay zero
    with pytest.raises(KeyError):
        s.load_state_dict({}, strict=True)
    name = "mid_block.resnets.0.conv1.bias"
    o, st, _ = s._slots[name]
    s._params[name].requires_grad = False
    assert not s.trainable(name) and s.trainable_ranges() == [(0, o), (o + (math.prod(st) + 63) // 64 * 64, GOLDEN["plain"][4])]
    s.expose_grads()
    assert s._params[name].grad is None and s._params["conv_in.weight"].grad is s._gviews["conv_in.weight"]
    assert s.requires_grad_(True) is s and s.trainable_ranges() == [(0, GOLDEN["plain"][4])]


class _Stream:
    cuda_stream = 0

    def __init__(self, log):
        self.log = log

    def wait_event(self, ev):
        self.log.append(("wait", ev))


class _Lib:
    def __init__(self, log):
        self.log = log

    def call(self, name, *args):
        self.log.append((name, args[1]) if name == "az_transpose_multi_bf16" else (name,))


class _Stubbed(P.ParamStore):
    """The store with its stream seam and the library replaced by recorders."""
    log: list = []

    def _stream(self):
        return _Stream(self.log)


def test_a_region_with_a_pending_event_is_refreshed_by_its_wait(monkeypatch):
    s = make("lora", _Stubbed)
    log = s.log = []
    monkeypatch.setattr(P, "lib", lambda: _Lib(log))
    tabs, loose = GOLDEN["lora"][5], GOLDEN["lora"][6]
    s.set_region_params_event(2, "ev2")
    s.refresh_transposed()                       # dirty from the start: regions 0 and 1 now, region 2 when it has landed
    assert log == [("az_transpose_multi_bf16", tabs[0]), ("az_transpose_multi_bf16", tabs[1])]
    assert not s._wt_dirty and s._wt_region_pending == {2} and s._region_events == {2: "ev2"}
    del log[:]
    s.refresh_transposed()                       # fresh: nothing
    s.wait_region_params(1)                      # no event, nothing pending: nothing
    assert log == []
    s.wait_region_params(2)
    assert log == [("wait", "ev2"), ("az_transpose_multi_bf16", tabs[2])] + [("az_transpose_bf16",)] * loose[2]
    assert s._wt_region_pending == set() and s._region_events == {}
    del log[:]
    s.wait_tail_params()
    assert log == []
    s.mark_params_dirty()
    s.set_region_params_event(1, "ev1")
    s.refresh_transposed()
    s.transposed_refreshed_externally()          # the optimizer refreshed every region itself: region 1's wait only waits
    s.wait_tail_params()
    assert [e for e in log if e[0] == "wait"] == [("wait", "ev1")] and sum(e[0] == "az_transpose_multi_bf16" for e in log) == 2


def test_ready_and_busy_events_are_waited_for_once():
    s = make("plain", _Stubbed)
    log = s.log = []
    s._wait_wt_ready()
    s.zero_grad()
    assert log == []
    s._wt_ready = "ready"
    s.grads_busy_until("upd")
    s.gflat[:64] = 1
    s.expose_grads()
    s._wait_wt_ready(); s._wait_wt_ready()
    s.zero_grad(); s.zero_grad()
    assert log == [("wait", "ready"), ("wait", "upd")] and not s.gflat.any() and all(p.grad is None for p in s.parameters())
