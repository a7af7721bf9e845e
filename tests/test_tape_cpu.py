"""Launch tape (tape.py): the peephole (fuse_records), the native tape and the Python replay over typed operations, and the
stop-event slot of the launch wrapper (include/aozora_hip.h az_set_launch_stop_event): host logic only, no device needed."""
import ctypes

import pytest

from aozora_sdxl_training_amd._lib import lib, AozoraError, ForkEvent, Call, Record, Wait, Live, get_option, set_option
from aozora_sdxl_training_amd.tape import NativeTape, fuse_records, replay


class _Stream:
    def __init__(self, h):
        self.cuda_stream = h


def _ev(h):
    e = ForkEvent.__new__(ForkEvent)      # no HIP call: only the handle and the type matter to the peephole
    e.cuda_event = h
    return e


def _call(name, stream, L):
    proto = L.protos[name][1]
    args = [0] * len(proto)
    args[[i for i, (_, an) in enumerate(proto) if an == "stream"][0]] = ctypes.c_void_p(stream.cuda_stream)
    return Call(name, tuple(args))


def _shape(seq):
    out = []
    for op in seq:
        if isinstance(op, Call) and op.name == "az_set_launch_stop_event":
            a = op.args[0]
            out.append(("set", a.value if hasattr(a, "value") else a))
        elif isinstance(op, Call):
            out.append(op.name)
        elif isinstance(op, Record):
            out.append(("record", op.event.cuda_event))
        elif isinstance(op, Wait):
            out.append(("wait_on", op.event.cuda_event))
        else:
            assert isinstance(op, Live)
            out.append(("live", op.args))
    return out


def test_record_behind_a_kernel_rides_on_it_and_a_repeated_record_is_an_alias():
    L = lib()
    A, B = _Stream(0x1000), _Stream(0x2000)
    e1, e2, e3 = _ev(11), _ev(22), _ev(33)
    seq = [_call("az_add_rows", A, L), Record(e1, A), Wait(B, e1), _call("az_silu_bwd", B, L), Record(e3, B),
           Record(e2, A), Wait(B, e2), _call("az_geglu_bwd", B, L)]
    out, fused = fuse_records(seq)
    assert fused == 3
    assert _shape(out) == [("set", 11), "az_add_rows", ("set", None), ("wait_on", 11), ("set", 33), "az_silu_bwd", ("set", None),
                              ("wait_on", 11), "az_geglu_bwd"]          # e2 marks the same point of A as e1: dropped, its wait re-pointed
    out, fused = fuse_records(seq, only_stream=A.cuda_stream)
    assert fused == 2 and ("record", 33) in _shape(out) and ("set", 33) not in _shape(out)


def test_anything_between_the_kernel_and_the_record_keeps_the_record():
    L = lib()
    A, B = _Stream(0x1000), _Stream(0x2000)
    for between in ([Wait(A, _ev(5))],                                         # the stream waits for something first
                    [Live(lambda: 0, ())],                                     # host logic
                    [_call("az_memset_async", A, L)],                          # not a kernel of the launch wrapper
                    [Call("az_set_option", (b"GEMM8", 1))]):                   # no stream argument: do not reason across it
        e = _ev(7)
        seq = [_call("az_add_rows", A, L)] + between + [Record(e, A), Wait(B, e)]
        out, fused = fuse_records(seq)
        assert fused == 0 and ("record", 7) in _shape(out)
    e = _ev(9)
    seq = [_call("az_add_rows", A, L), _call("az_add_rows", B, L), Record(e, A)]      # a launch on ANOTHER stream in between does not matter
    out, fused = fuse_records(seq)
    assert fused == 1 and _shape(out)[:3] == [("set", 9), "az_add_rows", ("set", None)]


def test_clearing_a_stop_event_no_launch_carried_is_an_error():
    L = lib()
    f = L._fn["az_set_launch_stop_event"]
    assert f(None) == 0
    assert f(ctypes.c_void_p(0x1234)) == 0
    assert f(None) != 0                   # nothing was launched while it was set: it would stay unrecorded
    assert f(None) == 0


def test_live_operation_with_an_argument_inside_a_fused_region_keeps_the_record():
    L = lib()
    A = _Stream(0x1000)
    e = _ev(7)
    seq = [_call("az_add_rows", A, L), Live([].append, (3,)), Record(e, A)]
    out, fused = fuse_records(seq)
    assert fused == 0 and _shape(out) == ["az_add_rows", ("live", (3,)), ("record", 7)]


@pytest.fixture
def exclusive_option():
    """LDS_EXCLUSIVE (what az_gemm_set_exclusive sets) starts at 0 and gets its value back: the process-wide option table is
    shared with every other test of this process."""
    saved = get_option("LDS_EXCLUSIVE")
    set_option("LDS_EXCLUSIVE", 0)
    yield
    set_option("LDS_EXCLUSIVE", saved)


def _synthetic(log):
    """Two host-only entry points of the dispatch table -- az_set_launch_stop_event(NULL) and az_gemm_set_exclusive (an option
    store; az_gemm.hip, az_runtime.hip: neither reaches a HIP call) -- with a live operation behind each; the live operations read
    the option, so the log shows that each ran between the right calls."""
    note = lambda *tag: log.append(tag + (get_option("LDS_EXCLUSIVE"),))
    return [Call("az_set_launch_stop_event", (None,)), Live(note, ()), Call("az_gemm_set_exclusive", (1,)), Live(note, ("second",))]


def test_native_tape_plays_calls_and_live_operations_in_order(exclusive_option):
    log = []
    nt = NativeTape(_synthetic(log))
    assert (nt.n, nt.n_calls, len(nt.callbacks)) == (4, 2, 2) and log == []
    nt.play()
    assert log == [(0,), ("second", 1)]           # each live operation fired once, with its arguments, behind the call in front of it


def test_native_tape_issues_a_call_outside_the_dispatch_table_from_python(exclusive_option):
    v = ctypes.c_int(-1)
    nt = NativeTape([Call("az_gemm_set_exclusive", (1,)), Call("az_get_option", (b"LDS_EXCLUSIVE", ctypes.byref(v)))])
    assert (nt.n, nt.n_calls) == (2, 1) and isinstance(nt.callbacks[1], Call) and v.value == -1
    nt.play()
    assert v.value == 1


def test_python_replay_matches_the_native_tape_and_disarms_the_stop_event_on_failure(exclusive_option):
    log = []
    replay(_synthetic(log))
    assert log == [(0,), ("second", 1)]
    f = lib()._fn["az_set_launch_stop_event"]
    # az_tape_add on a NULL tape returns its argument error before anything else (az_tape.hip)
    with pytest.raises(AozoraError, match="az_tape_add"):
        replay([Call("az_set_launch_stop_event", (ctypes.c_void_p(0x1234),)), Call("az_tape_add", (None, 0, 0, None, 0)),
                Live(log.append, ("not reached",))])
    assert f(None) == 0 and len(log) == 2         # the armed event was cleared by the failed replay; nothing ran behind the failure
