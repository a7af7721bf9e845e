"""Native launch tape (include/aozora_hip.h az_tape_*).  The recorded launch sequence of a resolution bucket is a list of typed
operations (_lib.Call / Record / Wait / Live): C-ABI calls by entry-point name, event records, stream waits, and the host logic the
executor marked as live (data-parallel region waits, scheduling hints, the end-of-backward join).  fuse_records rewrites it,
NativeTape compiles it into a C-side tape that az_tape_play re-issues without the interpreter -- the live operations stay Python
and run at the tape's BREAK operations -- and replay issues it from Python.  All three branch on the kind of an operation and on
nothing else.  SURVEY.md 8b names this seam `az_unet_step`; the reference issues the same sequence from Python / autograd every
step (train.py:2743-2767)."""
from __future__ import annotations

import ctypes
import struct

from ._lib import lib, AozoraError, ForkEvent, Call, Record, Wait, Live

OP_CALL, OP_EVENT_RECORD, OP_STREAM_WAIT, OP_BREAK = 0, 1, 2, 3


def _word(ty: str, a) -> int:
    if ty == "float":
        return struct.unpack("<I", struct.pack("<f", float(a)))[0]
    if hasattr(a, "value"):            # ctypes scalar / c_void_p
        a = a.value
    if a is None:
        return 0
    return int(a)


# Entry points whose LAST operation is a kernel launched on `stream` through the library's launch wrapper (az_launch): only these
# may carry a fork event as the completion signal of that kernel.  An ALLOW-list: an entry point missing here is merely not fused
# (its record packet stays), while a wrongly fused one -- last operation a memcpy, a memset, a stream wait -- would leave its event
# unrecorded.  tests/test_abi_cpu.py checks that every entry point with a stream argument is classified in exactly one of the two.
_KERNEL_ENTRIES = frozenset({
    "az_spin", "az_gemm_bf16", "az_gemm_nt_grouped_bf16", "az_gemm_tn_grouped_bf16", "az_gemm_geglu_fwd_bf16", "az_gemm_wgrad_bias_bf16",
    "az_conv2d_bf16", "az_conv2d_wgrad_bias_bf16", "az_attn_fwd", "az_attn_bwd", "az_groupnorm_fwd", "az_groupnorm_bwd",
    "az_groupnorm_bwd_ex", "az_layernorm_fwd", "az_layernorm_bwd", "az_layernorm_bwd_ex", "az_layernorm_bwd_partial",
    "az_ln_param_finish_multi", "az_geglu_fwd", "az_geglu_bwd", "az_silu_fwd", "az_silu_bwd", "az_add_rows", "az_upsample2x_fwd",
    "az_upsample2x_bwd", "az_upsample_nearest_fwd", "az_upsample_nearest_bwd", "az_colsum", "az_colsum_grad", "az_reduce_segs_to_bf16", "az_transpose_bf16", "az_transpose_bf16_batched",
    "az_transpose_multi_bf16", "az_f32_to_bf16", "az_timestep_embed", "az_nchw_to_nhwc_pad", "az_nhwc_to_nchw", "az_noise_target",
    "az_mse_loss_fwd_bwd", "az_sumsq_bf16", "az_sumsq", "az_clip_coef", "az_adamw_flat", "az_adamw_flat_ex", "az_adamw_flat_sr", "az_scale_bf16",
    "az_scale_f32", "az_stage_inputs", "az_adamw8bit_step", "az_ema_flat", "az_adamw_flat_master", "az_robust_loss_fwd_bwd", "az_adamw_flat_seg",
    "az_noise_shape", "az_noise_target_ex", "az_prodigy_begin", "az_prodigy_moments", "az_prodigy_finish", "az_prodigy_apply", "az_adafactor_step",
    "az_lora_down_bf16", "az_lora_up_bf16", "az_lora_wgrad_bf16", "az_lora_up_geglu_bf16",
    "az_lora_conv_down_bf16", "az_lora_conv_dgrad_bf16", "az_lora_conv_wgrad_bf16", "az_lora_dropout_bf16", "az_lora_max_norm_bf16",
    "az_dora_norm_bf16", "az_dora_scale_bf16", "az_dora_bwd_bf16"})
# ... and the ones with a stream argument that end in something else (graph capture / launch, event and stream calls, copies)
_NOT_KERNEL_ENTRIES = frozenset({"az_graph_begin", "az_graph_end", "az_graph_launch", "az_event_record", "az_stream_wait_event",
                                 "az_stream_sync", "az_memset_async", "az_memcpy_async", "az_titan_offload"})


def fuse_records(recorded, only_stream=None):
    """Peephole over a recorded launch sequence: `ABI call X on stream S` directly followed (on S) by `ForkEvent.record(S)` becomes
    `az_set_launch_stop_event(ev); X; az_set_launch_stop_event(NULL)` -- the event rides on X's last kernel as its completion
    signal and the record packet disappears from S (include/aozora_hip.h az_set_launch_stop_event; tools/event_cost.cpp).
    A second record on S with nothing queued on S since the first marks the same point: it is dropped and the waits on its event
    are re-pointed to the first event.  Anything else that touches S in between (another call, a wait, host logic) keeps the record.
    only_stream: fuse records on that stream only.  -> (new sequence, number of records fused)."""
    stream_arg = {name: [i for i, (_, an) in enumerate(args) if an == "stream"] for name, (_, args) in lib().protos.items()}
    out, fused = [], 0          # out: [operation, event handle or None]
    last = {}                   # stream handle -> index in out of the latest kernel-launching call on it, while nothing else touched the stream
    last_rec = {}               # stream handle -> the ForkEvent recorded on it last, while nothing else touched the stream since
    alias = {}                  # id(ForkEvent) -> the earlier ForkEvent that marks the same point of its stream (its record is dropped)
    for op in recorded:
        if isinstance(op, Call):
            idx = stream_arg.get(op.name)
            out.append([op, None])
            if not idx:
                last.clear(); last_rec.clear()      # option changes, context calls ...: do not reason across them
            else:
                st = _word("void*", op.args[idx[0]])
                last_rec.pop(st, None)
                if op.name not in _KERNEL_ENTRIES:
                    last.pop(st, None)
                else:
                    last[st] = len(out) - 1
        elif isinstance(op, Record):
            ev, st = op.event, op.stream.cuda_stream
            fork = isinstance(ev, ForkEvent)        # torch events are never fused
            if fork and (only_stream is None or st == only_stream):
                if st in last_rec:           # nothing was queued on the stream since the previous record: the same point of the stream
                    alias[id(ev)] = last_rec[st]
                    fused += 1
                    continue
                k = last.pop(st, None)
                if k is not None and out[k][1] is None:
                    out[k][1] = ev.cuda_event
                    last_rec[st] = ev
                    fused += 1
                    continue
            last.pop(st, None); last_rec.pop(st, None)
            if fork:
                last_rec[st] = ev
            out.append([op, None])
        elif isinstance(op, Wait):
            st = op.stream.cuda_stream
            out.append([Wait(op.stream, alias.get(id(op.event), op.event)), None])
            last.pop(st, None); last_rec.pop(st, None)
        else:
            out.append([op, None])
            last.clear(); last_rec.clear()   # host logic: anything may happen inside
    flat = []
    for op, ev in out:
        if ev is None:
            flat.append(op)
        else:
            flat += [Call("az_set_launch_stop_event", (ctypes.c_void_p(ev),)), op, Call("az_set_launch_stop_event", (None,))]
    return flat, fused


def disarm_stop_event():
    """Clear this thread's launch stop event after a failed replay (az_set_launch_stop_event(NULL); its 'never carried' error is
    the very state being cleaned up and is ignored)."""
    lib()._fn["az_set_launch_stop_event"](None)


def issue(op):
    """Issue one operation from Python."""
    if isinstance(op, Call):
        rc = lib()._fn[op.name](*op.args)
        if rc:
            raise AozoraError(f"{op.name} failed with code {rc} while re-issuing the launch tape")
    elif isinstance(op, Record):
        op.event.record(op.stream)
    elif isinstance(op, Wait):
        op.event.wait(op.stream)
    else:
        op.fn(*op.args)


def replay(recorded):
    """Re-issue a recorded sequence from Python (ExecPolicy.native_tape off)."""
    try:
        for op in recorded:
            issue(op)
    except BaseException:
        disarm_stop_event()        # a failing operation between `set` and `clear` must not leave the event armed
        raise


class NativeTape:
    def __init__(self, recorded):
        L = lib()
        self._L = L
        self.handle = ctypes.c_void_p()
        if L._fn["az_tape_create"](ctypes.byref(self.handle)):      # not through L.call: nothing here may land on a recording tape
            raise AozoraError("az_tape_create failed")
        self.callbacks = {}            # op index of a BREAK -> the operation to issue from Python there
        self.n = 0
        self.n_calls = 0
        add = L._fn["az_tape_add"]

        def push(kind, fn_id, words):
            arr = (ctypes.c_long * max(1, len(words)))(*[w if w < (1 << 63) else w - (1 << 64) for w in words])
            rc = add(self.handle, kind, fn_id, ctypes.cast(arr, ctypes.c_void_p), len(words))
            if rc:
                raise AozoraError(f"az_tape_add failed with code {rc}")
            self.n += 1

        for op in recorded:
            fid = L._fn["az_tape_fn_id"](op.name.encode()) if isinstance(op, Call) else -1
            if fid >= 0:
                push(OP_CALL, fid, [_word(t, a) for (t, _), a in zip(L.protos[op.name][1], op.args)])
                self.n_calls += 1
            elif isinstance(op, Record):
                push(OP_EVENT_RECORD, 0, [op.event.cuda_event, op.stream.cuda_stream])
            elif isinstance(op, Wait):
                push(OP_STREAM_WAIT, 0, [op.stream.cuda_stream, op.event.cuda_event])
            else:       # host logic, or an entry point outside the generated dispatch table: issued by the caller at a BREAK
                self.callbacks[self.n] = op
                push(OP_BREAK, 0, [])
        self._play = L._fn["az_tape_play"]

    def play(self):
        try:
            self._play_all()
        except BaseException:
            disarm_stop_event()        # a failing entry / callback between `set` and `clear` must not leave the event armed
            raise

    def _play_all(self):
        i = 0
        while i < self.n:
            nxt = self._play(self.handle, i)
            if nxt < 0:
                idx, rc = ctypes.c_long(), ctypes.c_int()
                self._L._fn["az_tape_last_error"](self.handle, ctypes.byref(idx), ctypes.byref(rc))
                raise AozoraError(f"native launch tape: operation {idx.value} failed with code {rc.value}")
            if nxt <= i:
                raise AozoraError("native launch tape made no progress")
            op = self.callbacks.get(nxt - 1)
            if op is not None:
                issue(op)
            i = nxt

    def __del__(self):
        try:
            if self.handle:
                self._L._fn["az_tape_destroy"](self.handle)
        except Exception:
            pass
