"""az_lora_dropout_bf16 (csrc/az_lora.hip) bit for bit against tests/lora_dropout_ref.py: the 16-byte path (rank % 8 == 0) and the
per-element path (rank 4), one to three parts, one row, odd row counts and more than one block, a padded row stride whose sentinel
columns must survive, each kind alone at 0.5 (inv = 2 is exact) and all three together, a row of infinities, every refusal, and a
recorded call replayed through the native launch tape with the device word rewritten between plays."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import elem_ref as R                # noqa: E402
import lora_dropout_ref as D        # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 123456789012                 # needs the key's second word
MIDS = [17, 401, 1679]
CASES = [(1, 1, 8, 1), (154, 77, 16, 3), (130, 65, 4, 1), (130, 65, 4, 3), (128, 64, 64, 3), (96, 48, 32, 1)]
SENTINEL = 0x4D4D
KINDS = {"element": (0.5, 0.0, 0.0), "rank": (0.0, 0.5, 0.0), "module": (0.0, 0.0, 0.5), "all": (0.1, 0.25, 0.5)}


def _bits(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def _input(rows, r, parts, seed=0):
    """bf16 bits [rows][parts r]: Gaussian values, the middle row alternating +inf / -inf."""
    g = torch.Generator().manual_seed(seed)
    u = _bits(torch.randn(rows, parts * r, generator=g).bfloat16()).copy()
    u[rows // 2] = np.where(np.arange(parts * r) % 2 == 0, 0x7F80, 0xFF80).astype(np.uint16)
    return u


def _device(u_bits, ldu):
    rows, width = u_bits.shape
    buf = np.full((rows, ldu), SENTINEL, dtype=np.uint16)
    buf[:, :width] = u_bits
    return R.bits_to_bf16(buf).to(DEV)


def _module_step(mids, t_mod, kept_only=False):
    """The first micro-step at which the reference keeps one of the parts and drops another (one part: drops it); kept_only: the first
    at which it keeps every part."""
    for step in range(1, 200):
        keeps = [D.keep_mod(SEED, step, mid, t_mod) for mid in mids]
        if all(keeps) if kept_only else ((len(mids) == 1 and not keeps[0]) or (any(keeps) and not all(keeps))):
            return step
    raise AssertionError("no such step")


def _run(u_bits, ldu, r, parts, rps, ps, step, word):
    from aozora_sdxl_training_amd import ops
    buf = _device(u_bits, ldu)
    word.fill_(step)
    ops.lora_dropout(buf[:, :parts * r], r, parts, rps, MIDS[:parts], D.thresholds(*ps), float(D.inv_of(ps[0], ps[1])), SEED, word)
    torch.cuda.synchronize()
    return _bits(buf)


@pytest.mark.parametrize("pad", [0, 8], ids=["dense", "ldu+8"])
@pytest.mark.parametrize("rows, rps, r, parts", CASES, ids=[f"{a}x{b}-r{c}-p{d}" for a, b, c, d in CASES])
def test_kernel_matches_the_reference_bit_for_bit(rows, rps, r, parts, pad):
    width, ldu = parts * r, parts * r + pad
    u = _input(rows, r, parts)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    inf_row = rows // 2
    runs = []
    for kind, ps in KINDS.items():          # module dropout: a step that drops a part (of three: and keeps another), and one that keeps all
        t_mod = D.thresholds(*ps)[2]
        runs += [(kind, ps, _module_step(MIDS[:parts], t_mod)), (kind, ps, _module_step(MIDS[:parts], t_mod, True))] if t_mod else [(kind, ps, 5)]
    for kind, ps, step in runs:
        ts = D.thresholds(*ps)
        got = _run(u, ldu, r, parts, rps, ps, step, word)
        want = D.apply_bits(u, r, rps, MIDS[:parts], ts, D.inv_of(ps[0], ps[1]), SEED, step)
        m = D.group_mask(SEED, step, MIDS[:parts], rows, rps, r, ts)
        print(kind, "kept", int(m.sum()), "of", m.size, "mismatches", int((got[:, :width] != want).sum()))
        assert np.array_equal(got[:, :width], want), kind
        assert (got[:, width:] == SENTINEL).all(), kind + ": sentinel columns were touched"
        # dropped elements are +0 (the row of infinities too), kept infinities stay infinities
        assert (got[:, :width][~m] == 0).all() and np.array_equal(got[inf_row, :width][m[inf_row]], u[inf_row][m[inf_row]])
        keeps = [D.keep_mod(SEED, step, mid, ts[2]) for mid in MIDS[:parts]]
        if rows * width >= 64 and kind != "module" and any(keeps):
            assert 0 < m.sum() < m.size, (kind, step)
        if kind == "module":
            for p, k in enumerate(keeps):       # not rescaled: a kept part keeps its bits, a dropped part is all +0
                assert np.array_equal(got[:, p * r:(p + 1) * r], u[:, p * r:(p + 1) * r] if k else np.zeros((rows, r), np.uint16))
    # a kind at 0 has no effect: element dropout alone equals the reference with the other two masks all-ones (checked above), and
    # the step that drops a module under "module" changes nothing while t_mod = 0
    a = _run(u, ldu, r, parts, rps, KINDS["element"], 5, word)
    b = D.apply_bits(u, r, rps, MIDS[:parts], (32768, 0, 0), 2.0, SEED, 5)
    keep = np.concatenate([D.keep_net(SEED, 5, mid, rows, r, 32768) for mid in MIDS[:parts]], axis=1)
    assert np.array_equal(a[:, :width], b) and np.array_equal(a[:, :width] != 0, keep & (u != 0))


def test_vector_and_element_paths_agree():
    """A rank-8 buffer whose row stride is no multiple of 8 takes the per-element kernel: the same bits as the 16-byte path."""
    rows, rps, r, parts = 66, 33, 8, 2
    u = _input(rows, r, parts, seed=2)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    ps = KINDS["all"]
    want = D.apply_bits(u, r, rps, MIDS[:parts], D.thresholds(*ps), D.inv_of(ps[0], ps[1]), SEED, 11)
    for ldu in (16, 24, 20):
        got = _run(u, ldu, r, parts, rps, ps, 11, word)
        assert np.array_equal(got[:, :16], want) and (got[:, 16:] == SENTINEL).all(), ldu


def test_refusals_return_nonzero_and_launch_nothing():
    from aozora_sdxl_training_amd import ops
    from aozora_sdxl_training_amd._lib import lib, AozoraError
    fn = lib()._fn["az_lora_dropout_bf16"]
    u = _input(8, 8, 3)
    buf = _device(u, 32)
    before = _bits(buf).copy()
    word = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(rows=8, r=8, parts=3, rps=4, ldu=32, t=(32768, 32768, 32768), w=P(word)):
        return fn(rows, r, parts, rps, P(buf), ldu, 1, 2, 3, *t, 4.0, SEED, w, st)
    codes = [call(parts=0), call(parts=4), call(r=12), call(r=128), call(rows=7), call(ldu=16), call(t=(-1, 0, 0)), call(t=(0, 65536, 0)),
             call(t=(0, 0, 1 << 20)), call(w=None)]
    torch.cuda.synchronize()
    assert codes == [-1140, -1140, -1141, -1141, -1142, -1143, -1144, -1144, -1144, -1145]
    assert np.array_equal(_bits(buf), before)
    view = buf[:, :24]
    for bad in (dict(r=4), dict(parts=2), dict(rps=3), dict(mids=[1, 2]), dict(ts=(0, 0, 0)), dict(ts=(1, 2, 65536)), dict(word=word.float()),
                dict(word=word.cpu()), dict(u=view.float())):
        kw = dict(u=view, r=8, parts=3, rps=4, mids=[1, 2, 3], ts=(32768, 0, 0), word=word)
        kw.update(bad)
        with pytest.raises(AozoraError):
            ops.lora_dropout(kw["u"], kw["r"], kw["parts"], kw["rps"], kw["mids"], kw["ts"], 2.0, SEED, kw["word"])
    torch.cuda.synchronize()
    assert np.array_equal(_bits(buf), before)


def test_replayed_launch_follows_the_device_word():
    """One recorded call, replayed through the native launch tape: its scalar arguments are the recorded ones, the micro-step is read
    from the device word at every play."""
    from aozora_sdxl_training_amd import ops
    from aozora_sdxl_training_amd._lib import lib
    from aozora_sdxl_training_amd.tape import NativeTape
    rows, rps, r, parts = 154, 77, 16, 3
    ps = KINDS["all"]
    ts, inv = D.thresholds(*ps), D.inv_of(ps[0], ps[1])
    u = _input(rows, r, parts, seed=4)
    src = _device(u, parts * r)
    buf = src.clone()
    word = torch.full((1,), 3, dtype=torch.int32, device=DEV)
    L = lib()
    L.recorder = []
    try:
        ops.lora_dropout(buf, r, parts, rps, MIDS, ts, float(inv), SEED, word)
        recorded = L.recorder
    finally:
        L.recorder = None
    assert [op.name for op in recorded] == ["az_lora_dropout_bf16"]
    torch.cuda.synchronize()
    assert np.array_equal(_bits(buf), D.apply_bits(u, r, rps, MIDS, ts, inv, SEED, 3))
    nt = NativeTape(recorded)
    assert nt.n_calls == 1 and not nt.callbacks
    outs = []
    for step in (9, 3, 2 ** 31 - 1):
        buf.copy_(src)
        word.fill_(step)
        nt.play()
        torch.cuda.synchronize()
        outs.append(_bits(buf).copy())
        assert np.array_equal(outs[-1], D.apply_bits(u, r, rps, MIDS, ts, inv, SEED, step)), step
    assert not np.array_equal(outs[0], outs[1])
