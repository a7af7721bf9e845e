"""LOSS_TYPE through trainer.train (the helpers of tests/test_trainer_gpu.py, 4 micro-steps): "MSE" and the key absent are the same run
bit for bit; pseudo-Huber at c = 2^20 reproduces the MSE run's first loss (there it is the squared error); a narrow Huber and L1 do
not -- before LOSS_TYPE was read every one of them trained MSE; a LOSS_TYPE that cannot be read is refused before a UNet is loaded."""
import contextlib
import io
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import test_trainer_gpu as T        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ABSENT = object()
_RUNS = {}


def run(tmp_factory, loss_type, mode="v_prediction"):
    """History, final parameters and output of a 4-micro-step run with this LOSS_TYPE (ABSENT: no such attribute), once per module."""
    key = (loss_type if loss_type is not ABSENT else None, loss_type is ABSENT, mode)
    if key in _RUNS:
        return _RUNS[key]
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd import checkpoint as C
    from aozora_sdxl_training_amd.trainer import train
    from aozora_sdxl_training_amd.telemetry import Reporter
    from aozora_sdxl_training_amd.unet_spec import mini_config
    model = mini_config(ctx_dim=64, pooled=32)
    tmp = str(tmp_factory.mktemp("loss_run"))
    over = dict(MAX_TRAIN_STEPS=4, SAVE_EVERY_N_STEPS=0)
    if loss_type is not ABSENT:
        over["LOSS_TYPE"] = loss_type
    cfg = T._config(tmp, mode, **over)
    assert hasattr(cfg, "LOSS_TYPE") == (loss_type is not ABSENT)
    T._base_checkpoint(cfg.SINGLE_FILE_CHECKPOINT_PATH, model)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        unet = C.load_unet(cfg.SINGLE_FILE_CHECKPOINT_PATH, DEV, model)
        h = train(cfg, unet=unet, device=DEV, reporter=Reporter(cfg.MAX_TRAIN_STEPS, asynchronous=False))
    torch.cuda.synchronize()
    assert h["micro_step"] == 4 and h["optimizer_step"] == 2 and len(h["losses"]) == 4
    _RUNS[key] = (h, unet.pflat.clone(), buf.getvalue())
    return _RUNS[key]


def test_mse_and_the_absent_key_are_the_same_run(tmp_path_factory):
    h0, p0, out0 = run(tmp_path_factory, ABSENT)
    h1, p1, out1 = run(tmp_path_factory, "MSE")
    assert h1["losses"] == h0["losses"] and h1["grad_norms"] == h0["grad_norms"] and h1["lrs"] == h0["lrs"] and torch.equal(p1, p0)
    assert "LOSS_TYPE" not in out0 and "LOSS_TYPE" not in out1


def test_huber_at_c_2_to_20_reproduces_the_first_mse_loss(tmp_path_factory):
    h0, _, _ = run(tmp_path_factory, "MSE")
    h, _, out = run(tmp_path_factory, "Huber:c=1048576,schedule=constant")
    a, b = h["losses"][0], h0["losses"][0]
    print(f"first loss: huber(c=2^20) {a!r} mse {b!r}")
    assert abs(a - b) <= 2e-6 * abs(b)
    assert "INFO: LOSS_TYPE: pseudo-Huber (c = 1.04858e+06, schedule constant)" in out and "the reported loss is this loss" in out


@pytest.mark.parametrize("loss_type", ["Huber:c=0.01", "L1"])
def test_other_losses_do_not_reproduce_the_mse_loss(tmp_path_factory, loss_type):
    h0, p0, _ = run(tmp_path_factory, "MSE")
    h, p, out = run(tmp_path_factory, loss_type)
    a, b = h["losses"][0], h0["losses"][0]
    print(f"first loss: {loss_type} {a!r} mse {b!r}")
    assert a == a and a > 0 and abs(a - b) > 2e-6 * abs(b)
    assert all(l == l and l > 0 for l in h["losses"]) and all(g > 0 for g in h["grad_norms"]) and not torch.equal(p, p0)
    assert "INFO: LOSS_TYPE:" in out


def test_min_snr_changes_the_weights_only(tmp_path_factory):
    """epsilon, gamma = 5: the first loss is the MSE run's first loss with every sample's weight times m_t (checked through the sign
    only: m_t <= 1, so the loss cannot grow), and the INFO line names gamma."""
    h0, _, _ = run(tmp_path_factory, "MSE", mode="epsilon")
    h, _, out = run(tmp_path_factory, "MSE:min_snr_gamma=5", mode="epsilon")
    assert 0 < h["losses"][0] <= h0["losses"][0] and h["losses"] != h0["losses"]
    assert "INFO: LOSS_TYPE: MSE, min-SNR gamma = 5" in out


def test_a_bad_loss_type_is_refused_before_a_unet_is_loaded(tmp_path, monkeypatch):
    from aozora_sdxl_training_amd import checkpoint as C
    from aozora_sdxl_training_amd.trainer import train

    def no_load(*a, **k):
        raise AssertionError("a UNet was loaded")
    monkeypatch.setattr(C, "load_unet", no_load)
    for mode, bad in (("v_prediction", "logcosh"), ("epsilon", "huber:c=0"), ("rectified_flow", "mse:min_snr_gamma=5"), ("epsilon", "l1:c=0.1")):
        cfg = T._config(str(tmp_path), mode, LOSS_TYPE=bad)
        assert not os.path.exists(cfg.SINGLE_FILE_CHECKPOINT_PATH)
        with pytest.raises(ValueError, match="LOSS_TYPE"):
            train(cfg, unet=None, device=DEV)
