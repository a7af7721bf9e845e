"""The training loop around the HIP step (train.py:2544-2830 restated on this package's objects): data feed -> micro-step
(TrainStep: noise mix, UNet forward, weighted MSE, backward) -> clip -> Raven / Titan / 8-bit AdamW / Prodigy -> LR curve -> reporter ->
checkpoints / resume.  It is the caller of the hot path (SURVEY.md 8a row a1 with the 8f rows plugged in); no GUI, no
offline caching -- `config` is any object with the reference's flat attribute names (config.TrainingConfig builds one from
a GUI preset: `python -m aozora_sdxl_training_amd.trainer --config X.json`, see main()).

Deviations kept deliberately: noise / rectified-flow jitter are drawn on a CPU generator (the
reference draws on the device generator, whose stream is backend specific), and the three per-micro-step `.item()` syncs of
the reference collapse into one read of the loss scalar, taken one micro-step late so that the device queue never drains.
"""
from __future__ import annotations

import gc
import time
from collections import deque
from pathlib import Path
from typing import Optional

import torch

from . import checkpoint as ckpt
from . import data as feed
from . import lora as lora_mod
from .clip import clip_grad_norm_
from .ema import EmaWeights, read_options as _ema_options
from .loss import fold_min_snr, parse_loss_type
from .noise import draw_aux, parse_noise_mode
from . import param_groups as pgroups
from .optimizers import Adafactor, PagedAdamW8bit, Prodigy, RavenAdamW, TitanAdamW
from .schedule import (CustomCurveLRScheduler, TimestepSampler, ddpm_alphas_cumprod, generate_noise, make_time_ids,
                       seeded_torch_generator, timestep_loss_curve_from_config, trainable_mask)
from .telemetry import Reporter
from .train_step import TrainStep

_RAVEN_DEFAULTS = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, debias_strength=0.3, momentum_dtype="bfloat16")
_ADAMW8_DEFAULTS = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)      # config.py PAGED_ADAMW_8BIT_PARAMS
_SR_8BIT_REFUSAL = ("stochastic_rounding is an option of raven and titan (RAVEN_PARAMS / TITAN_PARAMS): paged_adamw_8bit writes its "
                    "parameters through two roundings of its own, a different contract -- remove the key from PAGED_ADAMW_8BIT_PARAMS")
_MASTER_8BIT_REFUSAL = ("master_weights is an option of raven and titan (RAVEN_PARAMS / TITAN_PARAMS): paged_adamw_8bit has no fp32 master "
                        "copy -- remove the key from PAGED_ADAMW_8BIT_PARAMS")
_MASTER_SR_REFUSAL = ("master_weights and stochastic_rounding do not combine: stochastic rounding exists because there is no fp32 master "
                      "copy -- with one, the bf16 parameters are its round-to-nearest image; set one of the two keys")
_MASTER_HOST_TITAN_REFUSAL = ("master_weights does not combine with TITAN_HOST_GRADIENTS = true: that path runs the drop-in "
                              "optimizers.TitanAdamW (fp32 gradients in pinned host memory), which keeps no master copy -- drop one of the two")
_ADAMW8_DP_REFUSAL = "paged_adamw_8bit runs at one rank only: data-parallel training supports raven and titan"
_PRODIGY_DP_REFUSAL = ("prodigy runs at one rank only: its step size is estimated from two sums over ALL trainable elements, which the "
                       "data-parallel shards do not exchange -- data-parallel training supports raven and titan")
_PRODIGY_SR_REFUSAL = ("stochastic_rounding is an option of raven and titan (RAVEN_PARAMS / TITAN_PARAMS): prodigy always keeps an fp32 "
                       "master copy, of which the bf16 parameters are the round-to-nearest image -- remove the key from PRODIGY_PARAMS")
_PRODIGY_MASTER_REFUSAL = ("master_weights is an option of raven and titan (RAVEN_PARAMS / TITAN_PARAMS): prodigy always keeps an fp32 "
                           "master copy, there is nothing to switch -- remove the key from PRODIGY_PARAMS")
_PRODIGY_GROUPS_REFUSAL = ("param_groups is an option of raven, titan and paged_adamw_8bit: prodigy estimates ONE step size over all "
                           "trainable elements and takes one group -- remove the key from PRODIGY_PARAMS")
_PRODIGY_KEYS = ("betas", "beta3", "eps", "weight_decay", "use_bias_correction", "safeguard_warmup", "d0", "d_coef", "growth_rate",
                 "ema_decay", "ema_warmup")
_ADAFACTOR_DP_REFUSAL = ("adafactor runs at one rank only: its row and column means and the per-tensor RMS of the update run over WHOLE "
                         "tensors, which the data-parallel shards cut -- data-parallel training supports raven and titan")
_ADAFACTOR_GROUPS_REFUSAL = ("param_groups is an option of raven, titan and paged_adamw_8bit: optimizers.Adafactor takes one group (its "
                             "per-tensor scalars are dealt from one descriptor table) -- remove the key from ADAFACTOR_PARAMS")
_ADAFACTOR_MASTER_REFUSAL = ("master_weights is an option of raven and titan (RAVEN_PARAMS / TITAN_PARAMS): optimizers.Adafactor keeps no "
                             "fp32 master copy yet -- \"stochastic_rounding\": true is its answer to updates below the bf16 spacing; remove "
                             "the key from ADAFACTOR_PARAMS")
_ADAFACTOR_KEYS = ("eps", "clip_threshold", "decay_rate", "beta1", "weight_decay", "scale_parameter", "relative_step", "warmup_init",
                   "stochastic_rounding", "ema_decay", "ema_warmup")
_PARAMS_KEY = {"titan": "TITAN_PARAMS", "paged_adamw_8bit": "PAGED_ADAMW_8BIT_PARAMS", "prodigy": "PRODIGY_PARAMS", "adafactor": "ADAFACTOR_PARAMS"}


def _momentum_dtype(v):
    """create_optimizer (train.py:2262-2263, 2268-2269): the string "bfloat16" selects bf16, ANY other value fp32 (fp16 state
    is only reachable by constructing RavenAdamW / TitanAdamW directly with torch.float16)."""
    if isinstance(v, torch.dtype):
        return v
    return torch.bfloat16 if v == "bfloat16" else torch.float32


class _Silent:
    def log_step(self, *a, **k): pass
    def log_message(self, *a, **k): pass
    def shutdown(self): pass


class _NoState:
    """Placeholder for the training-state file of a data-parallel run (the optimizer state lives in the per-rank shards)."""
    def save_cpu_state(self): return {"_sharded": True}


def _optimizer(config, params):
    """create_optimizer (train.py:2257-2330) for the two optimizers of the hot path."""
    kind = str(getattr(config, "OPTIMIZER_TYPE", "raven")).lower()
    curve = getattr(config, "LR_CUSTOM_CURVE", [])
    lr = max(p[1] for p in curve) if curve else config.LEARNING_RATE
    user = dict(getattr(config, "TITAN_PARAMS" if kind == "titan" else "RAVEN_PARAMS", {}) or {})
    hp = {**_RAVEN_DEFAULTS, **user}
    mdt = _momentum_dtype(hp.pop("momentum_dtype", "bfloat16"))
    cls = TitanAdamW if kind == "titan" else RavenAdamW
    return cls([{"params": params, "lr_scale": 1.0}], lr=lr, betas=tuple(hp["betas"]), eps=hp["eps"], weight_decay=hp["weight_decay"],
               debias_strength=hp["debias_strength"], momentum_dtype=mdt, **_sr_args(config, hp))


def _sr_args(config, hp):
    """"stochastic_rounding": true in RAVEN_PARAMS / TITAN_PARAMS (absent = false; not in the reference) -> the optimizers' keywords;
    the seed is the run's SEED, so a resumed run (same seed, restored step count) draws the bits the uninterrupted run draws."""
    on = hp.get("stochastic_rounding", False)
    on = on.strip().lower() in ("true", "1", "t", "y", "yes") if isinstance(on, str) else bool(on)      # config.coerce_types' reading of a bool
    return dict(stochastic_rounding=on, sr_seed=int(getattr(config, "SEED", 0) or 0))


def _as_bool(v):
    return v.strip().lower() in ("true", "1", "t", "y", "yes") if isinstance(v, str) else bool(v)      # config.coerce_types' reading of a bool


def _master_option(config) -> bool:
    """"master_weights": true in RAVEN_PARAMS / TITAN_PARAMS (absent = false; not in the reference): an fp32 master copy of the trainable
    weights in the flat optimizers (dist.ShardedRaven / ShardedTitan; INTEGRATION.md "fp32 master weights").  Refuses, before anything
    is allocated, what it does not combine with: the 8-bit optimizer, stochastic rounding, Titan with host gradients."""
    kind = str(getattr(config, "OPTIMIZER_TYPE", "raven")).lower()
    if kind == "paged_adamw_8bit":
        if "master_weights" in dict(getattr(config, "PAGED_ADAMW_8BIT_PARAMS", {}) or {}):
            raise ValueError(_MASTER_8BIT_REFUSAL)
        return False
    if kind == "prodigy":           # its own master copy, always (prodigy_options refuses the key)
        return False
    if kind == "adafactor":         # no master copy (adafactor_options refuses the key)
        return False
    hp = dict(getattr(config, "TITAN_PARAMS" if kind == "titan" else "RAVEN_PARAMS", {}) or {})
    if not _as_bool(hp.get("master_weights", False)):
        return False
    if _as_bool(hp.get("stochastic_rounding", False)):
        raise ValueError(_MASTER_SR_REFUSAL)
    if kind == "titan" and bool(getattr(config, "TITAN_HOST_GRADIENTS", False)):
        raise ValueError(_MASTER_HOST_TITAN_REFUSAL)
    return True


def _optimizer_8bit(config, params, groups=None):
    """create_optimizer (train.py:2271-2288): PagedAdamW8bit from PAGED_ADAMW_8BIT_PARAMS at lr = max(curve), min_8bit_size 4096.
    groups (param_groups.Resolved, None = off; not in the reference's trainer): one torch group per resolved group with its lr_scale (the
    scheduler scales it, train.py:347-352) and weight_decay, the BASE group last -- the loop reports param_groups[-1]["lr"], the curve's
    unscaled value.  The kernel takes per-group hyper-parameters in its one launch already."""
    curve = getattr(config, "LR_CUSTOM_CURVE", [])
    lr = max(p[1] for p in curve) if curve else config.LEARNING_RATE
    hp = {**_ADAMW8_DEFAULTS, **dict(getattr(config, "PAGED_ADAMW_8BIT_PARAMS", {}) or {})}
    if "stochastic_rounding" in hp:
        raise ValueError(_SR_8BIT_REFUSAL)
    if "master_weights" in hp:
        raise ValueError(_MASTER_8BIT_REFUSAL)
    if groups is not None:
        members = [[] for _ in groups.groups]
        for p in params:
            members[groups.param_gid[p._az_name]].append(p)
        order = list(range(1, len(groups.groups))) + [0]
        params = [{"params": members[g], "lr_scale": groups.groups[g][0], "weight_decay": groups.groups[g][1]} for g in order]
    return PagedAdamW8bit(params, lr=lr, betas=tuple(hp["betas"]), eps=hp["eps"], weight_decay=hp["weight_decay"], min_8bit_size=4096)


def prodigy_options(config, world: int = 1) -> dict:
    """PRODIGY_PARAMS (config.py: `<mode>_prodigy_params` of the preset's active block, default {}) -> the keywords of
    optimizers.Prodigy, lr excepted (that is max(curve), as for the other optimizers).  Refuses, before anything is allocated: more than
    one rank, the options of the flat optimizers that have no meaning here, an unknown key (a typo must not silently train the default),
    eps <= 0, d0 <= 0, betas outside [0, 1).  Absent keys take the optimizer's defaults (INTEGRATION.md "The Prodigy optimizer")."""
    from .optimizers.prodigy import check_options
    if world > 1:
        raise ValueError(_PRODIGY_DP_REFUSAL)
    hp = dict(getattr(config, "PRODIGY_PARAMS", None) or {})
    for key, why in (("stochastic_rounding", _PRODIGY_SR_REFUSAL), ("master_weights", _PRODIGY_MASTER_REFUSAL), ("param_groups", _PRODIGY_GROUPS_REFUSAL)):
        if key in hp:
            raise ValueError(why)
    unknown = sorted(k for k in hp if k not in _PRODIGY_KEYS)
    if unknown:
        raise ValueError(f"PRODIGY_PARAMS holds unknown key(s) {unknown}: this build reads {sorted(_PRODIGY_KEYS)} (the learning rate comes "
                         "from LR_CUSTOM_CURVE)")
    kw = {k: hp[k] for k in _PRODIGY_KEYS[:9] if k in hp and hp[k] is not None}
    try:
        for k in ("eps", "weight_decay", "d0", "d_coef", "growth_rate", "beta3"):
            if k in kw:
                kw[k] = float(kw[k])
        if "betas" in kw:
            kw["betas"] = tuple(float(b) for b in kw["betas"])
    except (TypeError, ValueError):
        raise ValueError(f"PRODIGY_PARAMS: a numeric option cannot be read as a number: {hp}") from None
    for k in ("use_bias_correction", "safeguard_warmup"):
        if k in kw:
            kw[k] = _as_bool(kw[k])
    check_options(kw.get("betas", (0.9, 0.999)), kw.get("beta3"), kw.get("eps", 1e-8), kw.get("d0", 1e-6))
    return kw


def adafactor_options(config, world: int = 1) -> dict:
    """ADAFACTOR_PARAMS (config.py: `<mode>_adafactor_params` of the preset's active block, default {}) -> the keywords of
    optimizers.Adafactor, lr excepted (that is the curve's, as for the other optimizers; ignored under relative_step) and with the
    stochastic-rounding seed taken from SEED.  Refuses, before anything is allocated: more than one rank, param_groups, master_weights,
    an unknown key (a typo must not silently train the default), a value that cannot be read, and what the constructor refuses
    (warmup_init without relative_step, clip_threshold <= 0, beta1 outside [0, 1)).  Absent keys take the optimizer's defaults
    (INTEGRATION.md "The Adafactor optimizer")."""
    from .optimizers.adafactor import check_options
    if world > 1:
        raise ValueError(_ADAFACTOR_DP_REFUSAL)
    hp = dict(getattr(config, "ADAFACTOR_PARAMS", None) or {})
    for key, why in (("param_groups", _ADAFACTOR_GROUPS_REFUSAL), ("master_weights", _ADAFACTOR_MASTER_REFUSAL)):
        if key in hp:
            raise ValueError(why)
    unknown = sorted(k for k in hp if k not in _ADAFACTOR_KEYS)
    if unknown:
        raise ValueError(f"ADAFACTOR_PARAMS holds unknown key(s) {unknown}: this build reads {sorted(_ADAFACTOR_KEYS)} (the learning rate "
                         "comes from LR_CUSTOM_CURVE)")
    kw = {k: hp[k] for k in _ADAFACTOR_KEYS[:9] if k in hp and (hp[k] is not None or k == "beta1")}
    try:
        for k in ("clip_threshold", "decay_rate", "weight_decay"):
            if k in kw:
                kw[k] = float(kw[k])
        if kw.get("beta1") is not None:
            kw["beta1"] = float(kw["beta1"])
        if "eps" in kw:
            kw["eps"] = tuple(float(e) for e in kw["eps"])
            if len(kw["eps"]) != 2:
                raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"ADAFACTOR_PARAMS: a numeric option cannot be read as a number (eps: two numbers): {hp}") from None
    for k in ("scale_parameter", "relative_step", "warmup_init", "stochastic_rounding"):
        if k in kw:
            kw[k] = _as_bool(kw[k])
    check_options(kw.get("eps", (1e-30, 1e-3)), kw.get("clip_threshold", 1.0), kw.get("decay_rate", -0.8), kw.get("beta1"),
                  kw.get("weight_decay", 0.0), kw.get("scale_parameter", False), kw.get("relative_step", False), kw.get("warmup_init", False))
    kw["sr_seed"] = int(getattr(config, "SEED", 0) or 0)
    return kw


def train(config, unet=None, device="cuda:0", reporter: Optional[Reporter] = None, num_workers: Optional[int] = None):
    """Run config.MAX_TRAIN_STEPS micro-steps.  Returns dict(losses, grad_norms, lrs, micro_step, optimizer_step, saved).

    Data parallel: when torch.distributed is initialised (one process per GPU, backend nccl = RCCL), config.BATCH_SIZE
    stays the GLOBAL micro-batch: every rank builds the same schedule / tickets / noise and takes rows [r*b, (r+1)*b);
    the optimizer is dist.ShardedRaven (reduce-scatter -> clip -> sharded Raven -> all-gather, overlapped with the step);
    rank 0 reports and writes the model, every rank writes its own optimizer-state shard."""
    import torch.distributed as tdist
    dp = tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1
    world, rank = (tdist.get_world_size(), tdist.get_rank()) if dp else (1, 0)
    kind = str(getattr(config, "OPTIMIZER_TYPE", "raven")).lower()
    eightbit = kind == "paged_adamw_8bit"
    if eightbit and dp:
        raise ValueError(_ADAMW8_DP_REFUSAL)
    # OPTIMIZER_TYPE "prodigy" (optimizers.Prodigy; not in the reference): its options are read, and what it does not combine with
    # refused, before anything is allocated
    prodigy = kind == "prodigy"
    prodigy_kw = prodigy_options(config, world) if prodigy else None
    # OPTIMIZER_TYPE "adafactor" (optimizers.Adafactor; not in the reference): likewise
    adafactor = kind == "adafactor"
    adafactor_kw = adafactor_options(config, world) if adafactor else None
    # "ema_decay" [, "ema_warmup"] in the ACTIVE optimizer's dictionary: an fp32 EMA of the trainable weights (ema.py; not in the
    # reference, absent = off).  Read first: an invalid value is refused before anything is allocated.
    ema_decay, ema_warmup = _ema_options(getattr(config, _PARAMS_KEY.get(kind, "RAVEN_PARAMS"), None))
    # LORA_PARAMS (lora.options; not in the reference, absent or {} = off): rank-r adapters on the attention projections ("scope":
    # "attention", the default), on every Linear of every Transformer2DModel ("transformer"), or on those and conv1 / conv2 /
    # conv_shortcut of every ResnetBlock2D ("unet", with "conv_rank" / "conv_alpha" for the 3x3 ones), the base frozen.
    # Read, and what it does not combine with refused, before a UNet is loaded.
    lora_spec, lora_merged = lora_mod.options(config, world, ema_decay, unet.cfg if unet is not None else None)
    if unet is not None and getattr(unet, "lora", None) != lora_spec:
        raise ValueError(f"the UNet passed in was built with lora={getattr(unet, 'lora', None)!r} but LORA_PARAMS gives {lora_spec!r}: "
                         "build it with the matching spec (lora.load_unet)")
    master = _master_option(config)          # "master_weights" (not in the reference, absent = off); refusals before anything is allocated
    # "param_groups" in the active optimizer's dictionary (param_groups.py; not in the reference's trainer, absent or [] = off): the rules
    # are read, and what they do not combine with refused, before anything is allocated.  Like LOSS_TYPE they go into nothing that is
    # saved: a resumed run reads them from the preset again.
    group_rules = [] if (prodigy or adafactor) else pgroups.option(config)
    GA = int(config.GRADIENT_ACCUMULATION_STEPS)
    mode = getattr(config, "PREDICTION_TYPE", "epsilon")
    # LOSS_TYPE (loss.parse_loss_type; the reference's GUI offers "MSE" only): read before anything is allocated.  It goes into nothing
    # that is saved: a resumed run reads it from the preset again.
    loss_spec = parse_loss_type(getattr(config, "LOSS_TYPE", "MSE"), mode)
    # NOISE_MODE (noise.parse_noise_mode; the reference carries "normal" and never reads it): likewise read before the model is loaded,
    # refused when it cannot be read, and saved nowhere -- its draws depend on (SEED, micro_step) alone (noise.draw_aux).
    noise_spec = parse_noise_mode(getattr(config, "NOISE_MODE", "normal"))
    config.is_rectified_flow = (mode == "rectified_flow")
    micro_step = optimizer_step = 0
    model_to_load = Path(config.SINGLE_FILE_CHECKPOINT_PATH)
    sampler_seed, optimizer_state, ts_state = config.SEED, None, None
    ema_saved = master_saved = lora_resume = None
    if getattr(config, "RESUME_TRAINING", False):                                   # train.py:2558-2573
        rs = ckpt.load_training_state(config.RESUME_STATE_PATH, GA)
        micro_step, optimizer_step = rs["micro_step"], rs["optimizer_step"]
        sampler_seed, ts_state, optimizer_state = rs["sampler_seed"], rs["timestep_sampler_state"], rs["optimizer_state"]
        if lora_spec is None:
            model_to_load = Path(config.RESUME_MODEL_PATH)
        else:       # RESUME_MODEL_PATH holds the adapters alone; the base comes from (and saves merge into) SINGLE_FILE_CHECKPOINT_PATH
            lora_resume = Path(config.RESUME_MODEL_PATH)
        ema_saved, master_saved = rs["raw"].get("ema_state"), rs["raw"].get("master_state")
        ckpt.restore_rng(rs["raw"])
    if unet is None:
        unet = (ckpt.load_unet(model_to_load, device) if lora_spec is None else
                lora_mod.load_unet(model_to_load, device, None, lora_spec, config.SEED, lora_resume))
    names = [n for n, _ in unet.named_parameters()]
    excl = getattr(config, "UNET_EXCLUDE_TARGETS", []) or []
    if isinstance(excl, str):                                                        # "a, b" -> ["a", "b"] (train.py:304-307)
        excl = [k.strip() for k in excl.split(",") if k.strip()]
    lora_drop = lora_spec is not None and lora_spec.has_dropout
    if lora_spec is not None:        # the whole base frozen, every adapter trainable: one contiguous range of the flat buffers
        adapter_names = set(unet.lora_state_dict())          # A, B and, under DoRA, the magnitudes
        for n, p in unet.named_parameters():
            p.requires_grad = n in adapter_names
        if lora_drop:                # the masks are a function of (SEED, global micro-step): nothing of them goes into a training state
            unet.set_lora_dropout_seed(config.SEED)
        if rank == 0:
            n_ad = sum(p.numel() for n, p in unet.named_parameters() if n in adapter_names)
            drops = (f", dropout {lora_spec.dropout:g} / rank_dropout {lora_spec.rank_dropout:g} / module_dropout {lora_spec.module_dropout:g}"
                     if lora_drop else "")
            n_conv = sum(n.endswith(".lora_A.weight") and p.dim() == 4 for n, p in unet.named_parameters())
            n_lin = sum(n.endswith(".lora_A.weight") for n in adapter_names) - n_conv
            convs = f" and {n_conv} adapted 3x3 convolutions at conv_rank {lora_spec.conv3_rank}, conv_alpha {lora_spec.conv3_alpha:g}" if n_conv else ""
            print(f"INFO: LoRA is ON (rank {lora_spec.rank}, alpha {lora_spec.alpha:g}, scope {lora_spec.scope}{drops}, {n_lin} adapted linears{convs}, {n_ad} "
                  f"trainable elements{', merged model saved too' if lora_merged else ''}): an option outside the reference; the base is frozen, "
                  "UNET_EXCLUDE_TARGETS is not applied, and every model file holds the adapters alone (kohya-ss layout)")
    else:
        for (n, p), m in zip(unet.named_parameters(), trainable_mask(names, [k for k in excl if k])):
            p.requires_grad = m                                                      # train.py:2664-2667
    params = [p for p in unet.parameters() if p.requires_grad]
    # the rules against the trainable parameters (a rule that matches none is refused: a typo must not silently train the default)
    groups = None
    if group_rules:
        hp_g = dict(getattr(config, {"titan": "TITAN_PARAMS", "paged_adamw_8bit": "PAGED_ADAMW_8BIT_PARAMS"}.get(kind, "RAVEN_PARAMS"), None) or {})
        groups = pgroups.resolve_unet(unet, group_rules, hp_g.get("weight_decay", (_ADAMW8_DEFAULTS if eightbit else _RAVEN_DEFAULTS)["weight_decay"]))
    # the step object first: it creates the data-gradient stream, and the order in which a process creates its streams decides
    # which hardware queues they share (streams.py); the optimizer's copy / exchange streams come after it, as in bench.py
    loss_curve = fold_min_snr(timestep_loss_curve_from_config(config, 1000), loss_spec, mode)
    step = TrainStep(unet, mode=mode, grad_accum=GA, world_size=world, loss_curve=loss_curve, use_graph=False, loss=loss_spec, noise=noise_spec)
    if rank == 0 and (loss_spec.kind != "mse" or loss_spec.min_snr_gamma is not None):
        print(f"INFO: LOSS_TYPE: {loss_spec.describe()}: an option outside the reference; the reported loss is this loss, not the squared error.  "
              "(A LOSS_TYPE this build cannot read used to train MSE without a word and is now refused.)")
    if rank == 0 and noise_spec.needs_aux:
        print(f"INFO: NOISE_MODE: {noise_spec.describe()}: an option outside the reference, shaped in HIP between the staged inputs and the UNet forward.")
    from .dist import ShardedRaven, ShardedTitan
    titan = kind == "titan"
    # Single-GPU Titan: the device-accumulator form (dist.ShardedTitan in a group of one: fp32 gradient accumulator in HBM, the same
    # arithmetic -- titan.py:119-131, 162-184, 230-296 -- tests/test_fullsize_gpu.py cfg5) unless the preset asks for the reference's
    # residency with TITAN_HOST_GRADIENTS = true (optimizers.TitanAdamW: fp32 gradients in pinned HOST memory, 10.3 GB written over the
    # host link after every micro-step).  Measured at 1024^2, B = 4 x GA 8 (bench.py other_configs, round 5): 2 991 ms per iteration
    # with host gradients against 957 ms -- the host buffer exists for 12 GB cards, this one has 288 GB.
    host_titan = titan and not dp and bool(getattr(config, "TITAN_HOST_GRADIENTS", False))
    if eightbit:
        # one rank, the module-optimizer branch of the loop: expose_grads -> clip_grad_norm_ -> step (blockwise 8-bit AdamW in HIP)
        optimizer = _optimizer_8bit(config, params, groups)
    elif prodigy:
        # likewise: expose_grads -> clip_grad_norm_ -> step (two fused passes and two scalar kernels in HIP, d never leaves the device)
        curve0 = getattr(config, "LR_CUSTOM_CURVE", [])
        lr0 = max(p_[1] for p_ in curve0) if curve0 else config.LEARNING_RATE
        optimizer = Prodigy(params, lr=lr0, **prodigy_kw)
        if rank == 0:
            shown = {k: v for k, v in optimizer.param_groups[0].items() if k not in ("params", "lr")}
            print(f"INFO: OPTIMIZER_TYPE prodigy is ON ({shown}; {optimizer.state_bytes} bytes of fp32 state: master, starting point, m, v, s): "
                  "an optimizer outside the reference; its step size d is estimated on the device, the learning rate multiplies it")
            if lr0 < 1e-2:
                print(f"INFO: prodigy: the largest learning rate of LR_CUSTOM_CURVE is {lr0:g}.  Prodigy's learning rate is a MULTIPLIER of its own "
                      "step-size estimate and belongs near 1 (a warm-up to 1.0 and a decay); the reference's AdamW-scale curve of 8e-7 would train nothing")
    elif adafactor:
        # likewise: expose_grads -> clip_grad_norm_ -> step (five launches from one descriptor table in HIP, nothing read back)
        curve0 = getattr(config, "LR_CUSTOM_CURVE", [])
        lr0 = max(p_[1] for p_ in curve0) if curve0 else config.LEARNING_RATE
        optimizer = Adafactor(params, lr=lr0, **adafactor_kw)
        if rank == 0:
            shown = {k: v for k, v in optimizer.param_groups[0].items() if k not in ("params", "lr")}
            print(f"INFO: OPTIMIZER_TYPE adafactor is ON ({shown}; {optimizer.state_bytes} bytes of fp32 state: row and column second moments, "
                  f"full ones for vectors{', exp_avg' if adafactor_kw.get('beta1') is not None else ''}): an optimizer outside the reference; "
                  "arithmetic of transformers.optimization.Adafactor, pinned by tests/golden/adafactor_golden.pt")
            if adafactor_kw.get("relative_step"):
                print("INFO: adafactor: relative_step is ON: the step size is min(1e-2 or 1e-6 * step, 1 / sqrt(step)) of the optimizer step, "
                      "LR_CUSTOM_CURVE is ignored by the update and the reported learning rate is the curve's")
            elif not adafactor_kw.get("stochastic_rounding") and lr0 < 1e-4:
                print(f"INFO: adafactor: the largest learning rate of LR_CUSTOM_CURVE is {lr0:g} and stochastic_rounding is off.  Adafactor's "
                      "update is at most about lr per element; half a bf16 spacing of a 0.02-sized weight is 6e-5, so with round-to-nearest "
                      "the parameters do not move at all -- set \"stochastic_rounding\": true in ADAFACTOR_PARAMS")
    elif not host_titan:
        # The flat fused optimizer (one rank: no collectives): m / v resident in HBM (or, RAVEN_STATE_ON_HOST, prefetched under the
        # window's last micro-step and written back under the next window), update of the whole flat range in one launch per
        # contiguous trainable range -- the same arithmetic as optimizers.RavenAdamW (which remains the drop-in class for foreign
        # loops and keeps the reference's host residency), without its 0.2 s of exposed host-link time per optimizer step.
        hp = {**_RAVEN_DEFAULTS, **dict(getattr(config, "TITAN_PARAMS" if titan else "RAVEN_PARAMS", {}) or {})}
        curve0 = getattr(config, "LR_CUSTOM_CURVE", [])
        optimizer = (ShardedTitan if titan else ShardedRaven)(
            unet, lr=max(p_[1] for p_ in curve0) if curve0 else config.LEARNING_RATE, betas=tuple(hp["betas"]), eps=hp["eps"],
            weight_decay=hp["weight_decay"], debias_strength=hp["debias_strength"],
            momentum_dtype=_momentum_dtype(hp.get("momentum_dtype", "bfloat16")), clip_grad_norm=float(config.CLIP_GRAD_NORM),
            force_local=not dp,
            # m / v stay resident in HBM (10.3 GB of 288) unless the preset asks for the reference's residency -- pinned host memory,
            # streamed over the host link every optimizer step (raven.py:83-84, 114-117) -- with RAVEN_STATE_ON_HOST = true
            state_on_host=bool(getattr(config, "RAVEN_STATE_ON_HOST", False)), **_sr_args(config, hp),
            ema=dict(decay=ema_decay, warmup=ema_warmup) if ema_decay is not None else None, **(dict(master_weights=True) if master else {}),
            **(dict(groups=groups) if groups is not None else {}))
    else:
        optimizer = _optimizer(config, params)
    if rank == 0 and getattr(optimizer, "sr", getattr(optimizer, "_sr", False)):
        print(f"INFO: stochastic rounding of the bf16 parameter update is ON (seed {int(getattr(config, 'SEED', 0) or 0)}): an option outside "
              "the reference; results differ from the default round-to-nearest write-back")
    flat_opt = isinstance(optimizer, ShardedRaven)
    if rank == 0 and groups is not None:
        print(f"INFO: parameter groups are ON ({len(groups.groups)} group(s), {len(groups.seg_end)} segment(s) of the flat buffer, one update "
              "launch per contiguous range as without them): an option outside the reference; the reported learning rate is the curve's, unscaled")
        for line in pgroups.describe(groups):
            print(f"INFO: {line}: an option outside the reference")
    if rank == 0 and master:
        print(f"INFO: fp32 master weights are ON ({optimizer.w_dev.numel() * 4} bytes of fp32 on this rank): an option outside the reference; "
              "results differ from the default bf16-only update from the second optimizer step on")
    # the flat optimizers issue the EMA launches themselves, on the streams that update each range; a module optimizer's step() is
    # followed by ema.update() in the loop
    ema = None if ema_decay is None else (optimizer.ema if flat_opt else EmaWeights(unet, ema_decay, ema_warmup))
    if rank == 0 and ema is not None:
        print(f"INFO: EMA of the trainable weights is ON (decay {ema_decay}, warm-up {'on' if ema_warmup else 'off'}, {ema.nbytes} bytes of fp32 on this "
              "rank): an option outside the reference")
    # LORA_PARAMS "scale_weight_norms" (lora_norm.py; kohya-ss's max-norm regularisation, absent = off: no launch, no buffer): one launch
    # behind every optimizer step's update of the adapters.  The flat optimizers issue it inside step(), on the stream that updated the
    # adapters' region and ahead of its W^T copies; a module optimizer's step() is followed by apply() + mark_params_dirty() in the loop.
    # With an fp32 master (Raven / Titan "master_weights", Prodigy's w always) the master is scaled and the parameter is bf16(master).
    lora_norm = None
    if lora_spec is not None and lora_spec.max_norm is not None:
        from .lora_norm import LoraMaxNorm
        lora_norm = LoraMaxNorm(unet, lora_spec.max_norm, master=optimizer.master_address if (prodigy or (flat_opt and master)) else None)
        if flat_opt:
            optimizer.lora_norm = lora_norm
        if rank == 0:
            print(f"INFO: LoRA max-norm is ON (scale_weight_norms {lora_spec.max_norm:g}, {lora_norm.n} modules in one launch per optimizer step"
                  f"{', fp32 masters scaled with them' if lora_norm.has_master else ''}): an option outside the reference; written from kohya-ss's "
                  "rule as understood, unpinned against the package")
    # LORA_PARAMS "dora" (dora.py; absent = off: no launch, no buffer): the gains of the magnitudes are derived state that the forward reads;
    # one launch behind every optimizer step's update of the adapters, at the place of the max-norm pass.  The magnitudes were set to the
    # row norms when the adapters were drawn (lora.load_unet), ahead of the optimizer: its fp32 masters hold them.
    dora = unet.dora if lora_spec is not None and lora_spec.dora else None
    if dora is not None:
        if flat_opt:
            optimizer.dora = dora
        if rank == 0:
            print(f"INFO: DoRA is ON ({dora.n} magnitude vectors, {dora.g.numel()} elements; their gains are refreshed in one launch per optimizer "
                  "step): an option outside the reference; this project's own contract, unpinned against peft / LyCORIS")
    lr_scheduler = CustomCurveLRScheduler(optimizer, config.LR_CUSTOM_CURVE, config.MAX_TRAIN_STEPS)
    if getattr(config, "RESUME_TRAINING", False):
        if dp:       # every rank resumes its own shard (written next to rank 0's training-state file)
            shard = torch.load(str(config.RESUME_STATE_PATH) + f".rank{rank}", map_location="cpu", weights_only=False)
            ema_saved, master_saved = shard.get("ema_state"), shard.get("master_state")
            ckpt.resume_optimizer(optimizer, shard, lr_scheduler, micro_step)
        else:
            ckpt.resume_optimizer(optimizer, optimizer_state, lr_scheduler, micro_step)
        if ema is not None and ema_saved is not None:
            ema.load_state(ema_saved)
        elif ema is not None and rank == 0:
            print("INFO: the training state holds no EMA (\"ema_state\"): the EMA starts from the loaded parameters with k = 0")
        elif ema_saved is not None and rank == 0:
            print("INFO: the training state holds an EMA (\"ema_state\") but \"ema_decay\" is not set: ignored")
        if master and master_saved is not None:
            optimizer.load_master_state(master_saved)
            if rank == 0:
                print("INFO: fp32 master weights restored from the training state (\"master_state\")")
        elif master and rank == 0:
            print("INFO: the training state holds no fp32 master weights (\"master_state\"): the master starts from the loaded parameters")
        elif master_saved is not None and rank == 0:
            print("INFO: the training state holds fp32 master weights (\"master_state\") but \"master_weights\" is not set: ignored")

    dataset = feed.CachedLatentDataset(config)
    timestep_sampler = TimestepSampler(config)
    if ts_state is not None:
        timestep_sampler.load_state_dict(ts_state)
    elif getattr(config, "RESUME_TRAINING", False) and micro_step > 0:
        timestep_sampler.set_current_step(micro_step)
    schedule = feed.pack_schedule(feed.batch_schedule(dataset, config.MAX_TRAIN_STEPS, config.BATCH_SIZE, sampler_seed, timestep_sampler.ticket_pool,
                                                     timestep_sampler.bin_ranges, bool(getattr(config, "TIMESTEP_FORCE_IMAGE_BIN_SPREAD", False))),
                                  config.BATCH_SIZE)
    sampler = feed.PrecomputedBatchSampler(schedule, sampler_seed, micro_step if getattr(config, "RESUME_TRAINING", False) else 0)
    loader = torch.utils.data.DataLoader(dataset, batch_sampler=sampler, collate_fn=feed.collate,
                                         num_workers=int(getattr(config, "NUM_WORKERS", 0) if num_workers is None else num_workers))
    sigma_table = None if config.is_rectified_flow else (1.0 - ddpm_alphas_cumprod().float()).clamp_min(0.0).sqrt()
    own_reporter = reporter is None
    if reporter is None:
        reporter = Reporter(config.MAX_TRAIN_STEPS, "conv_in") if rank == 0 else _Silent()
    window = deque(maxlen=GA)
    step_times, optim_times = deque(maxlen=50), deque(maxlen=20)
    t_start = t_last = t_last_opt = time.time()
    noise_gen = torch.Generator()
    clip = float(config.CLIP_GRAD_NORM)
    hist = dict(losses=[], grad_norms=[], lrs=[], saved=[])
    if ema is not None:
        hist["saved_ema"] = []
    if prodigy:
        hist["prodigy_d"] = []
    if lora_norm is not None:
        hist.update(lora_keys_scaled=[], lora_avg_key_norm=[], lora_max_key_norm=[])
    # emergency-save flag: the GUI writes PROJECT_ROOT/force_save.flag and runs the trainer with cwd = PROJECT_ROOT
    # (gui.py:5947, 5983; train.py:2550 looks next to itself) -> default = the process' working directory
    flag = Path(getattr(config, "FORCE_SAVE_FLAG", None) or Path.cwd() / "force_save.flag")
    stem = ckpt.output_model_stem(config, config.SINGLE_FILE_CHECKPOINT_PATH)                # train.py:2334-2349, 2517
    if dp:      # the {uuid} part is random: every rank must write under rank 0's stem
        box = [stem]
        tdist.broadcast_object_list(box, src=0)
        stem = config._RESOLVED_OUTPUT_STEM = box[0]
    unet.zero_grad()
    # Per-micro-step loss read-back WITHOUT draining the queue (the reference blocks on loss.item() every micro-step,
    # train.py:2767): the device scalar is copied (after a scalar all-reduce under data parallel) into a pinned slot behind an
    # event and read LAG = 2 micro-steps LATER, when the next two are already queued (the pinned input staging of TrainStep is double
    # buffered to the same depth): a host hiccup of up to two micro-steps -- a slow DataLoader batch, a busy box -- then costs the GPU
    # nothing (with a lag of one, bench.py's trainer leg showed iterations of 955 / 1040 / 988 / 1264 / 1223 ms on a noisy box where
    # the bare loop, which runs two ahead, held 967).  Only the micro-step that closes an accumulation window is read at once (the
    # optimizer step needs the window mean and the gradient norm anyway).  The reported values and their order are unchanged; a
    # progress line appears up to two micro-steps later than in the reference.
    RING, LAG = 4, 2
    loss_dev = torch.zeros(RING, dtype=torch.float32, device=device)
    loss_host = torch.zeros(RING, dtype=torch.float32).pin_memory()
    loss_ev = [None] * RING
    pending = deque()

    def resolve(rec):
        """Read a queued micro-step's loss, book it, print its progress line."""
        k = rec["slot"]
        loss_ev[k].synchronize()
        v = float(loss_host[k]) / world
        hist["losses"].append(v)
        window.append(v)
        rec["timing"]["loss"] = v
        return v

    norm_host = torch.zeros(RING, dtype=torch.float32).pin_memory()

    def finish_window(rec):
        """The micro-step that closed an accumulation window: its loss, the window mean, the gradient norm of the optimizer step
        (read from the pinned slot its copy landed in) -> the reference's diagnostics record (train.py:2771-2800)."""
        resolve(rec)
        c = rec["closing"]
        raw = c["raw"] if c["raw"] is not None else float(norm_host[rec["slot"]])
        hist["grad_norms"].append(raw)
        hist["lrs"].append(c["lr"])
        if c.get("lora_norm_slot") is not None:      # the pass's statistics landed behind an event of their own: no queue is drained for them
            n_scaled, avg_norm, max_key = lora_norm.summary(c["lora_norm_slot"])
            hist["lora_keys_scaled"].append(n_scaled)
            hist["lora_avg_key_norm"].append(avg_norm)
            hist["lora_max_key_norm"].append(max_key)
        diag = dict(optim_step=c["optim_step"], avg_loss=sum(window) / len(window) if window else 0.0, current_lr=c["lr"],
                    raw_grad_norm=raw, clipped_grad_norm=min(raw, clip) if clip > 0 else raw, update_delta=1.0 if raw > 0 else 0.0,
                    optim_step_time=c["optim_step_time"], avg_optim_step_time=c["avg_optim_step_time"])
        window.clear()
        reporter.log_step(rec["micro_step"], timing_data=rec["timing"], diag_data=diag)

    def flush(keep=0):
        while len(pending) > keep:
            rec = pending.popleft()
            if rec.get("closing") is not None:
                finish_window(rec)
                continue
            resolve(rec)
            reporter.log_step(rec["micro_step"], timing_data=rec["timing"], diag_data=None)

    def write_model(path):
        """A model file of this run: the merged single-file checkpoint, or -- LoRA -- the adapters alone (+ `<stem>_merged` on request)."""
        if lora_spec is None:
            ckpt.save_model(path, unet, model_to_load, torch.bfloat16)
            return
        lora_mod.save_lora_file(path, unet, lora_spec)
        if lora_merged:
            ckpt.save_model(Path(path).with_name(Path(path).stem + "_merged.safetensors"), lora_mod.merged_state(unet), model_to_load, torch.bfloat16)

    done = False
    gc_frozen = False
    # The loop's CPU tensor work is a handful of tiny ops per micro-step (noise draw, time ids, collate).  With torch's default of one
    # intra-op thread per core every one of them wakes a 256-thread team on the bench boxes, and the op is as slow as the slowest core --
    # on a busy host that was the trainer leg's 80-200 ms hiccups which the bare step (no CPU tensor op in its loop) never saw.
    # Default cap: 8 threads (HOST_THREADS = 0 or >= the current count leaves torch's setting alone).
    host_threads = int(getattr(config, "HOST_THREADS", 8) or 0)
    prev_threads = torch.get_num_threads()
    if 0 < host_threads < prev_threads:
        torch.set_num_threads(host_threads)
    try:
        while not done:
            n_batches = 0
            for batch in loader:
                n_batches += 1
                if micro_step >= config.MAX_TRAIN_STEPS:
                    done = True
                    break
                if not batch:
                    continue
                GB = batch["latents"].shape[0]                   # global micro-batch (after dropped samples)
                micro_step += 1
                diag = None
                timesteps, first_ticket = timestep_sampler.sample(GB)
                noise = generate_noise(batch["latents"], noise_gen, "cpu", step=micro_step, seed=config.SEED)
                noise_aux = draw_aux(noise_spec, batch["latents"].shape, config.SEED, micro_step)     # None under "normal": nothing drawn
                jitter = None
                if config.is_rectified_flow:
                    jitter = torch.rand(timesteps.shape, dtype=torch.float32, generator=seeded_torch_generator("cpu", config.SEED, micro_step, 0x5D1))
                    sigma = float(((timesteps[0].float() + jitter[0]) / 1000.0).clamp(0.0, 1.0))
                else:
                    sigma = float(sigma_table[int(timesteps[0])])
                wscale = 1.0
                if dp:                                           # this rank's rows of the global draw (ragged batches: shares differ by <= 1)
                    rows = feed.shard_rows(GB, rank, world)
                    batch = feed.shard_batch(batch, rank, world, even=False)
                    timesteps, noise = timesteps[rows], noise[rows]
                    jitter = jitter[rows] if jitter is not None else None
                    noise_aux = noise_aux.rows(rows) if noise_aux is not None else None
                    wscale = (rows.stop - rows.start) * world / GB   # every sample weighs 1/GB, as in the single-process run
                latents = batch["latents"]
                B = latents.shape[0]
                tids = make_time_ids(batch.get("scaled_sizes", batch["original_sizes"]), batch.get("crop_coords", [(0, 0)] * B), batch["target_sizes"])
                last = (micro_step % GA == 0)
                # the m / v upload (182 ms of host link at one rank) starts TWO micro-steps (230 ms) before the optimizer step needs it, as in
                # bench.py; started with the last micro-step only, it was hidden or not depending on how far the host happened to run ahead
                # (iterations of 939 and 995-1071 ms in one bench.py trainer leg)
                if flat_opt and (micro_step - 1) % GA == max(0, GA - 2):
                    optimizer.prefetch()
                if B > 0:
                    # HOST tensors go in as they are: TrainStep stages them through its double-buffered pinned area in ONE asynchronous copy
                    # (train_step._host_inputs_in_one_copy).  A `.to(device)` of a pageable tensor here holds the host until the stream has
                    # reached the copy, i.e. until the PREVIOUS micro-step has finished (cProfile: 115 ms per micro-step inside `.to`) -- the
                    # loop then never runs ahead of the GPU and every hiccup of the host idles it
                    loss = step.micro_step(latents, noise, timesteps, batch["embeds"], batch["pooled"], tids, jitter, after_tail=optimizer.reduce_tail if (dp and last and optimizer.overlap) else None,
                                           weight_scale=wscale, noise_aux=noise_aux, lora_step=micro_step if lora_drop else None)
                    slot = micro_step % RING
                    loss_dev[slot:slot + 1].copy_(loss, non_blocking=True)
                else:                                            # fewer samples than ranks: this rank sits the micro-step out
                    slot = micro_step % RING
                    loss_dev[slot:slot + 1].zero_()
                if isinstance(optimizer, TitanAdamW):
                    optimizer.offload_flat(unet)                     # the flat-path form of Titan's post-accumulate hooks
                elif hasattr(optimizer, "accumulate"):
                    optimizer.accumulate()                           # the same under data parallel: fp32 accumulation (dist.ShardedTitan)
                if dp:                                           # reported loss = global mean: sum_r (b_r/GB) * local mean = sum_r loss_r / world
                    tdist.all_reduce(loss_dev[slot:slot + 1])
                loss_host[slot:slot + 1].copy_(loss_dev[slot:slot + 1], non_blocking=True)
                loss_ev[slot] = torch.cuda.Event()
                loss_ev[slot].record()
                now = time.time()
                step_times.append(now - t_last)
                t_last = now
                pending.append(dict(slot=slot, micro_step=micro_step,
                                    timing=dict(raw_step_time=step_times[-1], elapsed_time=now - t_start,
                                                eta=(config.MAX_TRAIN_STEPS - micro_step) * (sum(step_times) / len(step_times)),
                                                loss=0.0, timestep=str(first_ticket), sigma=sigma)))
                flush(keep=LAG)                                  # the loss of the micro-step LAG back (its copy has long landed)
                lr_scheduler.step(micro_step)
                if micro_step % GA == 0:                                                 # train.py:2771-2800
                    cur = pending[-1]
                    raw = None
                    if flat_opt:
                        # [reduce-scatter,] global norm, clip, flat update [, all-gather]: the norm stays on the device and is read with the
                        # closing micro-step's loss, LAG micro-steps later -- the host does not drain the queue at the window's end either
                        # (it did: ~6 ms of idle GPU per iteration while the next batch was fetched and the first micro-step issued)
                        nrm = optimizer.step()
                        norm_host[cur["slot"]:cur["slot"] + 1].copy_(nrm.reshape(1), non_blocking=True)
                        loss_ev[cur["slot"]] = torch.cuda.Event()
                        loss_ev[cur["slot"]].record()             # behind the loss copy AND the norm copy of this slot
                    elif isinstance(optimizer, TitanAdamW):
                        raw = optimizer.clip_grad_norm(clip if clip > 0 else float("inf"))
                        raw = float(raw.item() if isinstance(raw, torch.Tensor) else raw)
                        optimizer.step()
                    else:
                        unet.expose_grads()
                        raw = float(clip_grad_norm_(unet, clip if clip > 0 else float("inf")).item())
                        optimizer.step()
                    if ema is not None and not flat_opt:
                        ema.update()                              # same stream, right behind the step
                    norm_slot = None
                    if lora_norm is not None:
                        if flat_opt:
                            norm_slot = optimizer.lora_norm_slot  # issued inside step(), behind the update of the adapters' region
                        else:
                            norm_slot = lora_norm.apply()         # same stream, right behind the step; the W^T copies follow the scaled values
                            unet.mark_params_dirty()
                    if dora is not None and not flat_opt:
                        dora.refresh()                            # same stream, right behind the step: the next forward reads the new gains
                    optimizer.zero_grad(set_to_none=True)
                    optimizer_step += 1
                    if prodigy:                     # (this branch has already blocked on the norm's .item())
                        hist["prodigy_d"].append(optimizer.d_value())
                    if not gc_frozen:           # the launch tapes / pools built during the first window are permanent: keep the cyclic
                        gc.collect()            # collector from walking them (tens of thousands of objects) in the middle of later windows
                        gc.freeze()
                        gc_frozen = True
                    now = time.time()
                    optim_times.append(now - t_last_opt)
                    t_last_opt = now
                    lr_now = optimizer.param_groups[-1]["lr"]
                    cur["closing"] = dict(raw=raw, lr=lr_now, optim_step=optimizer_step, optim_step_time=optim_times[-1], lora_norm_slot=norm_slot,
                                          avg_optim_step_time=sum(optim_times) / len(optim_times))
                    every = int(getattr(config, "SAVE_EVERY_N_STEPS", 0) or 0)
                    # rank 0 alone consumes the flag file and tells the others: every rank must take the same branch, because
                    # the save path holds collectives (parameter all-gather wait, barrier)
                    forced = ckpt.consume_force_save_flag(flag) if rank == 0 else False
                    if dp:
                        ft = torch.tensor([1 if forced else 0], dtype=torch.int32, device=device)
                        tdist.broadcast(ft, src=0)
                        forced = bool(int(ft.item()))
                    if (every > 0 and optimizer_step % every == 0) or forced:            # train.py:2805-2815
                        reason = "Emergency checkpoint requested" if forced and not (every > 0 and optimizer_step % every == 0) else "Saving checkpoint"
                        flush()                                  # the progress lines of this window come before the checkpoint's (log order of the reference)
                        reporter.log_message(f"\n--- {reason} at optimizer step {optimizer_step} ---" + (f" (prodigy d = {optimizer.d_value():.6e})" if prodigy else "")
                                             + (f" (lora max-norm: {hist['lora_keys_scaled'][-1]} keys scaled, avg key norm {hist['lora_avg_key_norm'][-1]:.6g}, "
                                                f"max key norm {hist['lora_max_key_norm'][-1]:.6g})" if lora_norm is not None else ""))
                        mname, sname = ckpt.checkpoint_names(stem, optimizer_step)
                        if hasattr(optimizer, "synchronize_params"):
                            optimizer.synchronize_params()      # updates / all-gathers still running under the next forward's slots must have landed
                        # EMA: every rank takes part in the gather (state_dict) and keeps its own fp32 shard; rank 0 writes the file
                        ema_sd = ema.state_dict() if ema is not None else None
                        ema_extra = {"ema_state": ema.save_state()} if ema is not None else None
                        if master:               # this rank's fp32 master shard travels with the training state, like the EMA's
                            ema_extra = {**(ema_extra or {}), "master_state": optimizer.save_master_state()}
                        if dp:
                            Path(config.OUTPUT_DIR).mkdir(parents=True, exist_ok=True)
                            torch.save({**optimizer.save_cpu_state(), **(ema_extra or {})}, str(Path(config.OUTPUT_DIR) / sname) + f".rank{rank}")
                        if rank == 0:
                            write_model(Path(config.OUTPUT_DIR) / mname)
                            if ema is not None:
                                ckpt.save_model(Path(config.OUTPUT_DIR) / ckpt.ema_names(stem, optimizer_step), ema_sd, model_to_load, torch.bfloat16)
                            ckpt.save_training_state(Path(config.OUTPUT_DIR) / sname, optimizer_step, micro_step,
                                                     _NoState() if dp else optimizer, sampler.seed, sampler.epoch, timestep_sampler,
                                                     extra=None if dp else ema_extra)
                        del ema_sd
                        if dp:
                            tdist.barrier()
                        hist["saved"].append((mname, sname))
                        if ema is not None:
                            hist["saved_ema"].append(ckpt.ema_names(stem, optimizer_step))
                    if not flat_opt:
                        flush()                                  # the module-optimizer paths read their norm on the host: nothing left to wait for
            if n_batches == 0:
                break
        flush()
    finally:
        # an exception or KeyboardInterrupt in the loop must not leave the embedding process (bench legs, tests, foreign callers)
        # with the thread cap or a frozen collector generation
        if torch.get_num_threads() != prev_threads:
            torch.set_num_threads(prev_threads)
        if gc_frozen:
            gc.unfreeze()
    reporter.log_message("\nTraining complete.")
    if own_reporter:
        reporter.shutdown()
    # train.py:2832-2836: the final model, whatever SAVE_EVERY_N_STEPS says
    final = Path(config.OUTPUT_DIR) / f"{stem}.safetensors"
    if hasattr(optimizer, "synchronize_params"):
        optimizer.synchronize_params()           # the last step's overlapped update / all-gather must have landed
    ema_sd = ema.state_dict() if ema is not None else None       # (every rank: the gather is a collective)
    if rank == 0:
        write_model(final)
        if ema is not None:
            ckpt.save_model(Path(config.OUTPUT_DIR) / ckpt.ema_names(stem), ema_sd, model_to_load, torch.bfloat16)
        print("All tasks complete. Final model saved.")
    if dp:
        tdist.barrier()
    hist.update(micro_step=micro_step, optimizer_step=optimizer_step, final_model=str(final))
    if ema is not None:
        hist["final_ema_model"] = str(Path(config.OUTPUT_DIR) / ckpt.ema_names(stem))
    return hist


def set_seed(seed):
    """train.py:231-238."""
    import random
    import numpy as np
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    print(f"INFO: Set random seed to {seed}")


def _model_config(argv):
    """--unet-config FILE (JSON of unet_spec.UNetConfig fields): a UNet geometry other than SDXL-base (the test suite's
    reduced-width model); the GUI never passes it.  -> UNetConfig or None"""
    import argparse
    import json
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--unet-config", default=None)
    path = ap.parse_known_args(None if argv is None else list(argv))[0].unet_config
    if not path:
        return None
    from .unet_spec import UNetConfig
    with open(path) as f:
        fields = json.load(f)
    return UNetConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in fields.items()})


def main(argv=None) -> int:
    """Process entry: `python -m aozora_sdxl_training_amd.trainer --config X.json` -- what the GUI spawns for train.py
    (gui.py:5930-5975), here for the native step.  One process per GPU: started by torch.distributed.run (RANK / WORLD_SIZE /
    LOCAL_RANK in the environment) the ranks form an RCCL group and config.BATCH_SIZE is the GLOBAL micro-batch.
    Out of scope, refused with a message instead of being attempted: the Anima DiT mode, offline VAE / text-encoder caching
    (the cache must exist), fp16 mixed precision and paged_adamw_8bit, prodigy or adafactor under data parallel."""
    import os
    import sys
    from .config import TrainingConfig
    config = TrainingConfig(argv)
    if str(config.TRAINING_MODE).lower().startswith("anima"):
        print("ERROR: this build trains the SDXL UNet only; the preset's active mode is Anima DiT.")
        return 2
    if config.MIXED_PRECISION != "bfloat16":
        print(f"ERROR: MIXED_PRECISION={config.MIXED_PRECISION!r}: the HIP step computes in bf16 only.")
        return 2
    try:
        parse_loss_type(getattr(config, "LOSS_TYPE", "MSE"), getattr(config, "PREDICTION_TYPE", "epsilon"))
        noise_spec = parse_noise_mode(getattr(config, "NOISE_MODE", "normal"))
        model_cfg = _model_config(argv)     # --unet-config: the geometry LoRA targets are judged against (None = SDXL-base)
        lora_spec = lora_mod.options(config, int(os.environ.get("WORLD_SIZE", "1")), cfg=model_cfg)[0]
        if str(config.OPTIMIZER_TYPE).lower() == "prodigy":
            prodigy_options(config, int(os.environ.get("WORLD_SIZE", "1")))
        elif str(config.OPTIMIZER_TYPE).lower() == "adafactor":
            adafactor_options(config, int(os.environ.get("WORLD_SIZE", "1")))
        else:
            pgroups.option(config)
    except ValueError as e:
        print(f"ERROR: {e}.")
        return 2
    if str(config.OPTIMIZER_TYPE).lower() not in ("raven", "titan", "paged_adamw_8bit", "prodigy", "adafactor"):
        raise ValueError(f"Unsupported optimizer type: '{config.OPTIMIZER_TYPE}'")          # train.py:2290
    if str(config.OPTIMIZER_TYPE).lower() == "paged_adamw_8bit" and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        print(f"ERROR: {_ADAMW8_DP_REFUSAL}.")
        return 2
    if config.SEED:
        set_seed(config.SEED)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # this rank's CPUs = the NUMA node of its GPU, intra-op threads capped: before the pinned optimizer state is allocated and
    # before torch starts its intra-op pool (affinity.py; one rank: the mask is left alone)
    from .affinity import bind_rank
    placement = bind_rank(local, int(os.environ.get("LOCAL_WORLD_SIZE", world)), max_threads=int(getattr(config, "HOST_THREADS", 8) or 8))
    if world > 1 and int(os.environ.get("RANK", "0")) == 0:
        print(f"INFO: host placement of rank 0: {placement['n_cpus']} CPUs ({placement['cpus']}), {placement['threads']} threads, {placement['how']}")
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    if world > 1:
        import torch.distributed as tdist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        from .streams import host_link_streams
        host_link_streams(device)        # the m / v copy streams take their SDMA engines BEFORE the RCCL communicator exists (streams.py)
        tdist.init_process_group(backend=os.environ.get("AOZORA_DIST_BACKEND", "nccl"), device_id=torch.device(device)
                                 if os.environ.get("AOZORA_DIST_BACKEND", "nccl") == "nccl" else None)
    rank0 = int(os.environ.get("RANK", "0")) == 0
    if rank0:
        if config.RESUME_TRAINING:
            print("\n" + "=" * 50 + "\n--- RESUMING TRAINING SESSION ---\n")
        else:
            print("\n" + "=" * 50 + f"\n--- STARTING {'RECTIFIED FLOW' if config.is_rectified_flow else 'STANDARD SDXL'} TRAINING ---\n" + "=" * 50 + "\n")
        print(f"INFO: Noise type: {noise_spec.describe()}")
    Path(config.OUTPUT_DIR).mkdir(parents=True, exist_ok=True)
    unet = None
    if model_cfg is not None:
        src = config.RESUME_MODEL_PATH if config.RESUME_TRAINING else config.SINGLE_FILE_CHECKPOINT_PATH
        if lora_spec is None:
            unet = ckpt.load_unet(src, device, model_cfg)
        else:
            unet = lora_mod.load_unet(config.SINGLE_FILE_CHECKPOINT_PATH, device, model_cfg, lora_spec, config.SEED,
                                      config.RESUME_MODEL_PATH if config.RESUME_TRAINING else None)
    try:
        train(config, unet=unet, device=device)
    except pgroups.GroupsError as e:         # a rule that matches no trainable parameter is only known once the model is loaded
        print(f"ERROR: {e}.")
        return 2
    finally:
        if world > 1:
            import torch.distributed as tdist
            if tdist.is_initialized():
                tdist.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
