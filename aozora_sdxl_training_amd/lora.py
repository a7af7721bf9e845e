"""LoRA training (INTEGRATION.md "LoRA"; not in the reference, whose train.py is full fine-tuning only): the options of
`LORA_PARAMS`, the adapter file in the kohya-ss layout that ComfyUI and A1111 load, the merged model, and the loader.  Host-side
logic only; the arithmetic is az_lora_* (csrc/az_lora.hip), placed by lora_exec.py for AozoraUNet.linear / conv.  "scope" chooses the
linears that may carry an adapter: the attention projections (the default), every Linear of every Transformer2DModel, or those and the convolutions of every
ResnetBlock2D ("unet": conv1 / conv2 at `conv_rank` / `conv_alpha`, kohya-ss conv_dim / conv_alpha; unet_spec.LoraSpec).
"network_dropout", "rank_dropout" and "module_dropout" (kohya-ss's names; INTEGRATION.md "LoRA dropout") are probabilities
in [0, 1), 0 when absent.  "scale_weight_norms" (kohya-ss's name; INTEGRATION.md "LoRA max-norm") is the limit of every module's
|| (alpha / rank) B A ||_F, enforced after every optimizer step by lora_norm.LoraMaxNorm; absent or None = off.  "dora" (INTEGRATION.md
"DoRA"; absent = off) adds a trainable magnitude `<module>.dora_scale` to every adapted linear: `<key>.dora_scale` [out][1] in the file."""
from __future__ import annotations

import json
import math
from pathlib import Path
from typing import Dict, Optional, Tuple

import torch

from . import checkpoint as ckpt
from .unet_spec import LORA_RANKS, LORA_SCOPES, LoraSpec, lora_is_conv3, lora_modules

_KEYS = ("rank", "alpha", "targets", "save_merged", "scope")
_CONV_KEYS = ("conv_rank", "conv_alpha")        # of "scope": "unet"
_DROP_KEYS = ("network_dropout", "rank_dropout", "module_dropout")      # kohya-ss's own names; LoraSpec.dropout, .rank_dropout, .module_dropout
_NORM_KEY = "scale_weight_norms"               # kohya-ss's own name; LoraSpec.max_norm
_DORA_KEY = "dora"                             # LoraSpec.dora; the file says "dora_wd": "True" in ss_network_args (LyCORIS's name, as understood)
DORA_SUFFIX = ".dora_scale"
DP_REFUSAL = ("LORA_PARAMS under data parallel (more than one rank): the flat gradient exchange would move the whole frozen base's "
              "gradient (5 GB at SDXL size) for a few MB of adapters; run LoRA on one GPU")
EMA_REFUSAL = "LORA_PARAMS with \"ema_decay\": the EMA's file writer knows only the full model (EMA of adapters is a follow-up)"


def _as_bool(v) -> bool:
    return v.strip().lower() in ("true", "1", "t", "y", "yes") if isinstance(v, str) else bool(v)


def _probability(hp, key) -> float:
    """A dropout probability of LORA_PARAMS: a number (or a string that reads as one) in [0, 1); absent = 0."""
    v = hp.get(key, 0.0)
    if isinstance(v, (bool, list, tuple, dict)) or v is None:
        raise ValueError(f"LORA_PARAMS: {key} must be one number in [0, 1), got {v!r}")
    try:
        p = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"LORA_PARAMS: {key} cannot be read as a number: {v!r}") from None
    if not (0.0 <= p < 1.0):          # NaN fails both
        raise ValueError(f"LORA_PARAMS: {key} must be >= 0 and < 1, got {v!r}")
    return p


def _max_norm(hp) -> Optional[float]:
    """scale_weight_norms of LORA_PARAMS: a number (or a string that reads as one) > 0 and finite; absent or None = off."""
    v = hp.get(_NORM_KEY)
    if v is None:
        return None
    if isinstance(v, (bool, list, tuple, dict)):
        raise ValueError(f"LORA_PARAMS: {_NORM_KEY} must be one number > 0, got {v!r}")
    try:
        m = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"LORA_PARAMS: {_NORM_KEY} cannot be read as a number: {v!r}") from None
    if not (0.0 < m < math.inf):          # NaN fails both
        raise ValueError(f"LORA_PARAMS: {_NORM_KEY} must be > 0 and finite, got {v!r}")
    return m


def options(config, world: int = 1, ema_decay=None, cfg=None) -> Tuple[Optional[LoraSpec], bool]:
    """config.LORA_PARAMS -> (LoraSpec or None, save_merged).  Absent or {} = off.  Everything that cannot be read or combined is
    refused here (ValueError), before a UNet is loaded."""
    hp = getattr(config, "LORA_PARAMS", None)
    if not hp:
        return None, False
    if not isinstance(hp, dict):
        raise ValueError(f"LORA_PARAMS must be a dictionary, got {type(hp).__name__}")
    known = _KEYS + _CONV_KEYS + _DROP_KEYS + (_NORM_KEY, _DORA_KEY)
    unknown = sorted(k for k in hp if k not in known)
    if unknown:
        raise ValueError(f"LORA_PARAMS holds unknown key(s) {unknown}: this build reads {list(known)}")
    drops = [_probability(hp, k) for k in _DROP_KEYS]
    max_norm = _max_norm(hp)
    rank = hp.get("rank", 16)
    if isinstance(rank, (list, tuple, dict)):
        raise ValueError(f"LORA_PARAMS: one rank for all adapters, got {rank!r} (more than one rank is a follow-up)")
    try:
        rank_i, alpha = int(rank), float(hp.get("alpha", rank))
        if rank_i != float(rank):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"LORA_PARAMS: rank / alpha cannot be read as numbers: {hp}") from None
    if rank_i not in LORA_RANKS:
        raise ValueError(f"LORA_PARAMS: rank {rank_i} is not one of {list(LORA_RANKS)}")
    if not alpha > 0.0:
        raise ValueError(f"LORA_PARAMS: alpha must be > 0, got {alpha}")
    targets = hp.get("targets", "") or ""
    if isinstance(targets, (list, tuple)):
        targets = ", ".join(str(t) for t in targets)
    scope = hp.get("scope", "attention")
    if not isinstance(scope, str) or scope.strip().lower() not in LORA_SCOPES:
        raise ValueError(f"LORA_PARAMS: scope {scope!r} is not one of {list(LORA_SCOPES)}")
    scope = scope.strip().lower()
    conv_rank, conv_alpha = hp.get("conv_rank"), hp.get("conv_alpha")
    if (conv_rank is not None or conv_alpha is not None) and scope != "unet":
        raise ValueError(f"LORA_PARAMS: conv_rank / conv_alpha belong to \"scope\": \"unet\" (scope {scope!r} adapts no convolution)")
    if conv_rank is not None:
        try:
            if isinstance(conv_rank, (list, tuple, dict, bool)) or int(conv_rank) != float(conv_rank):
                raise ValueError
            conv_rank = int(conv_rank)
        except (TypeError, ValueError):
            raise ValueError(f"LORA_PARAMS: conv_rank cannot be read as one whole number: {conv_rank!r}") from None
        if conv_rank not in LORA_RANKS:
            raise ValueError(f"LORA_PARAMS: conv_rank {conv_rank} is not one of {list(LORA_RANKS)}")
    if conv_alpha is not None:
        try:
            if isinstance(conv_alpha, bool):
                raise ValueError
            conv_alpha = float(conv_alpha)
        except (TypeError, ValueError):
            raise ValueError(f"LORA_PARAMS: conv_alpha cannot be read as a number: {conv_alpha!r}") from None
        if not conv_alpha > 0.0:
            raise ValueError(f"LORA_PARAMS: conv_alpha must be > 0, got {conv_alpha}")
    dora = _as_bool(hp.get(_DORA_KEY, False))
    if dora:
        if scope == "unet":
            raise ValueError("LORA_PARAMS: \"dora\" with \"scope\": \"unet\": the norm kernel takes no 3x3 convolution (DoRA on the convolutions is a follow-up)")
        on = [k for k, p in zip(_DROP_KEYS, drops) if p > 0.0]
        if on:
            raise ValueError(f"LORA_PARAMS: \"dora\" with {on[0]}: the gain follows the unmasked up product (DoRA with dropout is a follow-up)")
        if max_norm is not None:
            raise ValueError(f"LORA_PARAMS: \"dora\" with {_NORM_KEY}: scaling A and B changes the row norms behind the gains (DoRA with max-norm is a follow-up)")
    if world > 1:
        raise ValueError(DP_REFUSAL)
    if ema_decay is not None:
        raise ValueError(EMA_REFUSAL)
    if scope == "unet" and conv_rank is None:
        conv_rank = rank_i              # "conv_rank" left out = "rank" (a LoraSpec of scope "unet" names it)
    spec = LoraSpec(rank_i, alpha, str(targets), scope, conv_rank, conv_alpha, *drops, max_norm, dora=dora)
    from .unet_spec import SDXL_BASE
    lora_modules(cfg if cfg is not None else SDXL_BASE, spec)        # a target that selects nothing / something outside the scope
    return spec, _as_bool(hp.get("save_merged", False))


# ---------------- the adapter file ---------------------------------------------------------------------------------------------------
def file_key(module: str) -> str:
    """`lora_unet_<single-file module path with . -> _>`: the module path is checkpoint._sd_name's (the 1680-name pin covers it)."""
    return "lora_unet_" + ckpt._sd_name(module + ".weight")[:-len(".weight")].replace(".", "_")


def _is_conv(module: str) -> bool:
    """A convolution of a ResnetBlock2D: its file tensors are 4-D (the 1x1 conv_shortcut too, with trailing 1 x 1)."""
    return lora_is_conv3(module) or (".resnets." in module and module.endswith(".conv_shortcut"))


def file_tensors(lora_state: Dict[str, torch.Tensor], spec: LoraSpec) -> Dict[str, torch.Tensor]:
    """A linear: lora_down [r][in], lora_up [out][r].  A convolution (kohya-ss): lora_down [r][Cin][kh][kw] -- the logical shape of A,
    a permutation of its device layout [r][kh][kw][Cin] -- and lora_up [Cout][r][1][1].  .alpha is the module's own alpha."""
    out = {}
    for name, t in lora_state.items():
        if name.endswith(DORA_SUFFIX):           # the magnitude [out] as a column [out][1]
            out[file_key(name[:-len(DORA_SUFFIX)]) + DORA_SUFFIX] = t.detach().to("cpu", torch.bfloat16).reshape(-1, 1).contiguous()
            continue
        module, _, leaf = name.rpartition(".lora_")
        key = file_key(module)
        t = t.detach().to("cpu", torch.bfloat16)
        if _is_conv(module) and t.dim() == 2:
            t = t[:, :, None, None]
        out[key + (".lora_down.weight" if leaf == "A.weight" else ".lora_up.weight")] = t.contiguous()
        out[key + ".alpha"] = torch.tensor(spec.alpha_of(module), dtype=torch.bfloat16)
    return out


def file_metadata(spec: LoraSpec) -> Dict[str, str]:
    meta = {"ss_network_module": "networks.lora", "ss_network_dim": str(spec.rank), "ss_network_alpha": f"{float(spec.alpha):g}",
            "ss_base_model_version": "sdxl_base_v1-0"}
    args = {}
    if spec.scope == "unet":
        args.update({"conv_dim": str(spec.conv3_rank), "conv_alpha": f"{spec.conv3_alpha:g}"})
    # kohya-ss: network_dropout has a key of its own, rank_dropout / module_dropout are network arguments (strings)
    if spec.dropout > 0:
        meta["ss_network_dropout"] = f"{float(spec.dropout):g}"
    if spec.rank_dropout > 0:
        args["rank_dropout"] = f"{float(spec.rank_dropout):g}"
    if spec.module_dropout > 0:
        args["module_dropout"] = f"{float(spec.module_dropout):g}"
    if spec.max_norm is not None:      # kohya-ss: a key of its own
        meta["ss_scale_weight_norms"] = str(float(spec.max_norm))
    if spec.dora:
        args["dora_wd"] = "True"
    if args:
        meta["ss_network_args"] = json.dumps(args)
    return meta


def save_lora_file(path, unet, spec: Optional[LoraSpec] = None):
    """Write ONLY the adapters: <key>.lora_down.weight [r][in], .lora_up.weight [out][r] (convolutions: file_tensors), .alpha (0-dim), bf16."""
    from safetensors.torch import save_file
    spec = spec if spec is not None else unet.lora
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    save_file(file_tensors(unet.lora_state_dict(), spec), str(path), metadata=file_metadata(spec))
    return path


def read_lora_file(path, unet) -> Dict[str, torch.Tensor]:
    """-> {<module>.lora_A.weight / .lora_B.weight: tensor} for unet.load_lora_state_dict; the file must hold exactly this UNet's
    adapters at its rank and alpha."""
    from safetensors import safe_open
    spec = unet.lora
    out = {}
    with safe_open(str(path), framework="pt", device="cpu") as f:
        keys = set(f.keys())
        meta = f.metadata() or {}
        if meta.get("ss_network_dim") not in (None, str(spec.rank)):
            raise ValueError(f"{Path(path).name} holds rank {meta.get('ss_network_dim')} adapters; LORA_PARAMS asks for rank {spec.rank}")
        state = unet.lora_state_dict()
        want = set()
        for name in state:
            if name.endswith(DORA_SUFFIX):
                want.add(file_key(name[:-len(DORA_SUFFIX)]) + DORA_SUFFIX)
                continue
            module = name.rpartition(".lora_")[0]
            want.update((file_key(module) + (".lora_down.weight" if name.endswith("A.weight") else ".lora_up.weight"), file_key(module) + ".alpha"))
        # keys the scope does not carry (a file with adapters on emb_layers, op, conv ... of a wider network): named, not dropped
        extra = sorted(keys - want)
        if extra:
            raise KeyError(f"{Path(path).name} holds adapters this LoraSpec does not, the first of them {extra[0]} ({len(extra)} keys in all)")
        for name, mine in state.items():
            if name.endswith(DORA_SUFFIX):
                k = file_key(name[:-len(DORA_SUFFIX)]) + DORA_SUFFIX
                if k not in keys:
                    raise KeyError(f"{k} is missing from {Path(path).name} (this LoraSpec has \"dora\"; a plain LoRA file holds no magnitudes)")
                t = f.get_tensor(k)
                if tuple(t.shape) != (mine.numel(), 1):
                    raise ValueError(f"{Path(path).name}: {k} has shape {tuple(t.shape)}; this LoraSpec gives {(mine.numel(), 1)}")
                out[name] = t.reshape(tuple(mine.shape))
                continue
            module, _, leaf = name.rpartition(".lora_")
            k = file_key(module) + (".lora_down.weight" if leaf == "A.weight" else ".lora_up.weight")
            if k not in keys:
                raise KeyError(f"{k} is missing from {Path(path).name}")
            t = f.get_tensor(k)
            if t.numel() != mine.numel() or tuple(t.shape[:2]) != tuple(mine.shape[:2]):
                raise ValueError(f"{Path(path).name}: {k} has shape {tuple(t.shape)}; this LoraSpec gives {module} {tuple(mine.shape)}")
            out[name] = t.reshape(tuple(mine.shape))       # a convolution's up matrix and conv_shortcut carry a trailing 1 x 1 in the file
            a = float(f.get_tensor(file_key(module) + ".alpha"))
            if a != float(torch.tensor(spec.alpha_of(module), dtype=torch.bfloat16)):
                raise ValueError(f"{Path(path).name}: alpha {a} of {module} differs from LORA_PARAMS' {spec.alpha_of(module)}")
    return out


def merged_state(unet) -> Dict[str, torch.Tensor]:
    """The base state dict with W + s B A in place of every adapted weight -- a 3x3 convolution: W[o][c][kh][kw] + s sum_j B[o][j]
    A[j][c][kh][kw] -- formed in fp32 on the CPU, rounded once (by save_model).  s is the module's own alpha / rank.  Under DoRA row o
    of the sum is scaled by m[o] / || row o || (the norm in fp32 from the same fp32 sum)."""
    return merge_into({k: v.detach().cpu() for k, v in unet.state_dict().items()},
                      {k: v.detach().float().cpu() for k, v in unet.lora_state_dict().items()}, unet.lora)


def merge_into(sd: Dict[str, torch.Tensor], ls: Dict[str, torch.Tensor], spec: LoraSpec) -> Dict[str, torch.Tensor]:
    for name, A in ls.items():
        if name.endswith(".lora_A.weight"):
            module = name[:-len(".lora_A.weight")]
            W, B = sd[module + ".weight"].float(), ls[module + ".lora_B.weight"].float()
            delta = (B @ A.float().reshape(A.shape[0], -1)).reshape(W.shape)      # [o][j] x [j][c kh kw]: the logical order of both
            merged = W + spec.scale_of(module) * delta
            m = ls.get(module + DORA_SUFFIX)
            if m is not None:
                merged = (m.float() / merged.reshape(merged.shape[0], -1).norm(dim=1)).reshape(-1, *([1] * (merged.dim() - 1))) * merged
            sd[module + ".weight"] = merged
    return sd


def load_unet(base_path, device, cfg, spec: LoraSpec, seed: int, adapters_path=None):
    """The base out of a single-file checkpoint into AozoraUNet(lora=spec); adapters from `adapters_path` (resume) or freshly drawn."""
    from .unet import AozoraUNet
    from .unet_spec import SDXL_BASE
    cfg = cfg if cfg is not None else SDXL_BASE
    cin, cout = ckpt.peek_channels(base_path)
    if (cin, cout) != (cfg.in_channels, cfg.out_channels):
        raise ValueError(f"checkpoint has in/out channels {cin}/{cout}; this build runs {cfg.in_channels}/{cfg.out_channels}")
    unet = AozoraUNet(cfg, device, lora=spec)
    unet.set_lora_dropout_seed(seed)          # the dropout masks follow SEED (nothing recorded yet: no cost)
    unet.load_state_dict(ckpt.read_unet_state(base_path, list(unet.state_dict())))
    if adapters_path is not None:
        unet.load_lora_state_dict(read_lora_file(adapters_path, unet))
    else:
        unet.init_lora(seed)
    return unet
