"""Parameter groups: a learning-rate scale and a weight decay per part of the UNet (an option outside the reference's trainer, off by
default -- INTEGRATION.md "Parameter groups").  The reference's optimizers loop over torch param_groups with their own lr / weight_decay
(raven.py:96-105) and its scheduler multiplies the curve by each group's lr_scale (train.py:347-352); here the rules of

    "param_groups": [{"match": "bias, norm", "weight_decay": 0.0}, {"match": ["down_blocks.0.*", "conv_in"], "lr_scale": 0.25}]

in RAVEN_PARAMS / TITAN_PARAMS / PAGED_ADAMW_8BIT_PARAMS become (a) a segment table over the flat parameter buffer for the one-launch
update of the flat optimizers (az_adamw_flat_seg) and (b) the group of every trainable parameter for the 8-bit optimizer's torch groups.
Pure Python, no device: every refusal here is a GroupsError (a ValueError), raised before anything is allocated."""
import fnmatch
import math
from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

ALIGN = 64              # elements: a slot of the flat buffers is padded to it (params.ALIGN); the padding belongs to its parameter's segment
MAX_GROUPS = 255
_KEYS = ("match", "lr_scale", "weight_decay")
HOST_PATH_REFUSAL = ("param_groups does not combine with {what}: that path streams pinned-host memory through the chunk pipeline, and no "
                     "segmented form of the chunk pipeline exists -- drop one of the two")


class GroupsError(ValueError):
    """A refusal of this option (trainer.main: `ERROR: ...`, exit status 2)."""


class Rule(NamedTuple):
    keywords: Tuple[str, ...]
    lr_scale: float
    weight_decay: float


class Resolved(NamedTuple):
    seg_end: List[int]                     # ascending exclusive ends in flat-buffer elements; the last one is flat_numel
    seg_gid: List[int]                     # group of each segment
    groups: List[Tuple[float, float]]      # (lr_scale, weight_decay) per group; group 0 is the base
    param_gid: Dict[str, int]              # trainable parameter name -> group
    counts: List[Tuple[int, int]]          # (parameters, elements without padding) per group


def _real(rule_no, key, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise GroupsError(f"param_groups[{rule_no}]: {key} must be a number, not {v!r}")
    v = float(v)
    if not math.isfinite(v) or v < 0:
        raise GroupsError(f"param_groups[{rule_no}]: {key} must be finite and >= 0, not {v!r}")
    return v


def parse_rules(spec, base_weight_decay) -> List[Rule]:
    """The value of "param_groups" -> rules; None or [] -> [] (off).  weight_decay defaults to the dictionary's own and is absolute."""
    if spec is None:
        return []
    if not isinstance(spec, (list, tuple)) or not all(isinstance(r, dict) for r in spec):
        raise GroupsError(f"param_groups must be a list of dictionaries {{\"match\": ..., \"lr_scale\": ..., \"weight_decay\": ...}}, not {spec!r}")
    rules = []
    for i, r in enumerate(spec):
        unknown = [k for k in r if k not in _KEYS]
        if unknown:
            raise GroupsError(f"param_groups[{i}]: unknown key(s) {unknown}; a rule has \"match\", \"lr_scale\" and \"weight_decay\" "
                             "(betas, eps and debias_strength stay global)")
        m = r.get("match", [])
        if isinstance(m, str):
            m = [k.strip() for k in m.split(",")]
        if not isinstance(m, (list, tuple)) or not all(isinstance(k, str) for k in m):
            raise GroupsError(f"param_groups[{i}]: \"match\" must be a comma-separated string or a list of keywords, not {r.get('match')!r}")
        kws = tuple(k.strip() for k in m if k.strip())
        if not kws:
            raise GroupsError(f"param_groups[{i}]: \"match\" is missing or empty")
        rules.append(Rule(kws, _real(i, "lr_scale", r.get("lr_scale", 1.0)), _real(i, "weight_decay", r.get("weight_decay", base_weight_decay))))
    return rules


def matches(name: str, keywords: Sequence[str]) -> bool:
    """schedule.trainable_mask's reading of a keyword (train.py:2664-2667)."""
    return any(fnmatch.fnmatch(name, kw if "*" in kw else f"*{kw}*") for kw in keywords)


def option(config) -> List[Rule]:
    """The rules of the ACTIVE optimizer's dictionary, [] when the key is absent or empty; refuses what the option does not combine with."""
    kind = str(getattr(config, "OPTIMIZER_TYPE", "raven")).lower()
    key = {"titan": "TITAN_PARAMS", "paged_adamw_8bit": "PAGED_ADAMW_8BIT_PARAMS"}.get(kind, "RAVEN_PARAMS")
    hp = dict(getattr(config, key, None) or {})
    rules = parse_rules(hp.get("param_groups"), hp.get("weight_decay", 0.01))       # (0.01: the default of all three dictionaries)
    if rules and kind == "titan" and bool(getattr(config, "TITAN_HOST_GRADIENTS", False)):
        raise GroupsError(HOST_PATH_REFUSAL.format(what="TITAN_HOST_GRADIENTS = true"))
    if rules and kind in ("raven", "titan") and bool(getattr(config, "RAVEN_STATE_ON_HOST", False)):
        raise GroupsError(HOST_PATH_REFUSAL.format(what="RAVEN_STATE_ON_HOST = true"))
    return rules


def resolve(slots: Iterable[Tuple[str, int, int]], trainable: Sequence[bool], rules: Sequence[Rule], base_weight_decay: float,
            flat_numel: Optional[int] = None) -> Resolved:
    """slots: (name, flat offset, elements) of every parameter, ascending and disjoint; trainable: one flag per slot.  The first rule
    that matches a trainable parameter decides its group, none: the base group 0; frozen parameters are ignored (their slot joins the
    segment in front of it: it is never inside an updated range).  Rules with equal (lr_scale, weight_decay) share a group."""
    slots = list(slots)
    if len(slots) != len(trainable):
        raise GroupsError("resolve: one trainable flag per slot")
    groups: List[Tuple[float, float]] = [(1.0, float(base_weight_decay))]
    rule_gid = []
    for r in rules:
        key = (r.lr_scale, r.weight_decay)
        if key not in groups:
            groups.append(key)
        rule_gid.append(groups.index(key))
    if len(groups) > MAX_GROUPS:
        raise GroupsError(f"param_groups resolves to {len(groups)} distinct (lr_scale, weight_decay) groups; at most {MAX_GROUPS}")
    used = [False] * len(rules)
    seg_end: List[int] = []
    seg_gid: List[int] = []
    param_gid: Dict[str, int] = {}
    counts = [[0, 0] for _ in groups]
    pos = 0
    for (name, off, n), tr in zip(slots, trainable):
        if off < pos:
            raise GroupsError(f"resolve: slot {name!r} at {off} overlaps the slot in front of it (ends at {pos})")
        gid = seg_gid[-1] if seg_gid else 0
        if tr:
            gid = 0
            for k, r in enumerate(rules):
                if matches(name, r.keywords):
                    gid, used[k] = rule_gid[k], True
                    break
            param_gid[name] = gid
            counts[gid][0] += 1
            counts[gid][1] += n
        pos = off + (n + ALIGN - 1) // ALIGN * ALIGN
        if seg_gid and seg_gid[-1] == gid:
            seg_end[-1] = pos
        else:
            if seg_end and seg_end[-1] < off:          # a gap in front of this slot stays with the segment before it
                seg_end[-1] = off
            seg_end.append(pos)
            seg_gid.append(gid)
    for k, r in enumerate(rules):
        if not used[k] and not any(tr and matches(nm, r.keywords) for (nm, _, _), tr in zip(slots, trainable)):   # (shadowed by an earlier rule: legal)
            raise GroupsError(f"param_groups[{k}] (match {', '.join(r.keywords)!r}) matches no trainable parameter")
    if not seg_end:
        seg_end, seg_gid = [0], [0]
    if flat_numel is not None:
        if flat_numel < seg_end[-1]:
            raise GroupsError("resolve: the slots reach past flat_numel")
        seg_end[-1] = int(flat_numel)
    return Resolved(seg_end, seg_gid, groups, param_gid, [tuple(c) for c in counts])


def resolve_unet(unet, rules: Sequence[Rule], base_weight_decay: float) -> Resolved:
    """resolve() over an AozoraUNet's slot table and its current requires_grad flags."""
    slots = sorted(((name, o, math.prod(st)) for name, (o, st, _) in unet._slots.items()), key=lambda s: s[1])
    params = dict(unet.named_parameters())
    return resolve(slots, [bool(params[name].requires_grad) for name, _, _ in slots], rules, base_weight_decay, unet.flat_numel)


def describe(res: Resolved) -> List[str]:
    """One line per group for the trainer's INFO output."""
    return [f"parameter group {g}{' (base)' if g == 0 else ''}: {c[0]} parameters, {c[1]} elements, lr_scale {s!r}, weight_decay {wd!r}"
            for g, ((s, wd), c) in enumerate(zip(res.groups, res.counts))]


def ghyper_rows(res_groups: Sequence[Tuple[float, float]], lr: float, bc1: float) -> List[List[float]]:
    """[wd_factor, step_size] per group in Python doubles, as the single-group vector is formed (the caller rounds ONCE to fp32):
    lr_g = lr * lr_scale_g; wd_factor = 1 - lr_g * wd_g (1 when wd_g == 0); step_size = lr_g / bc1."""
    rows = []
    for scale, wd in res_groups:
        lr_g = lr * scale
        rows.append([1.0 - lr_g * wd if wd != 0 else 1.0, lr_g / bc1])
    return rows
