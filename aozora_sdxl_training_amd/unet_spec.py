"""Structure of the SDXL-base UNet as the product sees it: configuration, diffusers parameter
names/shapes in diffusers' named_parameters() order (train.py:2665 iterates them for the freeze
keywords; raven.py:157-168 indexes optimizer state by position in that order), and the skip-stack
channel bookkeeping.  Structural pins: train.py:2418-2447 (key map), 2,567,463,684 params / 1680
tensors.  diffusers itself is not importable here: PARITY UNPINNED."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple


@dataclass
class UNetConfig:
    in_channels: int = 4
    out_channels: int = 4
    block_out_channels: Tuple[int, ...] = (320, 640, 1280)
    transformer_layers: Tuple[int, ...] = (0, 2, 10)
    layers_per_block: int = 2
    head_dim: int = 64
    cross_attention_dim: int = 2048
    addition_time_embed_dim: int = 256
    pooled_dim: int = 1280
    norm_groups: int = 32
    time_embed_dim: int = 0

    def __post_init__(self):
        if self.time_embed_dim == 0:
            self.time_embed_dim = 4 * self.block_out_channels[0]

    @property
    def add_in_dim(self) -> int:
        return self.pooled_dim + 6 * self.addition_time_embed_dim


SDXL_BASE = UNetConfig()


def mini_config(c0=64, layers=(0, 1, 2), ctx_dim=128, pooled=64, add_dim=32, groups=8) -> UNetConfig:
    """SDXL topology at small width (head_dim stays 64: the attention kernel is specialised for it)."""
    return UNetConfig(block_out_channels=(c0, 2 * c0, 4 * c0), transformer_layers=tuple(layers), head_dim=64,
                      cross_attention_dim=ctx_dim, addition_time_embed_dim=add_dim, pooled_dim=pooled, norm_groups=groups)


def skip_channels(cfg: UNetConfig) -> List[int]:
    ch = cfg.block_out_channels
    s = [ch[0]]
    for i in range(len(ch)):
        s += [ch[i]] * cfg.layers_per_block
        if i < len(ch) - 1:
            s.append(ch[i])
    return s


def up_resnet_channels(cfg: UNetConfig):
    ch = cfg.block_out_channels
    skips = skip_channels(cfg)
    out, prev = [], ch[-1]
    for i in range(len(ch)):
        cout = ch[len(ch) - 1 - i]
        blk = []
        for _ in range(cfg.layers_per_block + 1):
            s = skips.pop()
            blk.append((prev, s, cout))   # (hidden channels, skip channels, out channels)
            prev = cout
        out.append(blk)
    return out


def _resnet(pre, cin, cout, T):
    p = [(f"{pre}.norm1.weight", (cin,)), (f"{pre}.norm1.bias", (cin,)),
         (f"{pre}.conv1.weight", (cout, cin, 3, 3)), (f"{pre}.conv1.bias", (cout,)),
         (f"{pre}.time_emb_proj.weight", (cout, T)), (f"{pre}.time_emb_proj.bias", (cout,)),
         (f"{pre}.norm2.weight", (cout,)), (f"{pre}.norm2.bias", (cout,)),
         (f"{pre}.conv2.weight", (cout, cout, 3, 3)), (f"{pre}.conv2.bias", (cout,))]
    if cin != cout:
        p += [(f"{pre}.conv_shortcut.weight", (cout, cin, 1, 1)), (f"{pre}.conv_shortcut.bias", (cout,))]
    return p


def _transformer(pre, c, n, ctx):
    p = [(f"{pre}.norm.weight", (c,)), (f"{pre}.norm.bias", (c,)), (f"{pre}.proj_in.weight", (c, c)), (f"{pre}.proj_in.bias", (c,))]
    for i in range(n):
        b = f"{pre}.transformer_blocks.{i}"
        p += [(f"{b}.norm1.weight", (c,)), (f"{b}.norm1.bias", (c,)),
              (f"{b}.attn1.to_q.weight", (c, c)), (f"{b}.attn1.to_k.weight", (c, c)), (f"{b}.attn1.to_v.weight", (c, c)),
              (f"{b}.attn1.to_out.0.weight", (c, c)), (f"{b}.attn1.to_out.0.bias", (c,)),
              (f"{b}.norm2.weight", (c,)), (f"{b}.norm2.bias", (c,)),
              (f"{b}.attn2.to_q.weight", (c, c)), (f"{b}.attn2.to_k.weight", (c, ctx)), (f"{b}.attn2.to_v.weight", (c, ctx)),
              (f"{b}.attn2.to_out.0.weight", (c, c)), (f"{b}.attn2.to_out.0.bias", (c,)),
              (f"{b}.norm3.weight", (c,)), (f"{b}.norm3.bias", (c,)),
              (f"{b}.ff.net.0.proj.weight", (8 * c, c)), (f"{b}.ff.net.0.proj.bias", (8 * c,)),
              (f"{b}.ff.net.2.weight", (c, 4 * c)), (f"{b}.ff.net.2.bias", (c,))]
    p += [(f"{pre}.proj_out.weight", (c, c)), (f"{pre}.proj_out.bias", (c,))]
    return p


def param_table(cfg: UNetConfig = SDXL_BASE):
    """[(diffusers name, logical shape)] in diffusers registration order: conv_in, time_embedding,
    add_embedding, down_blocks, up_blocks, mid_block, conv_norm_out, conv_out; cross-attention blocks list
    `attentions` before `resnets`."""
    ch, T, n = cfg.block_out_channels, cfg.time_embed_dim, len(cfg.block_out_channels)
    p = [("conv_in.weight", (ch[0], cfg.in_channels, 3, 3)), ("conv_in.bias", (ch[0],)),
         ("time_embedding.linear_1.weight", (T, ch[0])), ("time_embedding.linear_1.bias", (T,)),
         ("time_embedding.linear_2.weight", (T, T)), ("time_embedding.linear_2.bias", (T,)),
         ("add_embedding.linear_1.weight", (T, cfg.add_in_dim)), ("add_embedding.linear_1.bias", (T,)),
         ("add_embedding.linear_2.weight", (T, T)), ("add_embedding.linear_2.bias", (T,))]
    prev = ch[0]
    for i in range(n):
        pre, c, nl = f"down_blocks.{i}", ch[i], cfg.transformer_layers[i]
        if nl:
            for j in range(cfg.layers_per_block):
                p += _transformer(f"{pre}.attentions.{j}", c, nl, cfg.cross_attention_dim)
        for j in range(cfg.layers_per_block):
            p += _resnet(f"{pre}.resnets.{j}", prev if j == 0 else c, c, T)
        if i < n - 1:
            p += [(f"{pre}.downsamplers.0.conv.weight", (c, c, 3, 3)), (f"{pre}.downsamplers.0.conv.bias", (c,))]
        prev = c
    up = up_resnet_channels(cfg)
    for i in range(n):
        lev = n - 1 - i
        pre, c, nl = f"up_blocks.{i}", ch[lev], cfg.transformer_layers[lev]
        if nl:
            for j in range(cfg.layers_per_block + 1):
                p += _transformer(f"{pre}.attentions.{j}", c, nl, cfg.cross_attention_dim)
        for j in range(cfg.layers_per_block + 1):
            hc, sc, co = up[i][j]
            p += _resnet(f"{pre}.resnets.{j}", hc + sc, co, T)
        if i < n - 1:
            p += [(f"{pre}.upsamplers.0.conv.weight", (c, c, 3, 3)), (f"{pre}.upsamplers.0.conv.bias", (c,))]
    cm = ch[-1]
    p += _transformer("mid_block.attentions.0", cm, cfg.transformer_layers[-1], cfg.cross_attention_dim)
    p += _resnet("mid_block.resnets.0", cm, cm, T) + _resnet("mid_block.resnets.1", cm, cm, T)
    p += [("conv_norm_out.weight", (ch[0],)), ("conv_norm_out.bias", (ch[0],)),
          ("conv_out.weight", (cfg.out_channels, ch[0], 3, 3)), ("conv_out.bias", (cfg.out_channels,))]
    return p


# --------------------------------------------------------------------------------------
# LoRA adapters (INTEGRATION.md "LoRA"): which projections carry one, and their table entries
# --------------------------------------------------------------------------------------
LORA_RANKS = (4, 8, 16, 32, 64)
LORA_PROJECTIONS = ("to_q", "to_k", "to_v", "to_out.0")       # of attn1 and attn2 of every BasicTransformerBlock
LORA_SCOPES = ("attention", "transformer", "unet")
LORA_CONVS = ("conv1", "conv2")                               # the 3x3 convolutions of a ResnetBlock2D: conv_rank / conv_alpha
# convolutions and linears of the UNet that scope "unet" leaves out, and why (lora_modules refuses a keyword that names one)
LORA_UNET_REFUSED = (
    (".time_emb_proj", "its data gradient is produced on the parameter-gradient branch and its forward is hoisted into a grouped launch"),
    (".downsamplers.", "a stride-2 convolution"),
    (".upsamplers.", "it reads its input through the fused nearest-2x gather"),
    ("conv_in", "the input convolution"),
    ("conv_out", "the output convolution"),
)


def lora_is_conv3(module: str) -> bool:
    """A 3x3 convolution of a ResnetBlock2D (conv_rank / conv_alpha govern it; the 1x1 conv_shortcut is a Linear)."""
    return module.rsplit(".", 1)[-1] in LORA_CONVS and ".resnets." in module


def lora_dropout_threshold(p: float) -> int:
    """t = clamp(int(p 65536 + 0.5), 1, 65535) for p > 0, 0 for p = 0: 16 uniform bits >= t keep an element with probability 1 - t / 65536."""
    return 0 if p <= 0.0 else min(65535, max(1, int(p * 65536.0 + 0.5)))


@dataclass(frozen=True)
class LoraSpec:
    """rank-r adapters: y += (alpha / rank) (x A^T) B^T.  scope: which layers may carry one -- "attention" (the default): the eight
    attention projections of every BasicTransformerBlock; "transformer": every Linear of every Transformer2DModel (proj_in, the eight
    projections, ff.net.0.proj, ff.net.2, proj_out: the default of the kohya-ss layout); "unet": those and conv1, conv2 and
    conv_shortcut of every ResnetBlock2D (kohya-ss conv_dim / conv_alpha, LoCon).  conv_rank / conv_alpha: rank and alpha of the 3x3
    convolutions; the 1x1 conv_shortcut takes rank / alpha like a Linear.  Scope "unet" carries its conv_rank explicitly (LORA_PARAMS
    may leave it out: lora.options puts rank there); conv_alpha None = alpha.  targets: comma-separated keywords
    read by the freeze keywords' rule (fnmatch(name, kw if '*' in kw else '*kw*')) against the module names of the scope; '' or
    '*' = all.  dropout / rank_dropout / module_dropout: kohya-ss network, rank and module dropout of the adapters' inner activation, each
    a probability in [0, 1) (INTEGRATION.md "LoRA dropout"); all three 0 (the default) = off, and such a spec equals one built without them.
    max_norm: kohya-ss scale_weight_norms, the limit of every module's || scale B A ||_F (INTEGRATION.md "LoRA max-norm"); None = off.
    dora: weight-decomposed LoRA (INTEGRATION.md "DoRA"): every adapted linear also carries a trainable magnitude `<module>.dora_scale`
    [out]; False (the default) = off, and such a spec equals one built without it.  Not with scope "unet", dropout or max_norm."""
    rank: int = 16
    alpha: float = 16.0
    targets: str = ""
    scope: str = "attention"
    conv_rank: Optional[int] = None
    conv_alpha: Optional[float] = None
    # LoRA dropout (INTEGRATION.md "LoRA dropout"; kohya-ss network_dropout, rank_dropout, module_dropout), each a probability in [0, 1)
    dropout: float = 0.0
    rank_dropout: float = 0.0
    module_dropout: float = 0.0
    # LoRA max-norm (INTEGRATION.md "LoRA max-norm"; kohya-ss scale_weight_norms): the limit of || (alpha / rank) B A ||_F per module,
    # enforced after every optimizer step; None (the default) = off, and such a spec equals one built without it
    max_norm: Optional[float] = None
    # DoRA (INTEGRATION.md "DoRA"; Liu et al., arXiv 2402.09353): a trainable per-output-channel magnitude beside every adapter; False
    # (the default) = off, and such a spec equals one built without it
    dora: bool = False

    def __post_init__(self):
        if self.max_norm is not None:
            m = self.max_norm
            if isinstance(m, bool) or not isinstance(m, (int, float)) or not (0.0 < float(m) < float("inf")):      # NaN fails both
                raise ValueError(f"LoRA max_norm must be a positive finite real number or None, got {m!r}")
        for key in ("dropout", "rank_dropout", "module_dropout"):
            p = getattr(self, key)
            if isinstance(p, bool) or not isinstance(p, (int, float)) or not (0.0 <= float(p) < 1.0):
                raise ValueError(f"LoRA {key} must be a real number in [0, 1), got {p!r}")
        if self.rank not in LORA_RANKS:
            raise ValueError(f"LoRA rank {self.rank!r} is not one of {LORA_RANKS}")
        if not (float(self.alpha) > 0.0):
            raise ValueError(f"LoRA alpha must be > 0, got {self.alpha!r}")
        if self.scope not in LORA_SCOPES:
            raise ValueError(f"LoRA scope {self.scope!r} is not one of {LORA_SCOPES}")
        if self.scope == "unet" and self.conv_rank is None:
            # a LoraSpec is resolved: lora.options fills conv_rank with rank where LORA_PARAMS leaves it out (conv_alpha may stay None = alpha)
            raise ValueError("LoRA scope \"unet\" needs the rank of the 3x3 convolutions: LoraSpec(rank, alpha, targets, \"unet\", conv_rank)")
        if self.conv_rank is not None and self.conv_rank not in LORA_RANKS:
            raise ValueError(f"LoRA conv_rank {self.conv_rank!r} is not one of {LORA_RANKS}")
        if self.conv_alpha is not None and not (float(self.conv_alpha) > 0.0):
            raise ValueError(f"LoRA conv_alpha must be > 0, got {self.conv_alpha!r}")
        if (self.conv_rank is not None or self.conv_alpha is not None) and self.scope != "unet":
            raise ValueError(f"LoRA conv_rank / conv_alpha belong to scope \"unet\" (scope {self.scope!r} adapts no convolution)")
        if not isinstance(self.dora, bool):
            raise ValueError(f"LoRA dora must be True or False, got {self.dora!r}")
        if self.dora and (self.scope == "unet" or self.max_norm is not None or self.has_dropout):
            raise ValueError("LoRA dora goes with scope \"attention\" or \"transformer\" and without dropout or max_norm (DoRA on the "
                             "convolutions, with dropout and with max-norm are follow-ups)")

    @property
    def scale(self) -> float:
        return float(self.alpha) / self.rank

    @property
    def conv3_rank(self) -> int:
        """Rank of the 3x3 convolutions: conv_rank, or rank where it is None."""
        return self.rank if self.conv_rank is None else self.conv_rank

    @property
    def conv3_alpha(self) -> float:
        return float(self.alpha if self.conv_alpha is None else self.conv_alpha)

    def rank_of(self, module: str) -> int:
        return self.conv3_rank if lora_is_conv3(module) else self.rank

    def alpha_of(self, module: str) -> float:
        return self.conv3_alpha if lora_is_conv3(module) else float(self.alpha)

    def scale_of(self, module: str) -> float:
        return self.alpha_of(module) / self.rank_of(module)

    @property
    def has_dropout(self) -> bool:
        return float(self.dropout) > 0.0 or float(self.rank_dropout) > 0.0 or float(self.module_dropout) > 0.0

    @property
    def dropout_thresholds(self) -> Tuple[int, int, int]:
        """(t_net, t_rank, t_mod): an element is kept iff its 16 random bits are >= t; 0 = the kind is off and draws nothing."""
        return tuple(lora_dropout_threshold(float(p)) for p in (self.dropout, self.rank_dropout, self.module_dropout))

    @property
    def dropout_inv(self) -> float:
        """1 / ((1 - dropout)(1 - rank_dropout)) in double; the kernel takes it rounded to fp32 (module dropout is not rescaled)."""
        return 1.0 / ((1.0 - float(self.dropout)) * (1.0 - float(self.rank_dropout)))


def lora_modules(cfg: UNetConfig, spec: LoraSpec) -> List[str]:
    """The adapted modules (names without '.weight') in parameter-table order.  A keyword that names a layer outside the scope, or
    one that selects nothing, is refused."""
    import fnmatch
    kws = [k.strip() for k in (spec.targets or "").split(",") if k.strip()] or ["*"]
    match = lambda name, kw: fnmatch.fnmatch(name, kw if "*" in kw else f"*{kw}*")
    table = param_table(cfg)
    linears = [n[:-7] for n, shape in table if n.endswith(".weight") and len(shape) == 2]
    if spec.scope == "unet":
        resnet_conv = lambda m: ".resnets." in m and m.rsplit(".", 1)[-1] in LORA_CONVS + ("conv_shortcut",)
        weights = [n[:-7] for n, shape in table if n.endswith(".weight") and len(shape) in (2, 4)]
        eligible = [m for m in weights if (m in linears and ".attentions." in m) or resnet_conv(m)]
        for kw in kws:
            if any(match(m, kw) for m in eligible):
                continue
            for m in weights:
                why = [w for key, w in LORA_UNET_REFUSED if key in m]
                if m not in eligible and why and match(m, kw):
                    raise ValueError(f"LoRA target {kw!r} names {m}: out of scope \"unet\" ({why[0]}); the scope adapts the Linears of "
                                     "every Transformer2DModel and conv1, conv2, conv_shortcut of every ResnetBlock2D")
            raise ValueError(f"LoRA target {kw!r} selects no Linear of a Transformer2DModel and no convolution of a ResnetBlock2D "
                             "(scope \"unet\")")
        return [m for m in eligible if any(match(m, kw) for kw in kws)]
    if spec.scope == "transformer":
        eligible = [m for m in linears if ".attentions." in m]
        for kw in kws:
            if not any(match(m, kw) for m in eligible):
                raise ValueError(f"LoRA target {kw!r} selects no linear of a Transformer2DModel (scope \"transformer\": proj_in, the "
                                 "attention projections, ff.net.0.proj, ff.net.2, proj_out)")
        return [m for m in eligible if any(match(m, kw) for kw in kws)]
    eligible = [m for m in linears if ".transformer_blocks." in m and (".attn1." in m or ".attn2." in m)]
    out_of_scope = [m for m in linears if m not in eligible and (".attentions." in m or ".ff." in m)]
    for kw in kws:
        if any(match(m, kw) for m in eligible):
            continue
        other = [m for m in out_of_scope if match(m, kw)]
        if other:
            raise ValueError(f"LoRA target {kw!r} names {other[0]}: adapters on proj_in / proj_out and the feed-forward linears are "
                             "out of scope (the GEGLU epilogue consumes the base product alone)")
        raise ValueError(f"LoRA target {kw!r} selects no attention projection")
    mods = [m for m in eligible if any(match(m, kw) for kw in kws)]
    return mods


def lora_table(cfg: UNetConfig, spec: LoraSpec):
    """[(name, shape)] of the adapter parameters, appended behind conv_out.bias in the parameter-table order of their modules.  Per
    attention, the down matrices A [r][in] of its fused group first (adjacent: one stacked operand), then the group's up matrices
    B [out][r], then to_out.0 (attn2: to_q first).  Every other linear of scope "transformer" (proj_in, ff.net.0.proj, ff.net.2,
    proj_out) is A, then B, at its module's place, and so are conv1, conv2 and conv_shortcut of scope "unet".  With spec.dora the
    magnitudes `<module>.dora_scale` (out,) of a group follow its up matrices, in the group's part order."""
    shapes = dict(param_table(cfg))
    order = lora_modules(cfg, spec)
    mods = set(order)
    out, done = [], set()
    for m in order:
        if ".attn1." in m or ".attn2." in m:
            a = m[:m.index(".to_")]
            if a in done:
                continue
            done.add(a)
            groups = ([["to_q", "to_k", "to_v"], ["to_out.0"]] if a.endswith("attn1") else [["to_q"], ["to_k", "to_v"], ["to_out.0"]])
        else:
            a, groups = None, [[m]]
        for g in groups:
            names = [f"{a}.{p}" for p in g if f"{a}.{p}" in mods] if a is not None else g
            for n in names:       # a 3x3 convolution: A (r, Cin, 3, 3), stored like the base weight [r][3][3][Cin]; conv_shortcut: (r, Cin)
                shp = shapes[n + ".weight"]
                out.append((n + ".lora_A.weight", (spec.rank_of(n), shp[1]) + (tuple(shp[2:]) if lora_is_conv3(n) else ())))
            out += [(n + ".lora_B.weight", (shapes[n + ".weight"][0], spec.rank_of(n))) for n in names]
            if spec.dora:
                out += [(n + ".dora_scale", (shapes[n + ".weight"][0],)) for n in names]
    return out
