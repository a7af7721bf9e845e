"""The LoRA adapter executor of AozoraUNet (INTEGRATION.md "LoRA"): which kernel carries each adapter product (LoraRoutes), the stacked
views of the adapters of one layer (LoraGroup) with the four per-group operations AozoraUNet.linear / conv call (LoraAdapters: fwd, du,
wgrad, dgrad), and the transposed-copy jobs of the adapter matrices (wt_jobs).  Host-side placement only: the arithmetic is az_lora_*
(csrc/az_lora.hip) and the general products behind ops.  lora.py holds the options and the file format."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import ops
from ._lib import AozoraError
from .param_groups import ALIGN


class LoraRoutes:
    """The routing rules and nothing else: no UNet, no device.  The thresholds are class attributes that an instance may override."""
    # Which kernel carries an adapter product follows tools/lora_time.py (profiles/lora_time.json): an az_lora_* kernel is used where it
    # beats az_gemm_bf16 beyond the repeat spread, or where the general product cannot express the contract -- a factor s != 1, a small
    # dimension that is no multiple of 8 (rank 4 and its 8-byte slices), `du` of several parts with s.  Everywhere else the general
    # product in its accumulate form computes the same contract:
    #   down   az_lora_down_bf16, except many rows at a stacked rank >= 64 (M = 16384, r = 64: 13.3 against 9.2 us)
    #   up     az_gemm_bf16, except few rows at rank <= 32 (the text context: 5.2 against 7.3 us) and a fused q|k|v group of rank <= 16
    #          at up to 4096 rows in ONE launch (22.2 against 25.6 us for three general products)
    #   tall   az_gemm_bf16 (the adapter kernel loses at every shape: 24.1 against 15.5 us)
    #   up + GEGLU (ff.net.0.proj; profiles/lora_ff_time.json)  az_lora_up_geglu_bf16 where the up product alone would be az_lora_up_bf16:
    #          against that kernel + az_geglu_fwd it wins beyond the spread (M = 4096, H = 5120: 65.2 against 69.2 us at rank 16, 120.9
    #          against 123.2 at rank 64; M = 16384, H = 2560, rank 16: 125.7 against 134.7), except many rows at rank 64, where two
    #          MI355X disagreed (233.7 against 241.5 us on one, 251.3 against 244.0 on the other): the two-launch form there.  Where the
    #          up product is the general product (s = 1, rank % 8 == 0, many rows) the fused kernel loses to it + az_geglu_fwd (65.3
    #          against 56.2, 120.4 against 55.6, 125.5 against 101.4, 233.2 against 108.7 us): the two-launch form there too
    # The thresholds are attributes so that a test can reach both sides at small shapes; they choose speed, not the contract (the fp32
    # summation order differs between the two kernels).
    DOWN_GEMM_ROWS, DOWN_GEMM_RANK = 8192, 64
    UP_FEW_ROWS, UP_FEW_RANK = 512, 32
    UP_FUSED_ROWS, UP_FUSED_RANK = 4096, 16
    UP_GEGLU_ROWS, UP_GEGLU_RANK = 8192, 64

    def down_general(self, rows, R) -> bool:
        """The down product over a stacked rank R goes to az_gemm_bf16 (True) or to az_lora_down_bf16 (False)."""
        return R % 8 == 0 and R >= self.DOWN_GEMM_RANK and rows >= self.DOWN_GEMM_ROWS

    def up_own(self, rows, r, s, parts=1) -> bool:
        """The up product goes to az_lora_up_bf16 (True) or to az_gemm_bf16 in its accumulate form (False)."""
        return (s != 1.0 or r % 8 != 0 or (rows <= self.UP_FEW_ROWS and r <= self.UP_FEW_RANK)
                or (parts == 3 and rows <= self.UP_FUSED_ROWS and r <= self.UP_FUSED_RANK))

    def up_geglu_fused(self, rows, r, s) -> bool:
        """az_lora_up_geglu_bf16 (True) wherever `up` would take az_lora_up_bf16, except many rows at a high rank; else two launches."""
        return self.up_own(rows, r, s) and not (rows >= self.UP_GEGLU_ROWS and r >= self.UP_GEGLU_RANK)

    @staticmethod
    def tall_general(s, ns) -> bool:
        """A tall reduction goes to az_gemm_bf16 (True) wherever it can express it, else to az_lora_wgrad_bf16."""
        return s == 1.0 and ns % 8 == 0

    def down(self, x, w, out):
        """out = x w^T (the stacked down matrices: x is read once)."""
        if self.down_general(x.shape[0], w.shape[0]):
            ops.gemm(x, w, out, trans_b=True)
        else:
            ops.lora_down(x, w, out)

    def up(self, u, w, y, s, parts=1):
        """y_p += s u_p w_p^T for the `parts` stacked parts."""
        r, N, rows = w.shape[1], w.shape[0] // parts, u.shape[0]
        if self.up_own(rows, r, s, parts):
            ops.lora_up(u, w, y, parts=parts, scale=s)
            return
        for p in range(parts):
            ops.gemm(u[:, p * r:(p + 1) * r], w[p * N:(p + 1) * N], y[:, p * N:(p + 1) * N], trans_b=True, accumulate=True)

    def up_geglu(self, u, w, proj, out, s):
        """proj += s u w^T, then out = GEGLU(proj): az_lora_up_geglu_bf16 (one launch, proj read once) wherever `up` would take
        az_lora_up_bf16, else the two-launch form (the general product, then az_geglu_fwd)."""
        if self.up_geglu_fused(u.shape[0], w.shape[1], s):
            ops.lora_up_geglu(u, w, proj, out, scale=s)
        else:
            self.up(u, w, proj, s)
            ops.geglu_fwd(proj, out)

    def tall(self, small, big, out, s, parts, small_major):
        """out_p += s small_p^T big_p; out_p [ns][nb] (small_major) or [nb][ns]."""
        ns, nb = small.shape[1] // parts, big.shape[1] // parts
        if self.tall_general(s, ns):
            for p in range(parts):
                sp, bp = small[:, p * ns:(p + 1) * ns], big[:, p * nb:(p + 1) * nb]
                if small_major:
                    ops.gemm(sp, bp, out[p * ns:(p + 1) * ns], trans_a=True, trans_b=False, accumulate=True, split_k=0)
                else:
                    ops.gemm(bp, sp, out[p * nb:(p + 1) * nb], trans_a=True, trans_b=False, accumulate=True, split_k=0)
        else:
            ops.lora_wgrad(small, big, out, parts=parts, scale=s, accumulate=True, small_major=small_major)

    # The three gathered products of an adapter on a 3x3 convolution (conv1 / conv2 of a ResnetBlock2D).  az_conv2d_bf16 expresses
    # each of them with Cout = r (s = 1 on all three here: the factor rides on the up product and on du; rank % 8 == 0), and the rule
    # above decides: tools/lora_conv_time.py (profiles/lora_conv_time.json) alternated both sides at the SDXL resnet shapes, B = 4 at
    # 1024^2, ranks 16 and 64 (adapter kernel against general kernel, us):
    #   down   128^2 x 320: 80.2 / 70.4 (r 16), 199.5 / 75.5 (r 64)      64^2 x 640: 42.9 / 59.8, 100.9 / 60.1
    #          32^2 x 1280: 28.4 / 113.2, 53.2 / 113.2                    32^2 x 2560: 54.4 / 221.0, 102.0 / 231.5
    #          the adapter kernel's one pass over x wins while the grid is small; the general kernel from 65536 pixels on, and from 16384
    #          on at rank 64 (the adapter kernel's time grows with the rank, the general kernel's does not)
    #   dgrad  the general kernel at every measured shape (95.4 / 26.6, 431.2 / 43.5; 44.7 / 14.4, 205.8 / 21.8; 27.4 / 10.3, 111.1 / 14.9;
    #          45.3 / 16.4, 185.1 / 25.9): nine k-steps per 16 x 16 tile with the rank padded to 32 lose to its LDS-staged tiles
    #   wgrad  the general kernel at every measured shape (178.7 / 75.0, 320.2 / 77.8; 88.5 / 42.1, 161.5 / 46.1; 47.2 / 25.6, 85.9 / 30.1;
    #          69.1 / 41.2, 126.1 / 44.1): the adapter kernel reads x once per tap
    # Each rule is a tuple of (rows, rank) pairs: the general kernel is issued where pixels >= rows and rank >= rank holds for one of
    # them -- the measured region where it won beyond the repeat spread -- and the az_lora_conv_* kernel everywhere else: below 4096
    # pixels and below rank 16 (nothing measured), and at the ranks the general kernel cannot take (rank 4: Cout % 8).  Attributes, so that
    # a test can reach both sides at small shapes; they choose speed, not the contract.
    CONV_DOWN_GEMM = ((65536, 16), (16384, 64))       # u = A (*) x
    CONV_DGRAD_GEMM = ((4096, 16),)                    # dx += A^T (*) du
    CONV_WGRAD_GEMM = ((4096, 16),)                    # dA += du^T (*) x

    @staticmethod
    def conv_general(rule, rows, r) -> bool:
        return r % 8 == 0 and any(rows >= lo_rows and r >= lo_rank for lo_rows, lo_rank in rule)

    def conv_down(self, g, x, geom, u):
        """u = A (*) x."""
        if self.conv_general(self.CONV_DOWN_GEMM, x.shape[0], g.r):
            ops.conv_fwd(ops.as4(x, *geom), g.A, ops.as4(u, *geom))
        else:
            ops.lora_conv_down(x, geom, g.A, u)

    def conv_dgrad(self, g, du, geom, dx):
        """dx += A^T (*) du over the transposed copy of the down matrix."""
        if self.conv_general(self.CONV_DGRAD_GEMM, du.shape[0], g.r):
            ops.conv_dgrad_wt(ops.as4(du, *geom), g.At, ops.as4(dx, *geom), accumulate=True)
        else:
            ops.lora_conv_dgrad(du, geom, g.At, dx)

    def conv_wgrad(self, g, x, geom, u, dy, du):
        """dA += du^T (*) x; dB += s dy^T u."""
        if self.conv_general(self.CONV_WGRAD_GEMM, x.shape[0], g.r):
            ops.conv_wgrad(ops.as4(du, *geom), ops.as4(x, *geom), g.GA, accumulate=True, split_k=0)
        else:
            ops.lora_conv_wgrad(du, x, geom, g.GA)
        self.tall(u, dy, g.GB, g.s, 1, False)


@dataclass(eq=False)
class LoraGroup:
    """The adapters of one layer call: a single projection, the adapted parts of a fused one, or a 3x3 convolution."""
    parts: List[int]        # column part of the fused output each adapted projection writes
    n: int                  # adapted parts, stacked side by side in the views below
    full: bool              # every part of the layer is adapted: one launch carries the whole group
    r: int                  # the modules' own rank (conv_rank differs from rank)
    N: int                  # output columns of one part
    K: int                  # input columns (Cin of a convolution)
    s: float                # alpha / rank
    names: List[str]        # parameter names, A in front of its B per part
    A: torch.Tensor         # [n r][K] down matrices; conv3: [r][3][3][Cin], the base weight's layout
    GA: torch.Tensor        # ... their gradient
    At: torch.Tensor        # [K][n r] transposed copy; conv3: [Cin][3][3][r] (the copies wt_jobs names)
    B: torch.Tensor         # [n N][r] up matrices
    GB: torch.Tensor        # ... their gradient
    Bt: torch.Tensor        # [n r][N] transposed copies, one per part
    conv3: bool = False     # the gathered products of a 3x3 convolution: the operations below need its (B, H, W)
    mids: List[int] = field(default_factory=list)     # module id per adapted part (index of <module>.weight in the parameter table): the dropout masks' key
    # DoRA (INTEGRATION.md "DoRA"; None / empty without it): the gains of the adapted parts side by side, the names of their magnitudes
    # (a slot of the flat buffer is padded: the gradients of adjacent parts are one vector only where N fills whole slots) and the parts
    # of the layer that carry no adapter (they pass through with a gain of 1)
    dg: Optional[torch.Tensor] = None        # [n N] fp32 gains g = m / norm
    dinv: Optional[torch.Tensor] = None      # [n N] fp32 1 / norm
    skip: List[int] = field(default_factory=list)
    ones: Optional[torch.Tensor] = None
    dm_names: List[str] = field(default_factory=list)

    @property
    def dora(self) -> bool:
        return self.dg is not None


class LoraAdapters:
    """The adapters of one AozoraUNet: views of its three flat buffers by slot, grouped per layer call and cached."""

    def __init__(self, slots: Dict[str, tuple], pflat, gflat, wtflat, scale_of: Callable[[str], float], trainable: Callable[[str], bool],
                 spec=None, mid_of: Optional[Callable[[str], int]] = None, dora=None):
        self.slots, self.flats, self.scale_of, self._trainable = slots, (pflat, gflat, wtflat), scale_of, trainable
        self.routes = LoraRoutes()
        # LoRA dropout (INTEGRATION.md "LoRA dropout"): (thresholds, inv) of a spec that has one, the seed of the masks, and the device
        # word that holds the micro-step -- armed by AozoraUNet.begin_step for a training step, None everywhere else (no masks: eval)
        self._mid_of = mid_of if mid_of is not None else (lambda module: 0)
        self.drop = (spec.dropout_thresholds, spec.dropout_inv) if spec is not None and spec.has_dropout else None
        self.seed = 0
        self.step_word = None
        self.dora = dora          # dora.DoraState under LoraSpec(dora=True), else None
        self._groups: Dict[tuple, Optional[LoraGroup]] = {}

    def group(self, mods, conv3=False) -> Optional[LoraGroup]:
        """The adapters of the modules `mods` (the projections of one linear() call, or the one 3x3 convolution of a conv() call), or None."""
        key = ("conv3",) + tuple(mods) if conv3 else tuple(mods)
        if key in self._groups:
            return self._groups[key]
        have = [(p, m) for p, m in enumerate(mods) if m + ".lora_A.weight" in self.slots]
        g = None
        if have:
            n = len(have)
            oA, stA, _ = self.slots[have[0][1] + ".lora_A.weight"]
            oB, stB, _ = self.slots[have[0][1] + ".lora_B.weight"]
            r, K, N = stA[0], stA[-1], stB[0]
            for i, (_, m) in enumerate(have):
                if self.slots[m + ".lora_A.weight"][0] != oA + i * math.prod(stA) or self.slots[m + ".lora_B.weight"][0] != oB + i * N * r:
                    raise AozoraError(f"adapters of {mods} are not adjacent in the flat buffer")
            a_shape = (n * r,) + tuple(stA[1:])
            views = lambda o, *shapes: [buf[o:o + math.prod(sh)].view(sh) for buf, sh in zip(self.flats, shapes)]
            A, GA, At = views(oA, a_shape, a_shape, a_shape[::-1])
            B, GB, Bt = views(oB, (n * N, r), (n * N, r), (n * r, N))
            g = LoraGroup([p for p, _ in have], n, n == len(mods), r, N, K, self.scale_of(have[0][1]),
                          [m + sfx for _, m in have for sfx in (".lora_A.weight", ".lora_B.weight")], A, GA, At, B, GB, Bt, conv3,
                          mids=[self._mid_of(m) for _, m in have])
            if self.dora is not None:
                g.dg, g.dinv = self.dora.gains([m for _, m in have])
                g.dm_names = [m + ".dora_scale" for _, m in have]
                g.names = g.names + g.dm_names
                g.skip, g.ones = [p for p in range(len(mods)) if p not in g.parts], self.dora.ones[:N]
        self._groups[key] = g
        return g

    def trainable(self, g) -> bool:
        return g is not None and any(self._trainable(n) for n in g.names)

    @staticmethod
    def _launches(g):
        """(index in the stack, column part of the fused output, number of parts) per launch: one launch for a whole group."""
        return [(0, 0, g.n)] if g.full else [(i, p, 1) for i, p in enumerate(g.parts)]

    def dropout(self, g, t, rows_per_sample):
        """The masks of this step on t = u or du [rows][n r], in place: one launch for the group, every part a module of its own.  Issued
        only under a spec that has dropout AND with a step word armed."""
        if self.drop is not None and self.step_word is not None:
            ops.lora_dropout(t, g.r, g.n, rows_per_sample, g.mids, self.drop[0], self.drop[1], self.seed, self.step_word)

    def fwd(self, g, x, u, y, geom=None, geglu_out=None, rows_per_sample=None):
        """u = x A_cat^T (x read once; conv3: u = A (*) x), the dropout masks on u, then y_p += s u_p B_p^T on the column slices of the
        fused output -- with `geglu_out` (ff.net.0.proj) by the product that also writes GEGLU(y) there."""
        if g.conv3:
            self.routes.conv_down(g, x, geom, u)
        else:
            self.routes.down(x, g.A, u)
        self.dropout(g, u, rows_per_sample)
        if geglu_out is not None:
            self.routes.up_geglu(u, g.B, y, geglu_out, g.s)
            return
        for i, p, n in self._launches(g):
            self.routes.up(u[:, i * g.r:(i + n) * g.r], g.B[i * g.N:(i + n) * g.N], y[:, p * g.N:(p + n) * g.N], g.s, n)

    def _dm_launches(self, g):
        """_launches for the magnitudes' gradient: a whole group in one launch only where its parts' slots are adjacent without padding."""
        return self._launches(g) if g.N % ALIGN == 0 else [(i, p, 1) for i, p in enumerate(g.parts)]

    def dora_fwd(self, g, v, y, bias=None, residual=None):
        """y = g v (+ bias, + residual) on the column slices of the fused output (az_dora_scale_bf16); a part without an adapter passes
        through with a gain of 1."""
        if (bias is not None or residual is not None) and (g.n != 1 or g.skip):
            raise AozoraError("dora: a fused projection carries neither bias nor residual")
        N = g.N
        for i, p, n in self._launches(g):
            ops.dora_scale(v[:, p * N:(p + n) * N], g.dg[i * N:(i + n) * N], y[:, p * N:(p + n) * N], bias=bias, residual=residual)
        for p in g.skip:
            ops.dora_scale(v[:, p * N:(p + 1) * N], g.ones, y[:, p * N:(p + 1) * N])

    def dora_bwd(self, g, dy, v, dv):
        """dv = g dy and dm += inv colsum(dy v) (az_dora_bwd_bf16; dm only where the magnitude is trainable); a part without an adapter: dv = dy."""
        N = g.N
        for i, p, n in self._dm_launches(g):
            # one launch writes dm of all its n parts: like dA / dB of a stacked group, a frozen part beside a trainable one receives a
            # gradient that nobody reads (the optimizers go by the freeze mask)
            train = any(self._trainable(nm) for nm in g.dm_names[i:i + n])
            dm = None
            if train:
                o = self.slots[g.dm_names[i]][0]
                dm = self.flats[1][o:o + n * N]
            ops.dora_bwd(dy[:, p * N:(p + n) * N], g.dg[i * N:(i + n) * N], dv[:, p * N:(p + n) * N], v=v[:, p * N:(p + n) * N],
                         inv=g.dinv[i * N:(i + n) * N], dm=dm)
        for p in g.skip:
            ops.dora_bwd(dy[:, p * N:(p + 1) * N], g.ones, dv[:, p * N:(p + 1) * N])

    def du(self, g, dy, du, rows_per_sample=None):
        """du_p = s dy_p B_p over the transposed copies of the up matrices, then the forward pass's masks on du."""
        for i, p, n in self._launches(g):
            ops.lora_down(dy[:, p * g.N:(p + n) * g.N], g.Bt[i * g.r:(i + n) * g.r], du[:, i * g.r:(i + n) * g.r], parts=n, scale=g.s)
        self.dropout(g, du, rows_per_sample)

    def wgrad(self, g, x, u, dy, du, geom=None):
        """dA_cat += du^T x (conv3: dA += du^T (*) x); dB_p += s dy_p^T u_p."""
        if g.conv3:
            self.routes.conv_wgrad(g, x, geom, u, dy, du)
            return
        self.routes.tall(du, x, g.GA, 1.0, 1, True)
        for i, p, n in self._launches(g):
            self.routes.tall(u[:, i * g.r:(i + n) * g.r], dy[:, p * g.N:(p + n) * g.N], g.GB[i * g.N:(i + n) * g.N], g.s, n, False)

    def dgrad(self, g, du, dx, geom=None):
        """dx += du A_cat (conv3: dx += A^T (*) du) over the transposed copy of the down matrices."""
        if g.conv3:
            self.routes.conv_dgrad(g, du, geom, dx)
        else:
            self.routes.up(du, g.At, dx, 1.0)


def wt_jobs(table, slots) -> Tuple[List[Tuple[int, int, int]], List[Tuple[int, int, int]]]:
    """The transposed-copy jobs of the adapters (`table`: the adapter part of the parameter table, `slots`: name -> (offset, storage
    shape, shape)) -> (linear jobs (offset, rows N, cols K), 3x3 jobs (offset, Cout, Cin)).  The backward data products of az_lora_* are NT
    products over transposed copies -- the adjacent down matrices of a fused group as ONE stacked [parts r][K] -> [K][parts r] job
    (dx += du A_cat), every up matrix [N][r] -> [r][N] on its own (stacked they are the [parts r][N] operand of du = s dy B).  The down
    matrix of a 3x3 convolution, stored [r][3][3][Cin] like its base weight, gets the base weight's kind of copy: [Cin][3][3][r], nine
    strided transposes -- the operand of az_lora_conv_dgrad_bf16 and of the general data-gradient kernel."""
    lin, conv = [], []
    i = 0
    while i < len(table):
        o, st, _ = slots[table[i][0]]
        if table[i][0].endswith(".dora_scale"):       # a magnitude vector: no product reads it transposed
            i += 1
            continue
        if math.prod(st) % ALIGN:
            raise AozoraError(f"adapter {table[i][0]} {st} does not fill whole {ALIGN}-element slots: stacked groups would not be adjacent")
        if len(st) == 4:
            conv.append((o, st[0], st[3]))
            i += 1
            continue
        n = 1
        if table[i][0].endswith(".lora_A.weight"):
            while i + n < len(table) and table[i + n][0].endswith(".lora_A.weight") and slots[table[i + n][0]][1] == st:
                n += 1
            if n > 3:
                raise AozoraError(f"{n} adjacent down matrices from {table[i][0]} on: a fused group has at most 3 parts")
        lin.append((o, n * st[0], st[1]))
        i += n
    return lin, conv
