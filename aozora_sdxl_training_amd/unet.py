"""AozoraUNet -- drop-in for the `unet` object of the reference's train loop (train.py:1437-1469 load,
2660-2667 setup, 2760-2761 call), executed entirely by hand-written HIP kernels (libaozora_hip.so).

Design:
  * parameters, gradients and the transposed weight copies live in three flat bf16 device buffers owned by
    `self.params` (params.ParamStore: layout, regions, W^T freshness, state dicts); the UNet binds the
    same buffers and dicts under its own names and forwards the store's methods;
  * activations are NHWC == row-major [B*H*W][C] bf16, so ResnetBlock2D and Transformer2DModel share
    a layout and no permutes exist; their pools, arenas and gradient-buffer rules are `self.acts`
    (activations.ActivationStore), shown under the UNet's old names in the same way;
  * the weight / bias gradient launches of the backward go through `self.branch` (branch.GradBranch: queue, batches, parked work, forks, join);
  * forward records a tape of backward closures (static topology => the launch sequence is identical
    every step and can be captured into a hipGraph); all activations needed by the backward are kept
    (no gradient checkpointing: 288 GB HBM);
  * every FLOP runs in libaozora_hip.so; torch supplies memory and the stream only.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import os
import torch

from . import ops
from ._lib import lib, AozoraError, wait_event, run_live
from .unet_spec import UNetConfig, SDXL_BASE, param_table, up_resnet_channels, LoraSpec, lora_table
from .lora_exec import LoraAdapters
from .params import ParamStore
from .activations import Act, POOL_ALIGN, _Arena, _Pool, ActivationStore      # (the four names are re-exported: tests and tools import them from here)
from .branch import GradBranch

@dataclass
class ExecPolicy:
    """Where the executor places launches and which fusions it uses: data of ONE AozoraUNet (`unet.policy`), not process state.
    Every setting computes bit-identical losses and gradients (tests/test_model_gpu.py::test_executor_placements_and_fusions_are_
    bitwise_neutral) except `tn_group`, which changes the fp32 summation order of the grouped weight gradients."""
    fork_events: bool = True     # fork / join events without the system-scope fence (_lib.ForkEvent) instead of torch.cuda.Event
    fuse_records: int = 2        # launch tape: a fork event recorded right behind a kernel becomes that kernel's completion signal
                                 #   (1: on the data-gradient stream only, 2: on every stream, 0: off)
    side_batch: int = 1          # parameter-gradient launches per fork at most (block ends flush earlier)
    ln_fused: bool = True        # LayerNorm backward: dx and the gamma / beta partial sums from ONE pass over x / dy
    ln_defer: bool = True        # ... the partial sums finished once per parameter region on the branch (not one launch per LayerNorm)
    hoist: bool = True           # K/V-of-context and time-embedding projections as grouped launches per parameter region
    xkv_side: bool = True        # cross-attention dK / dV on the parameter-gradient branch (nothing on the chain reads them); False: ONE kernel for
                                 #      dQ, dK, dV on the chain (az_attn.hip attn_bwd_cross_kernel).  Re-measured at the end of round 5 on three boxes
                                 #      (False with ATTN_SPLIT_TARGET 192 against True): -0.69, +0.2, -0.02 ms per micro-step -- no decision, kept
    temb_side: bool = True       # time_emb_proj data gradients on the branch behind their producer (no chain wait per ResnetBlock2D)
    geglu_fuse: bool = True      # GEGLU forward inside the epilogue of its projection (ff.net.0.proj)
    cat_inplace: bool = True     # skip concatenations written in place by their producers (K14): no copies
    xkv_group: bool = True       # the weight gradients of the cross-attention K / V projections (hoisted: one shared 77-token context, K = 308 rows,
                                 #      5 k-tiles: never split) are parked per parameter region and go out as ONE grouped launch
                                 #      (az_gemm_tn_grouped_bf16) instead of one 18-us launch per transformer block; same tiles, same bits
    tn_group: int = 0            # > 0: linear weight gradients parked until they add up to this many 128x128 tiles, then ONE grouped
                                 #      launch over whole k-ranges (az_gemm_tn_grouped_bf16: no split-K slabs, no reduce launches).
                                 #      Off by default: same-box A/B 117.4 -> 118.6 ms per micro-step (the 75-us workgroups of an unsplit
                                 #      product hold CU slots the data-gradient chain's next kernel needs)
    host_tape: bool = True       # re-issue a bucket's launch sequence from the recorded launch tape
    native_tape: bool = True     # ... played by the C side (az_tape_play); False: replayed from Python
    side_streams: int = 1        # parameter-gradient branch streams (more than one measured slower)
    side_priority: int = 0
    main_priority: int = 0


BF16 = torch.bfloat16
F32 = torch.float32


class _UNetCall(torch.autograd.Function):
    """Autograd bridge for the reference's own loop body: `pred = unet(...).sample; loss = f(pred);
    (loss / GA).backward()` (train.py:2760-2765).  forward = HIP forward, backward = HIP backward seeded
    with d(loss)/d(pred); parameter gradients are ACCUMULATED into the flat gradient buffer and exposed
    as `.grad` views (post-accumulate hooks do not fire: Titan users call optimizer.offload_flat(unet))."""

    @staticmethod
    def forward(ctx, anchor, unet, sample, t_f32, ehs, pooled, tids_f32):
        B, C, H, W = sample.shape
        unet.check_latent_shape(H, W)
        unet.begin_step((B, H, W, ehs.shape[1], "call"))
        x8 = unet.acts.pool.get((B, H, W, 8), BF16)
        ops.nchw_to_nhwc_pad(sample.contiguous(), x8, C)
        pred = unet.forward_nhwc(x8, t_f32, ehs, pooled, tids_f32)
        out = torch.empty(B, unet.cfg.out_channels, H, W, dtype=BF16, device=sample.device)
        ops.nhwc_to_nchw(pred.t.view(B, H, W, unet.cfg.out_channels), out, unet.cfg.out_channels)
        ctx.unet, ctx.pred, ctx.geom = unet, pred, (B, H, W)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        unet, (B, H, W) = ctx.unet, ctx.geom
        d8 = unet.acts.pool.get((B, H, W, 8), BF16)
        g = grad_out.contiguous()
        if g.dtype not in (BF16, F32):
            g = g.float()
        ops.nchw_to_nhwc_pad(g, d8, unet.cfg.out_channels)
        unet.backward_nhwc(ctx.pred, d8)
        unet.expose_grads()
        return None, None, None, None, None, None, None


class AozoraUNet:
    def __init__(self, cfg: UNetConfig = SDXL_BASE, device="cuda:0", policy: Optional[ExecPolicy] = None, lora: Optional[LoraSpec] = None):
        if not torch.cuda.is_available():
            raise AozoraError("AozoraUNet needs a HIP device; there is no CPU fallback")
        self.cfg = cfg
        self.policy = policy if policy is not None else ExecPolicy()
        self.config = SimpleNamespace(in_channels=cfg.in_channels, out_channels=cfg.out_channels,
                                      sample_size=128, cross_attention_dim=cfg.cross_attention_dim)
        self.device = torch.device(device)
        # library context of this UNet (az_init): its own copy of the execution-option table, made current on the issuing thread
        # at the start of every step -- two UNets (devices) in one process do not share option state
        # (context calls go to the bound functions directly, never through lib().call: they must not land on a launch tape that
        # happens to be recording -- a garbage-collected UNet's az_destroy replayed every step would be a double free)
        self._ctx = ctypes.c_void_p()
        if lib()._fn["az_init"](self.device.index if self.device.index is not None else torch.cuda.current_device(), ctypes.byref(self._ctx)):
            raise AozoraError("az_init failed")
        lib()._fn["az_make_current"](self._ctx)
        self.training = True
        # LoRA (INTEGRATION.md "LoRA"): the adapters are ordinary entries of the flat buffers BEHIND conv_out.bias -- the base slots keep
        # their offsets -- and the base table stays what state_dict / load_state_dict mean
        self.lora = lora
        base = param_table(cfg)
        P = self.params = ParamStore(cfg, base + (lora_table(cfg, lora) if lora is not None else []), len(base), self.device, owner=self)
        for k in ("pflat", "gflat", "wtflat", "flat_numel", "_table", "_base_table", "_slots", "_w", "_gw", "_params", "_gviews", "_wt_jobs",
                  "_wt_conv_jobs", "_wt", "_fused_w"):
            setattr(self, k, getattr(P, k))      # never rebound: the same objects under the names the layers, optimizers and tools read
        # the adapter executor (lora_exec.py): groups, routing rules and the four per-group operations linear() / conv() call
        mids = {n[:-len(".weight")]: i for i, (n, _) in enumerate(self._base_table) if n.endswith(".weight")}
        # DoRA (dora.py): the fp32 gains of the magnitudes, derived state that the FORWARD reads -- refreshed behind every parameter change
        self.dora = None
        if lora is not None and lora.dora:
            from .dora import DoraState
            self.dora = DoraState(self)
        self.adapters = (LoraAdapters(self._slots, self.pflat, self.gflat, self.wtflat, lora.scale_of, self._trainable, lora, mids.__getitem__,
                                      dora=self.dora)
                         if lora is not None else None)
        self._step_B = 1              # samples of the current step (forward_nhwc): rows / B = the rows of one sample, for rank dropout
        # the activation store (activations.py): pools, arenas, deferred readers, gradient-buffer rules
        A = self.acts = ActivationStore(self.device, on_replace=self._arena_replaced)
        self._pools, self._arenas, self._arena_clients = A.pools, A.arenas, A.clients      # never rebound: the same objects under the old names
        self._tape: List = []
        self.conv_in = True   # train.py:2694 probes hasattr(unet, 'conv_in')
        self._anchor = torch.zeros((), device=self.device, requires_grad=True)
        # the parameter-gradient branch (branch.py): the queue of weight / bias gradient launches, what the layers park, the fork events.
        # Its streams (round-robin): independent weight-gradient products of moderate size run side by side instead of each being
        # split-K'ed to fill the chip on its own (side_priority -1, a high-priority branch: +1 ms)
        self.branch = GradBranch(self.policy, A, [torch.cuda.Stream(device=self.device, priority=self.policy.side_priority)
                                                  for _ in range(max(1, self.policy.side_streams))], self.device)
        self._sides, self._ln_tables, self._tn_tables = self.branch.sides, self.branch.ln_tables, self.branch.tn_tables      # never rebound
        self._main_stream = None       # set by TrainStep: the exchange / copy streams are chosen to run beside it too
        self._hoisted: Dict[str, Act] = {}      # forward outputs computed ahead by grouped launches (name -> Act)
        self._group_tables = {}
        self._after_tail_hook = None
        self._tape_mark = self._tape_mark1 = 0
        for slot in (2, 1, 0):
            ops.set_workspace_slot(slot); ops.workspace(self.device)

    def __call__(self, sample, timestep, encoder_hidden_states, added_cond_kwargs=None, **_ignored):
        """diffusers call signature used at train.py:2760-2761; returns an object with `.sample` (B,C,H,W) bf16."""
        if added_cond_kwargs is None or "text_embeds" not in added_cond_kwargs or "time_ids" not in added_cond_kwargs:
            raise ValueError("SDXL needs added_cond_kwargs={'text_embeds', 'time_ids'}")
        if self.lora is not None and self.lora.has_dropout and torch.is_grad_enabled():
            raise AozoraError("this UNet's LoraSpec has dropout: its masks are keyed by the micro-step, which only "
                              "TrainStep.micro_step(lora_step=...) supplies; call the UNet under torch.no_grad() (eval: no masks) or train through TrainStep")
        B = sample.shape[0]
        t = torch.as_tensor(timestep, device=self.device).reshape(-1).float()
        if t.numel() == 1:
            t = t.expand(B)
        pooled = added_cond_kwargs["text_embeds"].to(device=self.device, dtype=BF16).contiguous()
        tids = added_cond_kwargs["time_ids"].to(self.device).float().contiguous()
        ehs = encoder_hidden_states.to(device=self.device, dtype=BF16).contiguous()
        out = _UNetCall.apply(self._anchor, self, sample.to(device=self.device, dtype=BF16), t.contiguous(), ehs, pooled, tids)
        return SimpleNamespace(sample=out)

    # ------------------------------------------------------------------ parameters ---------------
    # The parameter store (params.py) under the names callers use.  Methods of the UNet itself: the launch tape records the UNet's own bound
    # wait_region_params / _wait_wt_ready (Live operations), and the store holds all the state behind them.
    def named_parameters(self): return self.params.named_parameters()
    def parameters(self): return self.params.parameters()
    def state_dict(self): return self.params.state_dict()
    def load_state_dict(self, sd, strict=True): return self._dora_refreshed(self.params.load_state_dict(sd, strict), base=True)
    def lora_state_dict(self): return self.params.lora_state_dict()
    def load_lora_state_dict(self, sd): return self._dora_refreshed(self.params.load_lora_state_dict(sd))
    def init_lora(self, seed): return self._dora_refreshed(self.params.init_lora(seed), init=True)

    def _dora_refreshed(self, ret, init=False, base=False):
        """Behind a load: the gains of the DoRA magnitudes follow the new W, A, B, m (init: the magnitudes become the row norms first).
        A load of the base before any adapters exist (base) issues nothing: there is no magnitude to form a gain from yet."""
        if self.dora is not None and (self.dora.launches or not base):
            self.dora.refresh(init=init)
        return ret
    def trainable_ranges(self): return self.params.trainable_ranges()
    def expose_grads(self): return self.params.expose_grads()
    def zero_grad(self, set_to_none=True): return self.params.zero_grad(set_to_none)
    def requires_grad_(self, flag=True): return self.params.requires_grad_(flag)
    def mark_params_dirty(self): return self.params.mark_params_dirty()
    def region_bounds(self): return self.params.region_bounds()
    def tail_offset(self): return self.params.tail_offset()
    def refresh_transposed(self): return self.params.refresh_transposed()
    def transposed_refreshed_externally(self): return self.params.transposed_refreshed_externally()
    def set_region_params_event(self, k, ev): return self.params.set_region_params_event(k, ev)
    def wait_region_params(self, k): return self.params.wait_region_params(k)
    def wait_tail_params(self): return self.params.wait_tail_params()
    def _wait_wt_ready(self): return self.params._wait_wt_ready()
    def _trainable(self, name): return self.params.trainable(name)
    def refresh_transposed_async(self): return self.params.refresh_transposed_async(self._sides[0])

    def _region_hook(self, k):
        """Every gradient of region k has been issued.  Reads the hook at play time: TrainStep swaps it between replays."""
        if self._after_tail_hook is not None:
            self._after_tail_hook(k)

    def enter_micro_step(self, parity, defer_join=False) -> int:
        """TrainStep, before a micro-step on activation pool `parity` issues anything: wait for the deferred weight-gradient work of the
        pool's previous user, replace the arena if that user found it too small, and note how this micro-step's backward ends
        (GradBranch._end_join).  -> the arena's generation (ActivationStore.prepare)."""
        self.acts.wait_free(parity)
        gen = self.acts.prepare(parity)
        self.branch.enter(parity, defer_join)
        return gen

    def set_lora_dropout_seed(self, seed: int):
        """The seed of the LoRA dropout masks (config.SEED: masks are a function of (seed, micro-step) and of nothing else).  It rides
        in the arguments of recorded launches: a change lets go of every recorded launch tape and graph."""
        if self.adapters is None or self.adapters.seed == int(seed):
            return
        torch.cuda.synchronize(self.device)
        self.adapters.seed = int(seed)
        for ts in list(self.acts.clients):
            for bk in ts._buckets.values():
                bk.discard_recorded()

    # reference seams that are no-ops here ---------------------------------------------------------
    def enable_gradient_checkpointing(self):   # train.py:2660 -- not needed with 288 GB HBM
        return None

    def enable_xformers_memory_efficient_attention(self):
        return None

    def set_attn_processor(self, *_a, **_k):   # train.py:204-228 -- attention is az_attn_fwd/bwd
        return None

    def to(self, device=None, *_a, **_k):
        if device is not None and torch.device(device).type != "cuda":
            raise AozoraError("AozoraUNet lives on a HIP device only")
        return self

    def train(self, mode=True):
        self.training = mode
        return self

    # ------------------------------------------------------------------ tape helpers --------------
    def _wait_ready(self, a: Act):
        if a.ready is not None:
            wait_event(torch.cuda.current_stream(), a.ready)
            a.ready = None

    # ------------------------------------------------------------------ layers --------------------
    def _bias_grad(self, dy: torch.Tensor, bname: Optional[str], n_real: int, rows_per_seg=None, seg_out: Optional[Act] = None):
        """bias grad (first n_real columns of the column sums of dy); with `seg_out`, the per-segment
        column sums (segments of rows_per_seg rows = one sample) become seg_out's gradient [nseg][C]
        (the time-embedding add of ResnetBlock2D)."""
        rows, C = dy.shape
        if seg_out is not None and seg_out.need_grad:
            if C != n_real:
                raise AozoraError("segment sums need an unpadded gradient")
            rps = rows_per_seg
        else:
            seg_out, rps = None, rows
        bias = self._gw[bname] if (bname is not None and self._trainable(bname)) else None
        if seg_out is None and bias is None:
            return
        ops.colsum_grad(dy, rps, seg_out.g.view(-1) if seg_out is not None else None, bias, n_real)

    # ---- the adapter of a layer (lora_exec.LoraGroup `lg`): linear() and conv() place its launches through these three
    def _adapter_fwd(self, lg, x: Act, y: Act, geom=None, geglu_out: Optional[Act] = None):
        """The adapter follows the base product: u is taken from the pool behind y.  -> (u, whether the adapter is trainable).
        The rows of one sample (rank dropout): rows / B -- the context length for the K / V of a cross-attention, H W for a convolution."""
        u = self.acts.new(x.t.shape[0], lg.n * lg.r, need_grad=False)
        self.adapters.fwd(lg, x.t, u.t, y.t, geom, geglu_out.t if geglu_out is not None else None, x.t.shape[0] // self._step_B)
        return u, self.adapters.trainable(lg)

    def _adapter_du_buf(self, lg, x: Act) -> Optional[Act]:
        """du, first thing in a bwd(): whether or not the adapter is trainable (the pool's allocation order may not depend on the freeze mask)."""
        return self.acts.new(x.t.shape[0], lg.n * lg.r, need_grad=False) if lg is not None else None

    def _adapter_bwd(self, lg, l_train, x: Act, u: Act, dy, du: Act, geom=None):
        """Behind the base layer's weight gradient, in front of its data gradient: du on the chain if the input has a gradient, and the
        adapter's weight gradients on the branch.  (The layer adds adapters.dgrad to dx itself, directly behind its own data gradient.)"""
        rps = x.t.shape[0] // self._step_B
        if x.need_grad:
            self.adapters.du(lg, dy, du.t, rps)
        if l_train:
            def wgrad():
                # without an input gradient (the text context) nothing on the chain reads du, and dy may itself be produced on the
                # branch (the dK | dV kernel of a cross-attention): du then runs there too, in order behind its producer
                if not x.need_grad:
                    self.adapters.du(lg, dy, du.t, rps)
                self.adapters.wgrad(lg, x.t, u.t, dy, du.t, geom)
            self.branch.defer(wgrad)

    def linear(self, x: Act, wname: str, bname: Optional[str], residual: Optional[Act] = None,
               w_override: Optional[Tuple[torch.Tensor, torch.Tensor, bool]] = None, out: Optional[Act] = None,
               pre: Optional[Act] = None, side_dgrad: bool = False, geglu_out: Optional[Act] = None,
               lora_mods: Optional[List[str]] = None) -> Act:
        """pre: the forward product was already computed by a grouped launch (_hoist_shared_input_linears); only the backward
        closure is registered here, at the layer's own place on the tape.
        side_dgrad: the output's gradient is PRODUCED on the parameter-gradient branch (time_emb_proj: dY = the per-sample
        channel sums that ride on conv1's weight-gradient pass) and the input's gradient is read by the chain only at the very
        end of the backward pass (emb): the data gradient then runs on the branch too, in order behind its producer, instead
        of making the chain wait for the branch to catch up once per ResnetBlock2D.
        geglu_out: this linear is a GEGLU's projection: the product is issued as az_gemm_geglu_fwd_bf16, whose epilogue also
        writes value * gelu(gate) into geglu_out (geglu(..., pre=geglu_out) then only registers the backward closure).  With an
        adapter the GEGLU must see the adapted projection: plain product, down product, then az_lora_up_geglu_bf16 writes geglu_out.
        lora_mods: the module names of the projections a w_override fuses (their adapters stay per projection)."""
        if w_override is not None:
            W, GW, w_train = w_override
        else:
            W, GW, w_train = self._w[wname], self._gw[wname], self._trainable(wname)
        N = W.shape[0]
        WT = self._wt(W) if x.need_grad else None
        rows = x.t.shape[0]
        lg = None
        if self.adapters is not None:
            lg = self.adapters.group(lora_mods if lora_mods is not None else ([wname[:-len(".weight")]] if wname else []))
        dora = lg is not None and lg.dora
        if dora:
            # DoRA (INTEGRATION.md "DoRA"): v = the base product WITHOUT bias and residual (a hoisted one: `pre`), the up product on v in
            # place, then y = g v + bias + residual; v is kept for the backward.  The GEGLU follows on y: no fused form.
            v = pre if pre is not None else self.acts.new(rows, N, need_grad=False)
            y = out if out is not None else self.acts.new(rows, N)
            if pre is None:
                ops.gemm(x.t, W, v.t, trans_b=True, split_k=0 if (rows <= 512 and residual is None) else 1)
            u, l_train = self._adapter_fwd(lg, x, v)
            self.adapters.dora_fwd(lg, v.t, y.t, self._w[bname] if bname else None, residual.t if residual is not None else None)
            if geglu_out is not None:
                ops.geglu_fwd(y.t, geglu_out.t)
        elif pre is not None:
            y = pre
        else:
            y = out if out is not None else self.acts.new(rows, N)
            if geglu_out is not None and lg is None:
                ops.gemm_geglu_fwd(x.t, W, self._w[bname] if bname else None, y.t, geglu_out.t)
            else:
                # few-row products (the K/V projections of the 77-token context: 48 tiles) split along k to cover more CUs
                # (an adapted GEGLU projection: the plain product -- the GEGLU follows the adapter, in LoraRoutes.up_geglu)
                ops.gemm(x.t, W, y.t, trans_b=True, bias=self._w[bname] if bname else None,
                         residual=residual.t if residual is not None else None,
                         split_k=0 if (rows <= 512 and residual is None) else 1)
        if lg is not None and not dora:      # the adapter follows the base product (a hoisted one: here, at the layer's own place on the tape)
            u, l_train = self._adapter_fwd(lg, x, y, geglu_out=geglu_out)

        def bwd():
            dy = y.g
            if dy is None:
                return
            du = self._adapter_du_buf(lg, x)
            # DoRA: every consumer of dy but the bias and the residual reads dv = g dy (pool order independent of the freeze mask)
            dyv = self.acts.pool.get(tuple(dy.shape), BF16) if dora else dy
            on_side = side_dgrad and self.policy.temb_side and self.branch.concurrent and len(self.branch.sides) == 1
            if dora and on_side:      # dy would be produced on the branch and read by az_dora_bwd_bf16 on the chain, unordered
                raise AozoraError("DoRA on a layer whose data gradient runs on the parameter-gradient branch (side_dgrad) is not supported")
            if on_side:
                y.ready = None      # written on the branch, read on the branch
            else:
                self._wait_ready(y)
            b_train = bname is not None and self._trainable(bname)
            job = (dy, x.t, GW, self._gw[bname] if b_train else None)
            if dora:
                # dv = g dy and the magnitude's gradient, ahead of every reader of dv: on the chain where the input has a gradient, else
                # (the text context: dy may itself be produced on the branch) on the branch, in order ahead of the weight gradients
                if x.need_grad:
                    self.adapters.dora_bwd(lg, dy, v.t, dyv)
                elif l_train or w_train:
                    self.branch.defer(lambda: self.adapters.dora_bwd(lg, dy, v.t, dyv))
                job = (dyv, x.t, GW, None)       # a trainable base weight takes dv; its bias the layer's own dy
                if w_train and b_train:
                    self.branch.defer(lambda: self._bias_grad(dy, bname, N))

            def wgrad():        # parameter gradients run as a free-running branch beside the data-gradient chain
                if w_train:
                    self.branch._linear_wgrad(*job)
                elif b_train:
                    self._bias_grad(dy, bname, N)
            if w_train and pre is not None and w_override is not None and rows <= 512 and self.policy.xkv_group and self.branch.concurrent and not on_side:
                # a hoisted context projection (K | V of a cross-attention): parked until the region's backward is through
                self.branch.park_xkv(job)
            elif w_train and self.policy.tn_group > 0 and 256 <= rows <= 8192 and not on_side:
                self.branch.park_tn(job)      # ... until the parked products add up to a chip-filling grid, then ONE grouped launch
            elif w_train or b_train:
                self.branch.defer(wgrad)
            if lg is not None:
                self._adapter_bwd(lg, l_train, x, u, dyv, du)
            if x.need_grad:
                dx, add = self.acts.gbuf(x)
                oop = add is not None and add is not dx

                def dgrad():
                    ops.gemm(dyv, WT, dx, trans_b=True, accumulate=add is dx, residual=add if oop else None,      # dX = dY . W  as  dY . (W^T)^T
                             split_k=0 if (rows <= 512 and not oop) else 1)
                    if lg is not None:
                        self.adapters.dgrad(lg, du.t, dx)         # dx += du A_cat, directly behind the base product
                if on_side:
                    self.branch.defer(dgrad)
                    x.ready = self.branch.flush()
                else:
                    dgrad()
            if residual is not None:   # dy becomes the residual's gradient (never written again: acts.gbuf)
                self.acts.give_grad(residual, dy)
        self._tape.append(bwd)
        return y

    def conv(self, x: Act, geom, wname, bname, stride=1, rowbias: Optional[Act] = None, residual: Optional[Act] = None,
             upsample=False, out: Optional[Act] = None, up_to: Optional[Tuple[int, int]] = None) -> Tuple[Act, tuple]:
        """3x3 conv (pad 1). The gradient handed to this op may carry more (zero) channels than Cout
        (conv_out: dpred is padded 4 -> 8 so that rows stay 16-byte chunks).
        upsample (Upsample2D): `geom` is x's own (half) resolution; forward and weight gradient read x through a
        nearest-2x gather inside the operand fetch, so the upsampled activation never exists; the data gradient comes out at
        the upsampled resolution into a scratch gradient and is folded 2x2 -> 1 by az_upsample2x_bwd.
        up_to: the upsample's target (H, W), each side 2n or 2n - 1 of x's (the skip tensor's geometry the result is concatenated
        with: F.interpolate(size=), the 2x image with its last row / column cropped); None: 2x.  The scratch gradient then has the
        cropped resolution and az_upsample_nearest_bwd folds it."""
        B, Hs, Ws = geom
        if upsample:
            H, W_ = up_to if up_to is not None else (2 * Hs, 2 * Ws)
            if H not in (2 * Hs - 1, 2 * Hs) or W_ not in (2 * Ws - 1, 2 * Ws):
                raise AozoraError(f"upsample target {(H, W_)} is not (2n or 2n-1) of {(Hs, Ws)}")
        else:
            H, W_ = Hs, Ws
        cropped = upsample and (H, W_) != (2 * Hs, 2 * Ws)
        Wt = self._w[wname]
        Cout, ks, _, Cin = Wt.shape
        Ho = (H + 2 - 3) // stride + 1
        Wo = (W_ + 2 - 3) // stride + 1
        y = out if out is not None else self.acts.new(B * Ho * Wo, Cout)      # out: a [rows][Cout] view with any row stride (one half of a skip concat)
        if tuple(y.t.shape) != (B * Ho * Wo, Cout):
            raise AozoraError("conv destination shape")
        x4 = ops.as4(x.t, B, Hs, Ws)
        ops.conv_fwd(x4, Wt, ops.as4(y.t, B, Ho, Wo), stride=stride, bias=self._w[bname],
                     rowbias=rowbias.t if rowbias is not None else None,
                     residual=ops.as4(residual.t, B, Ho, Wo) if residual is not None else None, upsample=upsample)
        # the adapter of conv1 / conv2 (scope "unet") follows the base launch: it sees the base's x and adds to a y that already holds
        # bias, the time-embedding row bias and the residual (y may be the strided half of a skip concatenation)
        lg = None
        if self.adapters is not None and ks == 3 and stride == 1 and not upsample:
            lg = self.adapters.group([wname[:-len(".weight")]], conv3=True)
        if lg is not None:
            u, l_train = self._adapter_fwd(lg, x, y, geom=geom)

        def bwd():
            dy = y.g
            if dy is None:
                return
            du = self._adapter_du_buf(lg, x)
            dy4 = ops.as4(dy, B, Ho, Wo)
            need_seg = rowbias is not None and rowbias.need_grad
            if need_seg:
                self.acts.gbuf_single(rowbias, "segment-sum target")      # allocate on the main path (pool order is stream-agnostic)
            self._wait_ready(y)

            def wgrad():
                b_train = self._trainable(bname)
                fuse = self._trainable(wname) and (b_train or need_seg) and (not need_seg or ((Ho * Wo) % 64 == 0 and dy.shape[1] == Cout))
                if fuse:        # bias / time-embedding gradients (channel sums of dY) ride on the weight-gradient pass
                    ops.conv_wgrad(dy4, x4, self._gw[wname], stride=stride, cout_real=Cout, accumulate=True, split_k=0,
                                   bias_grad=self._gw[bname] if b_train else None,
                                   seg_grad=rowbias.g.view(-1) if need_seg else None, upsample=upsample)
                else:
                    if rowbias is not None or b_train:
                        self._bias_grad(dy, bname, Cout, rows_per_seg=Ho * Wo, seg_out=rowbias)
                    if self._trainable(wname):
                        ops.conv_wgrad(dy4, x4, self._gw[wname], stride=stride, cout_real=Cout, accumulate=True, split_k=0, upsample=upsample)
            self.branch.defer(wgrad)
            if need_seg:       # the time-embedding gradient is produced on the side stream and read by the chain soon: issue now
                rowbias.ready = self.branch.flush()
            if lg is not None:
                self._adapter_bwd(lg, l_train, x, u, dy, du, geom)
            if x.need_grad:
                dx, add = self.acts.gbuf(x)
                if upsample:            # d(upsampled x) into a scratch buffer, then the 2x2 -> 1 fold into dx
                    if add is not None:
                        raise AozoraError("upsample input must have a single consumer")
                    dxs = dx
                    dx = self.acts.pool.get((B * H * W_, Cin), BF16)
                oop = add is not None and add is not dx
                res4 = ops.as4(add, B, H, W_) if oop else None
                if Cout % 8 == 0 and dy.shape[1] == Cout:
                    o_w = (Wt.data_ptr() - self.pflat.data_ptr()) // 2
                    wt = self.wtflat[o_w:o_w + Wt.numel()].view(Cin, 3, 3, Cout)
                    ops.conv_dgrad_wt(dy4, wt, ops.as4(dx, B, H, W_), stride=stride, accumulate=add is dx, residual=res4)
                else:
                    ops.conv_dgrad(dy4, Wt, ops.as4(dx, B, H, W_), stride=stride, cout_real=Cout, accumulate=add is dx, residual=res4)
                if lg is not None:
                    self.adapters.dgrad(lg, du.t, dx, geom)       # dx += A^T (*) du, directly behind the base data gradient
                if cropped:
                    ops.upsample_nearest_bwd(dx.view(B, H, W_, Cin), dxs.view(B, Hs, Ws, Cin))
                elif upsample:
                    ops.upsample2x_bwd(dx.view(B, H, W_, Cin), dxs.view(B, Hs, Ws, Cin))
            if residual is not None:
                self.acts.give_grad(residual, dy)
        self._tape.append(bwd)
        return y, (B, Ho, Wo)

    def groupnorm(self, x: Act, geom, prefix, eps, silu) -> Act:
        B, H, W_ = geom
        C = x.t.shape[1]
        G = self.cfg.norm_groups
        y = self.acts.new(B * H * W_, C)
        stats = self.acts.pool.get((B * G * 2,), F32)
        gam, bet = self._w[prefix + ".weight"], self._w[prefix + ".bias"]
        x3 = ops.as3(x.t, B, H * W_)
        ops.groupnorm_fwd(x3, gam, bet, y.t.view(B, H * W_, C), stats, G, eps, silu)

        def bwd():
            dy = y.g
            if dy is None:
                return
            tg, tb = self._trainable(prefix + ".weight"), self._trainable(prefix + ".bias")
            dy3 = ops.as3(dy, B, H * W_)
            dx3, add3 = None, None
            if x.need_grad:
                dx, add = self.acts.gbuf(x)
                dx3 = ops.as3(dx, B, H * W_)
                if add is not None:
                    add3 = ops.as3(add, B, H * W_)
            ops.groupnorm_bwd(x3, gam, bet, stats, dy3, dx3, self._gw[prefix + ".weight"] if tg else None,
                              self._gw[prefix + ".bias"] if tb else None, G, silu, dx_add=add3)
        self._tape.append(bwd)
        return y

    def layernorm(self, x: Act, prefix) -> Act:
        rows, C = x.t.shape
        y = self.acts.new(rows, C)
        stats = self.acts.pool.get((2 * rows,), F32)
        gam, bet = self._w[prefix + ".weight"], self._w[prefix + ".bias"]
        ops.layernorm_fwd(x.t, gam, bet, y.t, stats, 1e-5)

        def bwd():
            dy = y.g
            if dy is None:
                return
            dx, add = self.acts.gbuf(x)
            gw = self._gw[prefix + ".weight"] if self._trainable(prefix + ".weight") else None
            gb = self._gw[prefix + ".bias"] if self._trainable(prefix + ".bias") else None
            self._wait_ready(y)
            if self.policy.ln_fused:                              # one pass over x / dy for dx and the gamma / beta gradients
                if self.policy.ln_defer:
                    # ... whose per-block partial sums are parked: all LayerNorms of a parameter region are finished by ONE
                    # launch on the parameter-gradient branch (GradBranch.finish_ln) instead of one finish launch each on the chain.
                    # (The buffer is taken whether or not the parameters are frozen: the pool's allocation order may not
                    # depend on the freeze mask.)
                    nblk = ops.ln_partial_blocks(rows)
                    part = self.acts.pool.get((nblk * C * 2,), F32)
                if self.policy.ln_defer and (gw is not None or gb is not None):
                    ops.layernorm_bwd_partial(x.t, gam, stats, dy, dx, part, dx_add=add, nblk=nblk)
                    self.branch.park_ln((part, gw, gb, nblk, C))
                    return
                ops.layernorm_bwd(x.t, gam, stats, dy, dx, gw, gb, dx_add=add)
                return
            if gw is not None or gb is not None:       # gamma / beta gradients leave the data-gradient chain
                self.branch.defer(lambda: ops.layernorm_bwd(x.t, gam, stats, dy, None, gw, gb))
            ops.layernorm_bwd(x.t, gam, stats, dy, dx, None, None, dx_add=add)
        self._tape.append(bwd)
        return y

    def silu(self, x: Act) -> Act:
        y = self.acts.new(*x.t.shape)
        ops.silu_fwd(x.t, y.t)

        def bwd():
            if y.g is None:
                return
            self._wait_ready(y)
            dx, add = self.acts.gbuf(x)
            if add is not None and add is not dx:
                raise AozoraError("SiLU input gradient cannot be accumulated out of place")
            ops.silu_bwd(x.t, y.g, dx, accumulate=add is dx)
        self._tape.append(bwd)
        return y

    def attention(self, x: Act, B, T, prefix, ctx: Optional[Act], ctx_len, residual: Act) -> Act:
        C = x.t.shape[1]
        heads = C // self.cfg.head_dim
        scale = 1.0 / math.sqrt(self.cfg.head_dim)
        if ctx is None:
            qkv = self.linear(x, None, None, w_override=self._fused_w([prefix + ".to_q.weight", prefix + ".to_k.weight", prefix + ".to_v.weight"]),
                              lora_mods=[prefix + ".to_q", prefix + ".to_k", prefix + ".to_v"])
            q3 = qkv.t.view(B, T, 3 * C)[..., :C]
            k3 = qkv.t.view(B, T, 3 * C)[..., C:2 * C]
            v3 = qkv.t.view(B, T, 3 * C)[..., 2 * C:]
            Tk, kv_train = T, True
        else:
            q = self.linear(x, prefix + ".to_q.weight", None)
            kv_w = self._fused_w([prefix + ".to_k.weight", prefix + ".to_v.weight"])
            kv_mods = [prefix + ".to_k", prefix + ".to_v"]
            kv_train = kv_w[2] or (self.adapters is not None and self.adapters.trainable(self.adapters.group(kv_mods)))
            kv = self.linear(ctx, None, None, w_override=kv_w, pre=self._hoisted.pop(prefix + ".kv", None), lora_mods=kv_mods)
            q3 = q.t.view(B, T, C)
            k3 = kv.t.view(B, ctx_len, 2 * C)[..., :C]
            v3 = kv.t.view(B, ctx_len, 2 * C)[..., C:]
            Tk = ctx_len
        o = self.acts.new(B * T, C)
        lse = self.acts.pool.get((B * heads * T,), F32)
        ops.attn_fwd(q3, k3, v3, o.t.view(B, T, C), lse, heads, scale)

        def bwd():
            do = o.g
            if do is None:
                return
            delta = self.acts.pool.get((B * heads * T,), F32)
            if ctx is None:
                dqkv = self.acts.gbuf_single(qkv, "attention projections")
                d3 = dqkv.view(B, T, 3 * C)
                dq3, dk3, dv3 = d3[..., :C], d3[..., C:2 * C], d3[..., 2 * C:]
            else:
                dq = self.acts.gbuf_single(q, "attention projections")
                dkv = self.acts.gbuf_single(kv, "attention projections")
                dq3 = dq.view(B, T, C)
                dk3, dv3 = dkv.view(B, ctx_len, 2 * C)[..., :C], dkv.view(B, ctx_len, 2 * C)[..., C:]
            o3, do3 = o.t.view(B, T, C), do.view(B, T, C)
            if ctx is not None and not ctx.need_grad and self.policy.xkv_side:
                # dK / dV of a cross-attention feed only the to_k | to_v weight gradients (the text context has no gradient):
                # the data-gradient chain needs delta + dQ alone; the dK / dV kernel and its ordered reduce go to the
                # parameter-gradient branch in front of that weight gradient (queued later on the same in-order stream), and
                # are not issued at all while to_k | to_v are frozen
                ops.attn_bwd(q3, k3, v3, o3, do3, lse, delta, dq3, dk3, dv3, heads, scale, parts=3)
                if kv_train:
                    self.branch.defer(lambda: ops.attn_bwd(q3, k3, v3, o3, do3, lse, delta, dq3, dk3, dv3, heads, scale, parts=4))
            else:
                ops.attn_bwd(q3, k3, v3, o3, do3, lse, delta, dq3, dk3, dv3, heads, scale)
        self._tape.append(bwd)
        return self.linear(o, prefix + ".to_out.0.weight", prefix + ".to_out.0.bias", residual=residual)

    def geglu(self, proj: Act, pre: Optional[Act] = None) -> Act:
        """pre: the output was already written by the projection's fused epilogue (linear(..., geglu_out=pre))."""
        rows, H2 = proj.t.shape
        if pre is not None:
            y = pre
        else:
            y = self.acts.new(rows, H2 // 2)
            ops.geglu_fwd(proj.t, y.t)

        def bwd():
            if y.g is None:
                return
            dp = self.acts.gbuf_single(proj, "GEGLU projection")
            ops.geglu_bwd(proj.t, y.g, dp)
        self._tape.append(bwd)
        return y

    def _hoist_shared_input_linears(self, blocks, ctx_a: Act, emb_s: Act):
        """The products whose input does not depend on the layer -- attn2.to_k|to_v of the text context (K/V of every
        cross-attention) and time_emb_proj of every ResnetBlock2D -- for the given blocks, as TWO grouped launches instead of
        one small (20 us, launch-bound) GEMM per layer on the chain.  Called once per parameter region, right where the region's
        parameters are known to have landed (data parallel: behind wait_region_params).  Outputs land in self._hoisted."""
        if not self.policy.hoist:
            return
        kv_jobs, te_jobs = [], []
        for kind, pre, n_layers in blocks:
            if kind == "resnet":
                te_jobs.append((pre + ".temb", self._w[pre + ".time_emb_proj.weight"], self._w[pre + ".time_emb_proj.bias"]))
            else:
                for i in range(n_layers):
                    ap = f"{pre}.transformer_blocks.{i}.attn2"
                    kv_jobs.append((ap + ".kv", self._fused_w([ap + ".to_k.weight", ap + ".to_v.weight"])[0], None))
        for a, jobs in ((ctx_a, kv_jobs), (emb_s, te_jobs)):
            if not jobs:
                continue
            rows, K = a.t.shape
            outs = [self.acts.new(rows, W.shape[0]) for _, W, _ in jobs]
            key = (a.t.data_ptr(), rows, K) + tuple((W.data_ptr(), o.t.data_ptr(), b.data_ptr() if b is not None else 0, W.shape[0], W.stride(0),
                                                      o.t.stride(0)) for (_, W, b), o in zip(jobs, outs))
            tab = self._group_tables.get(key)
            if tab is None:
                recs, tiles = [], 0
                for (name, W, b), o in zip(jobs, outs):
                    N = W.shape[0]
                    if W.shape[1] != K or N % 8 or W.stride(0) % 8 or o.t.stride(0) % 8 or W.data_ptr() % 16 or o.t.data_ptr() % 16:
                        raise AozoraError("grouped projection: operand layout")
                    recs.append([W.data_ptr(), o.t.data_ptr(), b.data_ptr() if b is not None else 0, N, W.stride(0), o.t.stride(0), tiles])
                    tiles += (N + 159) // 160
                tab = (torch.tensor(recs, dtype=torch.int64, device=self.device), len(recs), tiles, sum(r[3] for r in recs))
                self._group_tables[key] = tab
            ops.gemm_nt_grouped(a.t, tab[0], tab[1], tab[2], tab[3])
            for (name, _, _), o in zip(jobs, outs):
                self._hoisted[name] = o

    def _region_blocks(self, region):
        """(kind, prefix, transformer layers) of the blocks whose parameters lie in parameter region 0 / 1 / 2, forward order."""
        cfg = self.cfg
        nlev = len(cfg.block_out_channels)
        out = []

        def add_level(pre, n_res, tl):
            for j in range(n_res):
                out.append(("resnet", f"{pre}.resnets.{j}", 0))
                if tl > 0:
                    out.append(("attn", f"{pre}.attentions.{j}", tl))
        if region == 0:
            for i in range(nlev - 1):
                add_level(f"down_blocks.{i}", cfg.layers_per_block, cfg.transformer_layers[i])
        elif region == 1:
            add_level(f"down_blocks.{nlev - 1}", cfg.layers_per_block, cfg.transformer_layers[nlev - 1])
        else:
            out.append(("resnet", "mid_block.resnets.0", 0))
            out.append(("attn", "mid_block.attentions.0", cfg.transformer_layers[-1]))
            out.append(("resnet", "mid_block.resnets.1", 0))
            for i in range(nlev):
                add_level(f"up_blocks.{i}", cfg.layers_per_block + 1, cfg.transformer_layers[nlev - 1 - i])
        return out

    def tblock(self, h: Act, B, T, ctx: Act, ctx_len, pre) -> Act:
        self._tape.append(self.branch.block_end)       # runs AFTER this block's backward: its parameter gradients go out as one batch
        n = self.layernorm(h, pre + ".norm1")
        h = self.attention(n, B, T, pre + ".attn1", None, 0, residual=h)
        n = self.layernorm(h, pre + ".norm2")
        h = self.attention(n, B, T, pre + ".attn2", ctx, ctx_len, residual=h)
        n = self.layernorm(h, pre + ".norm3")
        if self.policy.geglu_fuse:       # the GEGLU rides in the epilogue of its projection (pool order: projection first, output second, as unfused)
            W0 = self._w[pre + ".ff.net.0.proj.weight"]
            p_out = self.acts.new(n.t.shape[0], W0.shape[0])
            g_out = self.acts.new(n.t.shape[0], W0.shape[0] // 2)
            p = self.linear(n, pre + ".ff.net.0.proj.weight", pre + ".ff.net.0.proj.bias", out=p_out, geglu_out=g_out)
            g = self.geglu(p, pre=g_out)
        else:
            p = self.linear(n, pre + ".ff.net.0.proj.weight", pre + ".ff.net.0.proj.bias")
            g = self.geglu(p)
        return self.linear(g, pre + ".ff.net.2.weight", pre + ".ff.net.2.bias", residual=h)

    def transformer(self, x: Act, geom, ctx: Act, ctx_len, pre, n_layers, out: Optional[Act] = None) -> Act:
        B, H, W_ = geom
        self._tape.append(self.branch.block_end)
        n = self.groupnorm(x, geom, pre + ".norm", 1e-6, False)
        h = self.linear(n, pre + ".proj_in.weight", pre + ".proj_in.bias")
        for i in range(n_layers):
            h = self.tblock(h, B, H * W_, ctx, ctx_len, f"{pre}.transformer_blocks.{i}")
        return self.linear(h, pre + ".proj_out.weight", pre + ".proj_out.bias", residual=x, out=out)

    def resnet(self, x: Act, geom, emb_s: Act, pre, out: Optional[Act] = None) -> Act:
        self._tape.append(self.branch.block_end)
        n1 = self.groupnorm(x, geom, pre + ".norm1", 1e-5, True)
        t = self.linear(emb_s, pre + ".time_emb_proj.weight", pre + ".time_emb_proj.bias", pre=self._hoisted.pop(pre + ".temb", None), side_dgrad=True)
        h, _ = self.conv(n1, geom, pre + ".conv1.weight", pre + ".conv1.bias", rowbias=t)
        n2 = self.groupnorm(h, geom, pre + ".norm2", 1e-5, True)
        if (pre + ".conv_shortcut.weight") in self._w:
            wsc = self._w[pre + ".conv_shortcut.weight"]
            gsc = self._gw[pre + ".conv_shortcut.weight"]
            Cout, Cin = wsc.shape[0], wsc.shape[3]
            sc = self.linear(x, None, pre + ".conv_shortcut.bias",
                             w_override=(wsc.view(Cout, Cin), gsc.view(Cout, Cin), self._trainable(pre + ".conv_shortcut.weight")),
                             lora_mods=[pre + ".conv_shortcut"])
        else:
            sc = x
        y, _ = self.conv(n2, geom, pre + ".conv2.weight", pre + ".conv2.bias", residual=sc, out=out)
        return y

    def concat(self, a: Act, b: Act, cat: Optional[Act] = None) -> Act:
        """torch.cat([a, b], dim=channels).  cat: the concatenation's buffer when both halves were WRITTEN IN PLACE by
        their producers (`out=` views handed out by forward(): the up path's activation into the left columns, the down path's
        skip tensor -- which its own consumers read through the row stride -- into the right ones): nothing is copied, the
        concatenation never exists as a separate pass.  Without it (policy.cat_inplace False) the two halves are copied."""
        rows, C1 = a.t.shape
        C2 = b.t.shape[1]
        if cat is not None:
            y = cat
            ld = y.t.stride(0)
            if (tuple(y.t.shape) != (rows, C1 + C2) or a.t.data_ptr() != y.t.data_ptr() or b.t.data_ptr() != y.t.data_ptr() + 2 * C1
                    or a.t.stride(0) != ld or b.t.stride(0) != ld):
                raise AozoraError("in-place concat: the halves are not views of the destination")
        else:
            y = self.acts.new(rows, C1 + C2)
            ops.add_rows(a.t, None, y.t[:, :C1])
            ops.add_rows(b.t, None, y.t[:, C1:])

        def bwd():
            if y.g is None:
                return
            self.acts.give_grad(a, y.g[:, :C1], alias=y.g_alias)      # slices of the concat's gradient (nobody's dY unless y.g is)
            self.acts.give_grad(b, y.g[:, C1:], alias=y.g_alias)
        self._tape.append(bwd)
        return y

    def upsample(self, x: Act, geom, up_to: Optional[Tuple[int, int]] = None) -> Tuple[Act, tuple]:
        """Stand-alone nearest upsample to `up_to` (H, W) (each side 2n or 2n - 1; None: 2x) and its adjoint."""
        B, H, W_ = geom
        C = x.t.shape[1]
        Ho, Wo = up_to if up_to is not None else (2 * H, 2 * W_)
        y = self.acts.new(B * Ho * Wo, C)
        ops.upsample_nearest_fwd(x.t.view(B, H, W_, C), y.t.view(B, Ho, Wo, C))

        def bwd():
            if y.g is None:
                return
            dx = self.acts.gbuf_single(x, "upsample input")
            if not y.g.is_contiguous():
                raise AozoraError("upsample gradient must be contiguous")
            ops.upsample_nearest_bwd(y.g.view(B, Ho, Wo, C), dx.view(B, H, W_, C))
        self._tape.append(bwd)
        return y, (B, Ho, Wo)

    # ------------------------------------------------------------------ whole model ---------------
    def __del__(self):
        try:
            if getattr(self, "branch", None) is not None:
                self.branch.reset_events()
            if getattr(self, "_ctx", None):
                lib()._fn["az_destroy"](self._ctx)
                self._ctx = None
        except Exception:
            pass

    # ------------------------------------------------------------------ activations --------------
    # The activation store (activations.py) under the names callers use; the layers call self.acts directly.
    _pool = property(lambda self: self.acts.pool)                # rebound during a run: read through, never held
    generation = property(lambda self: self.acts.generation)
    def activation_bytes(self) -> dict: return self.acts.activation_bytes()
    def prepare_pool(self, parity) -> int: return self.acts.prepare(parity)
    def wait_pool_free(self, parity): return self.acts.wait_free(parity)
    def has_deferred(self): return self.acts.has_deferred()
    def _arena_of(self, parity) -> _Arena: return self.acts.arena_of(parity)
    def _settle_arena(self, arena: _Arena): return self.acts.settle(arena)

    # The parameter-gradient branch (branch.py) has one switch that callers set on the UNet; the layers call self.branch directly.
    concurrent_wgrad = property(lambda self: self.branch.concurrent, lambda self, on: setattr(self.branch, "concurrent", on))

    def _arena_replaced(self, arena: _Arena):
        """The store replaces `arena` (ActivationStore.settle: the device is synchronised, the arena's pools are dropped, the old
        memory is still held): the executor's own holders of its addresses let go -- the per-step lists, then the launch tapes /
        graphs of the TrainStep objects."""
        self._tape, self._hoisted = [], {}
        self.branch.drop()
        # _group_tables stays, like the branch's pointer tables (GradBranch.drop): recorded launches of the OTHER parity's buckets
        # hold their raw addresses
        for client in list(self.acts.clients):
            client._arena_replaced(arena)

    def check_latent_shape(self, H: int, W: int):
        """Every latent size whose sides hold one pixel per level of the coarsest grid runs (SDXL: H, W >= 4); a side that is no
        multiple of 2**(levels - 1) comes back up through size-targeted upsamples (forward_nhwc).  Smaller ones are refused here,
        before anything is launched."""
        lo = 2 ** (len(self.cfg.block_out_channels) - 1)
        if H < lo or W < lo:
            raise AozoraError(f"latent shape {H}x{W} cannot run: each side must be at least {lo}")

    def begin_step(self, key, lora_step_word: Optional[torch.Tensor] = None):
        """lora_step_word: the device word that holds this step's micro-step for the LoRA dropout masks (TrainStep arms it under a spec
        that has dropout); None = no masks (the drop-in __call__ path never arms one)."""
        lib()._fn["az_make_current"](self._ctx)      # this thread's launches read THIS UNet's option table from here on
        if self.adapters is not None:
            self.adapters.step_word = lora_step_word
        self.acts.begin(key, recording=lib().recorder is not None)
        self.refresh_transposed()
        self._tape = []
        self._hoisted = {}
        self.branch.begin()

    def forward_nhwc(self, x8: torch.Tensor, t_f32: torch.Tensor, ctx: torch.Tensor, pooled: torch.Tensor,
                     time_ids_f32: torch.Tensor) -> Act:
        """x8 (B,H,W,8) bf16 (channels 4..7 zero) ; t_f32 (B,) ; ctx (B,L,ctx_dim) bf16 ; pooled (B,P) bf16 ;
        time_ids_f32 (B,6) fp32 (values already rounded through bf16, train.py:2731). -> pred Act [B*H*W][4]"""
        cfg = self.cfg
        B, H, W_, _ = x8.shape
        self.check_latent_shape(H, W_)
        self._step_B = B              # rows / B = the rows of one sample (rank dropout of an adapter: _adapter_fwd / _adapter_bwd)
        L = ctx.shape[1]
        ch = cfg.block_out_channels
        nlev = len(ch)
        T = cfg.time_embed_dim
        # forward: the data chain has the CUs (and their LDS) to itself (kept so even with deferred weight-gradient work
        # around: measured 0.851 vs 0.835 it/s)
        run_live(lib().call, "az_gemm_set_exclusive", 1)
        # ---- embeddings (a7.1) ----
        tsin = self.acts.new(B, ch[0], need_grad=False)
        ops.timestep_embed(t_f32, ch[0], tsin.t)
        e = self.linear(tsin, "time_embedding.linear_1.weight", "time_embedding.linear_1.bias")
        e = self.silu(e)
        emb_t = self.linear(e, "time_embedding.linear_2.weight", "time_embedding.linear_2.bias")
        idsin = self.acts.new(B * 6, cfg.addition_time_embed_dim, need_grad=False)
        ops.timestep_embed(time_ids_f32.reshape(-1), cfg.addition_time_embed_dim, idsin.t)
        addin = self.acts.new(B, cfg.add_in_dim, need_grad=False)
        ops.add_rows(pooled, None, addin.t[:, :cfg.pooled_dim])
        ops.add_rows(idsin.t.view(B, 6 * cfg.addition_time_embed_dim), None, addin.t[:, cfg.pooled_dim:])
        a = self.linear(addin, "add_embedding.linear_1.weight", "add_embedding.linear_1.bias")
        a = self.silu(a)
        emb = self.linear(a, "add_embedding.linear_2.weight", "add_embedding.linear_2.bias", residual=emb_t)
        emb_s = self.silu(emb)
        ctx_a = Act(ctx.reshape(B * L, ctx.shape[2]), need_grad=False)
        # ---- down ----
        xin = Act(x8.view(B * H * W_, x8.shape[3]), need_grad=False)
        geom = (B, H, W_)
        # Skip concatenations without copies (K14): the s-th skip tensor (push order) is consumed by up-path resnet u = S-1-s, whose
        # other input has C1(u) channels; the [rows][C1 + C2] buffer of that concatenation is allocated when the skip tensor is
        # produced, the producer writes into its right columns, and the up path's producer later writes into the left ones.
        lpb = cfg.layers_per_block
        n_skips = 1 + nlev * lpb + (nlev - 1)
        cats: Dict[int, Act] = {}

        def c1_of(u):
            i, j = divmod(u, lpb + 1)
            lev = nlev - 1 - i
            return ch[lev] if j > 0 else (ch[nlev - 1] if i == 0 else ch[lev + 1])

        def skip_dest(rows, C2):
            """destination view for the next skip tensor (None: plain allocation, copied by concat later)"""
            if not self.policy.cat_inplace:
                return None
            u = n_skips - 1 - len(skips)
            cat = self.acts.new(rows, c1_of(u) + C2)
            cats[u] = cat
            return Act(cat.t[:, c1_of(u):])

        def up_dest(u):
            """destination view for the up-path activation that up-path resnet u concatenates with its skip tensor"""
            cat = cats.get(u)
            return Act(cat.t[:, :c1_of(u)]) if cat is not None else None

        skips: List[Act] = []
        level_geom = [geom]      # geometry of every level on the way down: the up path's upsamplers return to exactly these
        if self.dora is not None:
            # the magnitudes and their gains lie behind conv_out.bias (region 2: updated on the background stream, the norm pass behind it)
            # and are read from the first transformer of the down path on: their region's event is taken up front
            run_live(self.wait_region_params, 2)
        h, _ = self.conv(xin, geom, "conv_in.weight", "conv_in.bias", out=skip_dest(B * H * W_, ch[0]))
        self._hoist_shared_input_linears(self._region_blocks(0), ctx_a, emb_s)
        skips.append(h)
        for i in range(nlev):
            pre = f"down_blocks.{i}"
            if i == nlev - 1:
                self._tape_mark1 = len(self._tape)     # backward entries in [mark1, mark) belong to the last down block (region 1)
                run_live(self.wait_region_params, 1)  # DP overlap: region 1's all-gather must have landed by now
                self._hoist_shared_input_linears(self._region_blocks(1), ctx_a, emb_s)
            rows = geom[0] * geom[1] * geom[2]
            for j in range(lpb):
                if cfg.transformer_layers[i] > 0:
                    h = self.resnet(h, geom, emb_s, f"{pre}.resnets.{j}")
                    h = self.transformer(h, geom, ctx_a, L, f"{pre}.attentions.{j}", cfg.transformer_layers[i], out=skip_dest(rows, ch[i]))
                else:
                    h = self.resnet(h, geom, emb_s, f"{pre}.resnets.{j}", out=skip_dest(rows, ch[i]))
                skips.append(h)
            if i < nlev - 1:
                Hd, Wd = (geom[1] - 1) // 2 + 1, (geom[2] - 1) // 2 + 1      # 3x3, stride 2, pad 1: ceil(side / 2)
                h, geom = self.conv(h, geom, f"{pre}.downsamplers.0.conv.weight", f"{pre}.downsamplers.0.conv.bias", stride=2,
                                    out=skip_dest(geom[0] * Hd * Wd, ch[i]))
                level_geom.append(geom)
                skips.append(h)
        # ---- mid ----
        self._tape_mark = len(self._tape)       # backward entries >= mark belong to mid / up / head-out (the "tail" region)
        run_live(self.wait_region_params, 2)  # DP overlap: the tail parameters' all-gather must have landed by now
        self._hoist_shared_input_linears(self._region_blocks(2), ctx_a, emb_s)
        h = self.resnet(h, geom, emb_s, "mid_block.resnets.0")
        h = self.transformer(h, geom, ctx_a, L, "mid_block.attentions.0", cfg.transformer_layers[-1])
        h = self.resnet(h, geom, emb_s, "mid_block.resnets.1", out=up_dest(0))
        # ---- up ----
        u = 0
        for i in range(nlev):
            lev = nlev - 1 - i
            pre = f"up_blocks.{i}"
            for j in range(lpb + 1):
                h = self.concat(h, skips.pop(), cats.get(u))
                u += 1
                nxt = up_dest(u) if j < lpb else None       # the block's last output feeds the upsampler (or conv_norm_out), not a concat
                if cfg.transformer_layers[lev] > 0:
                    h = self.resnet(h, geom, emb_s, f"{pre}.resnets.{j}")
                    h = self.transformer(h, geom, ctx_a, L, f"{pre}.attentions.{j}", cfg.transformer_layers[lev], out=nxt)
                else:
                    h = self.resnet(h, geom, emb_s, f"{pre}.resnets.{j}", out=nxt)
            if i < nlev - 1:       # Upsample2D: nearest upsample to the geometry of the skip tensor it meets next, folded into the conv's operand gather
                h, geom = self.conv(h, geom, f"{pre}.upsamplers.0.conv.weight", f"{pre}.upsamplers.0.conv.bias", upsample=True, out=up_dest(u),
                                    up_to=level_geom[lev - 1][1:])
        n = self.groupnorm(h, geom, "conv_norm_out", 1e-5, True)
        pred, _ = self.conv(n, geom, "conv_out.weight", "conv_out.bias")
        return pred

    def backward_nhwc(self, pred: Act, dpred8: torch.Tensor, after_tail=None):
        """dpred8 (B,H,W,8) bf16: d(loss)/d(pred), channels >= out_channels zero. Gradients are
        ACCUMULATED into the flat gradient buffer."""
        lib().call("az_gemm_set_exclusive", 0)       # the parameter-gradient stream shares the CUs from here on
        run_live(self._wait_wt_ready)              # an asynchronous W^T refresh must have finished before the first dgrad
        B, H, W_, Cp = dpred8.shape
        pred.g = dpred8.view(B * H * W_, Cp)
        mark, mark1 = self._tape_mark, self._tape_mark1
        self._after_tail_hook = after_tail
        for idx in range(len(self._tape) - 1, -1, -1):
            if idx == mark - 1:
                self.branch.region_end()
                run_live(self._region_hook, 2)   # every gradient of region 2 has been issued (main + side stream)
            if idx == mark1 - 1:
                self.branch.region_end()
                run_live(self._region_hook, 1)   # ... and now those of region 1 (the last down block)
            self._tape[idx]()
        self.branch.region_end()
        self._tape = []
        self.branch.join()      # the parameter-gradient branches, if any was forked (or let them run on)
