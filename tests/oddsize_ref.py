"""The CPU oracle for latent sizes whose sides are not multiples of 4.

oracle/unet_ref.py upsamples by scale_factor=2, so a level that was halved from an odd side (45 -> 23) comes back one pixel
too large (46) and the skip concatenation raises.  diffusers' UNet2DConditionModel.forward handles that case: when a side of
the sample is not a multiple of 2**num_upsamplers it hands every non-final up block `upsample_size` = the spatial shape of the
next skip tensor, and Upsample2D calls F.interpolate(size=upsample_size, mode="nearest") instead of scale_factor=2.  The
subclass below restates exactly that rule and nothing else; on multiple-of-4 sizes it runs the oracle's own statements
(tests/test_oddsize_cpu.py checks bit identity).  Install it with `trainer.net = OddSizeRefUNet(cfg, trainer.params)`."""
import torch
import torch.nn.functional as F

from oracle.unet_ref import RefUNet


class OddSizeRefUNet(RefUNet):
    def _forward(self, sample, timesteps, ctx, pooled, time_ids):
        cfg = self.cfg
        ch = cfg.block_out_channels
        nlev = len(ch)
        factor = 2 ** (nlev - 1)         # diffusers: default_overall_up_factor = 2 ** num_upsamplers
        sized = any(s % factor != 0 for s in sample.shape[-2:])
        emb = self.embed(timesteps, pooled, time_ids, sample.dtype)
        h = self._conv(sample, "conv_in")
        skips = [h]
        for i in range(nlev):
            pre = f"down_blocks.{i}"
            for j in range(cfg.layers_per_block):
                h = self.resnet(h, emb, f"{pre}.resnets.{j}")
                if cfg.transformer_layers[i] > 0:
                    h = self.transformer(h, ctx, f"{pre}.attentions.{j}", cfg.transformer_layers[i])
                skips.append(h)
            if i < nlev - 1:
                h = self._conv(h, f"{pre}.downsamplers.0.conv", stride=2, pad=1)
                skips.append(h)
        h = self.resnet(h, emb, "mid_block.resnets.0")
        h = self.transformer(h, ctx, "mid_block.attentions.0", cfg.transformer_layers[-1])
        h = self.resnet(h, emb, "mid_block.resnets.1")
        for i in range(nlev):
            lev = nlev - 1 - i
            pre = f"up_blocks.{i}"
            for j in range(cfg.layers_per_block + 1):
                h = torch.cat([h, skips.pop()], dim=1)
                h = self.resnet(h, emb, f"{pre}.resnets.{j}")
                if cfg.transformer_layers[lev] > 0:
                    h = self.transformer(h, ctx, f"{pre}.attentions.{j}", cfg.transformer_layers[lev])
            if i < nlev - 1:
                if sized:      # upsample_size = down_block_res_samples[-1].shape[2:]
                    h = F.interpolate(h, size=tuple(skips[-1].shape[2:]), mode="nearest")
                else:
                    h = F.interpolate(h, scale_factor=2.0, mode="nearest")
                h = self._conv(h, f"{pre}.upsamplers.0.conv")
        h = F.silu(self._gn(h, "conv_norm_out", 1e-5))
        return self._conv(h, "conv_out")


def cropped_fold(dy: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """The adjoint of nearest upsampling (B,C,H,W) -> (B,C,Ho,Wo), Ho in {2H-1, 2H}, Wo in {2W-1, 2W}, written as the 2x2 fold
    the kernel computes: source pixel (y, x) sums dy[2y + a][2x + b] over the a, b in {0, 1} that lie inside the target, in
    dy-row-major order, in fp32."""
    B, C, Ho, Wo = dy.shape
    assert Ho in (2 * H - 1, 2 * H) and Wo in (2 * W - 1, 2 * W)
    full = torch.zeros(B, C, 2 * H, 2 * W, dtype=torch.float32)
    full[:, :, :Ho, :Wo] = dy.float()
    out = torch.zeros(B, C, H, W, dtype=torch.float32)
    for a in range(2):
        for b in range(2):
            out = out + full[:, :, a::2, b::2]
    return out
