"""ControlNet for the SDXL UNet, restated from diffusers 0.26.3 (`ControlNetModel`, `StableDiffusionXLControlNetPipeline`) on the modules of oracle.unet_ref. diffusers is
not installed next to this project (as for the UNet itself), so parity with it is NOT pinned by a test: this file and DESIGN.md §21 are the statement of the semantics.

  config      the UNet config + conditioning_channels = 3, conditioning_embedding_out_channels = (16, 32, 96, 256); no up path, no conv_norm_out / conv_out
  keys        the UNet's own for conv_in, time_embedding, add_embedding, down_blocks.*, mid_block.*; controlnet_cond_embedding.{conv_in, blocks.0..5, conv_out};
              controlnet_down_blocks.{k} (1x1, one per skip, skip order); controlnet_mid_block
  embedding   all 3x3, pad 1, bias: silu(conv_in 3 -> c0); for i < 3: silu(blocks[2i]: c_i -> c_i, stride 1), silu(blocks[2i+1]: c_i -> c_(i+1), stride 2); conv_out
              c3 -> block_out_channels[0], no activation. Input RGB in [0, 1], [B, 3, 8h, 8w]; output on the latent grid
  forward     x = conv_in(sample) + cond_embedding; embedding, down path, mid block exactly the UNet's, over the TEXT rows of the context only (L - num_tokens rows: the
              rule of the reference's CNAttnProcessor, attention_processor.py:530-531); residual k = zero_conv_k(skip_k) * conditioning_scale, the mid one likewise
  UNet side   skip_k += residual_k after the whole down path has run (the hidden state flowing down is the unmodified one); mid_out += mid_residual
  loop        with CFG the condition is repeated for both halves; step i of n runs the ControlNet iff not (i / n < start or (i + 1) / n > end)
"""
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.unet_ref import UNet2DConditionModelRef, sinusoid  # noqa: E402


def control_active(i, n, start, end):
    """diffusers: controlnet_keep[i] = 1.0 - float(i / n < start or (i + 1) / n > end)"""
    return not (i / n < start or (i + 1) / n > end)


class ControlNetConditioningEmbeddingRef(nn.Module):
    def __init__(self, out_channels, cond_channels=3, widths=(16, 32, 96, 256)):
        super().__init__()
        self.conv_in = nn.Conv2d(cond_channels, widths[0], 3, padding=1)
        blocks = []
        for i in range(len(widths) - 1):
            blocks.append(nn.Conv2d(widths[i], widths[i], 3, padding=1))
            blocks.append(nn.Conv2d(widths[i], widths[i + 1], 3, padding=1, stride=2))
        self.blocks = nn.ModuleList(blocks)
        self.conv_out = nn.Conv2d(widths[-1], out_channels, 3, padding=1)

    def forward(self, x):
        x = F.silu(self.conv_in(x))
        for b in self.blocks:
            x = F.silu(b(x))
        return self.conv_out(x)


def _embeddings(m, cfg, sample, timestep, added_cond_kwargs):
    b = sample.shape[0]
    t = torch.as_tensor(timestep, device=sample.device).reshape(-1).expand(b)
    emb = m.time_embedding(sinusoid(t, cfg.time_proj_dim).to(sample.dtype))
    text_embeds, time_ids = added_cond_kwargs["text_embeds"], added_cond_kwargs["time_ids"]
    tid = sinusoid(time_ids.flatten(), cfg.addition_time_embed_dim).reshape(b, -1)
    return emb + m.add_embedding(torch.cat([text_embeds, tid.to(text_embeds.dtype)], dim=-1).to(emb.dtype))


def _down_and_mid(m, x, emb, ctx):
    """the UNet's down path and mid block on modules of `m` -> (skips, mid output)"""
    skips = [x]
    for blk in m.down_blocks:
        for j, res in enumerate(blk.resnets):
            x = res(x, emb)
            if hasattr(blk, "attentions"):
                x = blk.attentions[j](x, ctx)
            skips.append(x)
        if hasattr(blk, "downsamplers"):
            x = blk.downsamplers[0](x)
            skips.append(x)
    x = m.mid_block.resnets[0](x, emb)
    x = m.mid_block.attentions[0](x, ctx)
    x = m.mid_block.resnets[1](x, emb)
    return skips, x


class ControlNetRef(nn.Module):
    """the UNet's own conv_in, embeddings, down path and mid block (the modules of a UNet2DConditionModelRef of the same config, its up path dropped) + the condition
    embedding + the zero convolutions"""

    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        u = UNet2DConditionModelRef(cfg)
        self.conv_in, self.time_embedding, self.add_embedding, self.down_blocks, self.mid_block = u.conv_in, u.time_embedding, u.add_embedding, u.down_blocks, u.mid_block
        ch = list(cfg.block_out_channels)
        self.controlnet_cond_embedding = ControlNetConditioningEmbeddingRef(ch[0], cfg.conditioning_channels, tuple(cfg.conditioning_embedding_out_channels))
        skip = [ch[0]]
        for i in range(len(ch)):
            skip += [ch[i]] * cfg.layers_per_block
            if i != len(ch) - 1:
                skip.append(ch[i])
        self.controlnet_down_blocks = nn.ModuleList([nn.Conv2d(c, c, 1) for c in skip])
        self.controlnet_mid_block = nn.Conv2d(ch[-1], ch[-1], 1)
        self.num_tokens = 0

    def forward(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale=1.0, added_cond_kwargs=None, guess_mode=False, return_dict=False):
        if guess_mode:
            raise ValueError("guess_mode=True is not restated")
        L = encoder_hidden_states.shape[1]
        ctx = encoder_hidden_states[:, :L - self.num_tokens]
        emb = _embeddings(self, self.config, sample, timestep, added_cond_kwargs)
        x = self.conv_in(sample) + self.controlnet_cond_embedding(controlnet_cond)
        skips, mid = _down_and_mid(self, x, emb, ctx)
        s = torch.as_tensor(conditioning_scale, dtype=sample.dtype).reshape(-1, 1, 1, 1)      # one number, or one per batch element
        return [z(k) * s for z, k in zip(self.controlnet_down_blocks, skips)], self.controlnet_mid_block(mid) * s


class UNetWithResidualsRef(UNet2DConditionModelRef):
    """UNet2DConditionModelRef.forward with diffusers' `down_block_additional_residuals` / `mid_block_additional_residual` (oracle/ cannot change: the forward is
    restated here from the same pieces)"""

    def forward(self, sample, timestep, encoder_hidden_states, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False,
                down_block_additional_residuals=None, mid_block_additional_residual=None):
        emb = _embeddings(self, self.config, sample, timestep, added_cond_kwargs)
        ctx = encoder_hidden_states
        skips, x = _down_and_mid(self, self.conv_in(sample), emb, ctx)
        if down_block_additional_residuals is not None:
            assert len(down_block_additional_residuals) == len(skips)
            skips = [s + r for s, r in zip(skips, down_block_additional_residuals)]
        if mid_block_additional_residual is not None:
            x = x + mid_block_additional_residual
        for blk in self.up_blocks:
            for j, res in enumerate(blk.resnets):
                x = res(torch.cat([x, skips.pop()], dim=1), emb)
                if hasattr(blk, "attentions"):
                    x = blk.attentions[j](x, ctx)
            if hasattr(blk, "upsamplers"):
                x = blk.upsamplers[0](x)
        return (self.conv_out(F.silu(self.conv_norm_out(x))),)


def build_unet_with_residuals(cfg, state_dict, ip_state=None, ip_scale=1.0, num_tokens=4):
    """oracle.build_unet for the subclass"""
    from oracle.attn_processors_ref import AttnProcessor2_0Ref, IPAttnProcessor2_0Ref
    m = UNetWithResidualsRef(cfg)
    m.load_state_dict({k: v.float() for k, v in state_dict.items()}, strict=True)
    if ip_state is not None:
        procs = {}
        for name in m.attn_processors.keys():
            if name.endswith("attn1.processor"):
                procs[name] = AttnProcessor2_0Ref()
                continue
            hs = cfg.block_out_channels[-1] if name.startswith("mid_block") else (list(reversed(cfg.block_out_channels))[int(name[len("up_blocks."):].split(".")[0])]
                                                                               if name.startswith("up_blocks") else cfg.block_out_channels[int(name[len("down_blocks."):].split(".")[0])])
            procs[name] = IPAttnProcessor2_0Ref(hs, cfg.cross_attention_dim, scale=ip_scale, num_tokens=num_tokens)
        m.set_attn_processor(procs)
        torch.nn.ModuleList(m.attn_processors.values()).load_state_dict({k: v.float() for k, v in ip_state.items()})
    return m.eval()


def build_controlnet(cfg, state_dict, num_tokens=0):
    m = ControlNetRef(cfg)
    m.load_state_dict({k: v.float() for k, v in state_dict.items()}, strict=True)
    m.num_tokens = num_tokens
    return m.eval()


class ControlledRef:
    """the (ControlNet, UNet) pair behind the plain `unet(x, t, encoder_hidden_states=, added_cond_kwargs=)` signature, so that oracle.sample_loop runs the controlled
    loop unchanged: evaluation i of n runs the ControlNet iff control_active(i, n, start, end); the condition is repeated over the batch (CFG halves)"""

    def __init__(self, unet, controlnet, cond, scale, start, end, n):
        self.unet, self.controlnet, self.cond, self.scale, self.window, self.n, self.calls = unet, controlnet, cond, scale, (start, end), n, 0

    def __call__(self, x, t, encoder_hidden_states=None, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False):
        i, self.calls = self.calls, self.calls + 1
        if not control_active(i, self.n, *self.window):
            return self.unet(x, t, encoder_hidden_states, added_cond_kwargs=added_cond_kwargs)
        cond = self.cond.repeat(x.shape[0] // self.cond.shape[0], 1, 1, 1)
        down, mid = self.controlnet(x, t, encoder_hidden_states, cond, self.scale, added_cond_kwargs=added_cond_kwargs)
        return self.unet(x, t, encoder_hidden_states, added_cond_kwargs=added_cond_kwargs, down_block_additional_residuals=down, mid_block_additional_residual=mid)
