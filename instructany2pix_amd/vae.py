"""HIP-backed VAE with the surface the reference uses on diffusers' `AutoencoderKL` (`pipe.vae`):

  vae.encode(image).latent_dist.sample(generator) * vae.config.scaling_factor     img2img `prepare_latents`, reached from
                                                                                   instructany2pix/ddim/pnp_pipeline.py:195-204
  vae.decode(latents / vae.config.scaling_factor, return_dict=False)[0]           instructany2pix/ddim/sdxl_pipeline.py:859-871
  vae.config.{scaling_factor, force_upcast}, vae.dtype

First "next" row of SURVEY.md §8f. All arithmetic runs in libia2p_hip.so (`ia2p_vae_encode` / `ia2p_vae_decode`).
Precision note: the reference upcasts this model to fp32 (`force_upcast`, sdxl_pipeline.py:860-865) because the residual stream of the
original SDXL VAE checkpoint passes the fp16 maximum. The HIP executor keeps fp16 storage (fp32 accumulation and norm statistics) and
extends its range instead: the stream is stored multiplied by `VAEConfig.stream_scale` (2^-7: magnitudes up to 8.4e6), exactly undone by
the GroupNorms (csrc/vae_engine.hip). So `config.force_upcast` reads False (callers need not upcast anything), and every output is checked
for non-finite values: an overflow raises instead of producing black images (tests/test_vae_gpu.py drives both).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import torch

from . import _ffi
from .config import VAEConfig


class DiagonalGaussianDistribution:
    """diffusers' posterior object: parameters = [mean | logvar] along channels, logvar clamped to [-30, 20]."""

    def __init__(self, parameters: torch.Tensor):
        self.parameters = parameters
        self.mean, logvar = torch.chunk(parameters.float(), 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)

    def sample(self, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        dev = generator.device if generator is not None else self.mean.device
        noise = torch.randn(self.mean.shape, generator=generator, device=dev, dtype=torch.float32).to(self.mean.device)
        return (self.mean + self.std * noise).to(self.parameters.dtype)

    def mode(self) -> torch.Tensor:
        return self.mean.to(self.parameters.dtype)


class HipAutoencoderKL(_ffi.Executor):
    dtype = torch.float16

    def __init__(self, config: VAEConfig, device="cuda:0"):
        config.validate()
        self._cfg = config
        self.config = SimpleNamespace(**{**config.__dict__, "force_upcast": False})
        super().__init__("vae", _ffi.make_vae_config(config), device)
        torch.cuda.set_device(self.device)       # process-wide and left set: callers rely on it
        self._factor = 2 ** (len(config.block_out_channels) - 1)

    def load_state_dict(self, state_dict, strict: bool = True):
        items = state_dict.items() if hasattr(state_dict, "items") else state_dict
        torch.cuda.set_device(self.device)
        for k, v in items:
            self.load_tensor(k, v)
        if strict:
            self.finalize()

    def _workspace(self, B, h, w, decode):
        return self.workspace(self._lib.ia2p_vae_workspace_bytes(self._h, B, h, w, int(decode)))

    def max_batch(self, h: int, w: int, decode: bool) -> int:
        """The largest B one encode / decode of h x w latents takes. The executor's kernels address an operand with a 31-bit byte offset and refuse a
        larger one (include/ia2p.h, "Operand size"); the largest operand is the widest full-resolution activation, [B H W, C] fp16: block_out_channels[0]
        channels behind the encoder's conv_in, block_out_channels[1] entering the decoder's last block (SDXL VAE at 1024 x 1024: 7 and 3)."""
        boc = self._cfg.block_out_channels
        ch = boc[min(1, len(boc) - 1)] if decode else boc[0]
        return max(1, (0x7ffffe00 - 1) // (h * self._factor * w * self._factor * ch * 2))

    @torch.no_grad()
    def encode(self, image: torch.Tensor, return_dict: bool = True):
        B, c, H, W = image.shape
        f = self._factor
        if c != self._cfg.in_channels or H % f or W % f:
            raise ValueError(f"image must be [B, {self._cfg.in_channels}, H, W] with H, W divisible by {f}")
        x = image.to(device=self.device, dtype=torch.float16).contiguous()
        h, w = H // f, W // f
        ws = self._workspace(B, h, w, False)
        mom = torch.empty(B, 2 * self._cfg.latent_channels, h, w, dtype=torch.float16, device=self.device)
        self.check(self._lib.ia2p_vae_encode(self._h, _ffi.current_stream(), _ffi.ptr(x), _ffi.ptr(mom), B, h, w, _ffi.ptr(ws), ws.numel()))
        self._check_finite(mom, "encode")
        dist = DiagonalGaussianDistribution(mom)
        return SimpleNamespace(latent_dist=dist) if return_dict else (dist,)

    @torch.no_grad()
    def decode(self, z: torch.Tensor, return_dict: bool = True):
        B, c, h, w = z.shape
        if c != self._cfg.latent_channels:
            raise ValueError(f"latents must have {self._cfg.latent_channels} channels")
        x = z.to(device=self.device, dtype=torch.float16).contiguous()
        f = self._factor
        ws = self._workspace(B, h, w, True)
        img = torch.empty(B, self._cfg.out_channels, h * f, w * f, dtype=torch.float16, device=self.device)
        self.check(self._lib.ia2p_vae_decode(self._h, _ffi.current_stream(), _ffi.ptr(x), _ffi.ptr(img), B, h, w, _ffi.ptr(ws), ws.numel()))
        self._check_finite(img, "decode")
        return SimpleNamespace(sample=img) if return_dict else (img,)

    check_finite = True        # every encode / decode ends with a blocking device-to-host check for non-finite values (an fp16 overflow must not pass
                               # silently where the reference runs fp32); serving loops that check elsewhere may set this to False

    def _check_finite(self, t, what):
        if self.check_finite and not bool(torch.isfinite(t).all()):
            raise _ffi.IA2PError(f"HipAutoencoderKL.{what}: non-finite output -- the activations left the range of fp16 storage at stream_scale="
                                 f"{self._cfg.stream_scale:g} (the reference runs this model in fp32); lower VAEConfig.stream_scale (a power of two)")

    # hooks with the signatures the loops in ddim.py accept (vae_encode= / vae_decode=)
    def encode_to_latents(self, image, generator=None, seeds=None, draw=0):
        """the scaled posterior sample. `seeds` (one per image; None, or every entry None: the draw of `generator` / the global RNG, as ever): image b is sampled
        on the device from its own stream (seeds[b], draw) (noise.py; `ia2p_posterior_sample_seeded`) and wins over `generator`. An image whose entry is None in
        a list that names seeds for others is sampled from `generator` / the global RNG next to them."""
        dist = self.encode(image).latent_dist
        if seeds is None or all(s is None for s in seeds):
            return dist.sample(generator) * self._cfg.scaling_factor
        from . import noise as _noise
        seeds, mom = list(seeds), dist.parameters
        if len(seeds) != mom.shape[0]:
            raise ValueError(f"{len(seeds)} seeds for {mom.shape[0]} images: one per image")
        sf = self._cfg.scaling_factor
        own = [b for b, s in enumerate(seeds) if s is not None]
        if len(own) == len(seeds):
            return _noise.posterior_sample(mom, seeds, draw, sf)
        rest = [b for b, s in enumerate(seeds) if s is None]
        out = torch.empty_like(dist.mean, dtype=mom.dtype)
        out[rest] = DiagonalGaussianDistribution(mom[rest]).sample(generator) * sf
        out[own] = _noise.posterior_sample(mom[own], [seeds[b] for b in own], draw, sf)
        return out

    def decode_from_latents(self, latents):
        return self.decode(latents / self._cfg.scaling_factor, return_dict=False)[0]
