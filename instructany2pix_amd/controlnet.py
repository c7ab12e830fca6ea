"""HIP-backed ControlNet with the call surface of diffusers' `ControlNetModel` (0.26.3), as `StableDiffusionXLControlNetPipeline` drives it.

The reference attaches no ControlNet; it prepares the seam: `IPAdapter.set_ip_adapter` installs `CNAttnProcessor` on `pipe.controlnet` when the pipe has one
(instructany2pix/diffusion/ip_adapter/ip_adapter.py:143-148), and that processor's only job is to cut the image tokens off the context
(`encoder_hidden_states[:, :end_pos]`, attention_processor.py:530-531). Here: `set_image_tokens(num_tokens)`.

    down, mid = controlnet(sample, t, encoder_hidden_states=ctx, controlnet_cond=image, conditioning_scale=s,
                           added_cond_kwargs={...}, return_dict=False)
    eps = unet(sample, t, encoder_hidden_states=ctx, added_cond_kwargs={...},
               down_block_additional_residuals=down, mid_block_additional_residual=mid)[0]

All arithmetic runs in libia2p_hip.so (`ia2p_controlnet_*`): the UNet executor's down path and mid block under a second arena, the condition embedding
(`ia2p_controlnet_embed`, once per condition image) and the zero convolutions with the conditioning scale in their epilogue. No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Dict, Iterable, Optional, Tuple, Union

import torch

from . import _ffi
from .config import ControlNetConfig
from .unet import _inputs, per_row


class HipControlNetModel(_ffi.Executor):
    dtype = torch.float16

    def __init__(self, config: ControlNetConfig, device: Union[str, torch.device] = "cuda:0"):
        config.validate()
        self.config = config
        super().__init__("controlnet", _ffi.make_controlnet_config(config), device)
        self.num_tokens = 0                 # trailing image-token rows of the contexts this model is handed (set_image_tokens)
        self.cache_context_kv = True
        self._kv = None                     # (context tensor kept alive, its _version, num_tokens, weight generation, (B, L), kv buffer)
        self._weights_gen = 0
        self._cond = None                   # (condition tensor kept alive, its _version, weight generation, embedded condition)
        self._ws_key = None
        self._res = None                    # the residual buffer: the returned tensors view it

    # ---- weights --------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict: Union[Dict[str, torch.Tensor], Iterable[Tuple[str, torch.Tensor]]], strict: bool = True):
        """Load parameters by diffusers key (`weights.controlnet_param_specs` names them); a dict or an iterator of (key, tensor)."""
        items = state_dict.items() if hasattr(state_dict, "items") else state_dict
        for k, v in items:
            self._weights_gen += 1
            self.load_tensor(k, v)
        torch.cuda.synchronize(self.device)
        if strict:
            self.finalize()

    def set_image_tokens(self, num_tokens: int):
        """The contexts end in `num_tokens` image-token rows (an IP-Adapter pipe): this model attends to the text rows in front of them only."""
        self.check(self._lib.ia2p_controlnet_set_image_tokens(self._h, int(num_tokens)))
        self.num_tokens = int(num_tokens)

    def check_unet(self, unet):
        """ValueError unless this ControlNet's residuals fit `unet`'s skips (block_out_channels, layers_per_block, cross_attention_dim)."""
        self.check(self._lib.ia2p_controlnet_check_unet(self._h, unet._ctx))

    def set_gn_fuse(self, mode: int):
        self.check(self._lib.ia2p_set_gn_fuse(self._h, int(mode)))

    # ---- condition embedding ------------------------------------------------------------------------------------------
    @_ffi.on_device
    def embed_condition(self, image: torch.Tensor) -> torch.Tensor:
        """image [B, 3, 8 h, 8 w] in [0, 1] -> the embedded condition on the latent grid, channels-last [B, h, w, block_out_channels[0]]. Depends on the image and the
        weights only: compute it once per request and hand it to `__call__` as `controlnet_cond` (a 4-d tensor whose last dimension is block_out_channels[0] and
        whose second is not `conditioning_channels` is taken as embedded)."""
        if image.ndim != 4 or image.shape[1] != self.config.conditioning_channels or image.shape[2] % 8 or image.shape[3] % 8 or image.shape[2] < 8 or image.shape[3] < 8:
            raise ValueError(f"the condition image must be [B, {self.config.conditioning_channels}, 8 h, 8 w]; got {tuple(image.shape)}")
        B, _, H, W = image.shape
        h, w = H // 8, W // 8
        img = image.to(device=self.device, dtype=torch.float16).contiguous()
        out = torch.empty(B, h, w, self.config.block_out_channels[0], dtype=torch.float16, device=self.device)
        n = self._lib.ia2p_controlnet_embed_bytes(self._h, B, h, w)
        ws = self.workspace(self._lib.ia2p_controlnet_embed_workspace_bytes(self._h, B, h, w))
        self._ws_key = None
        self.check(self._lib.ia2p_controlnet_embed(self._h, _ffi.current_stream(), _ffi.ptr(img), B, h, w, _ffi.ptr(out), n, _ffi.ptr(ws), ws.numel()))
        return out

    def _embedded(self, cond, B, h, w):
        C0 = self.config.block_out_channels[0]
        if cond.ndim == 4 and tuple(cond.shape[1:]) == (h, w, C0) and cond.shape[1] != self.config.conditioning_channels:
            e = cond.to(device=self.device, dtype=torch.float16).contiguous()
        else:
            if cond.ndim != 4 or tuple(cond.shape[2:]) != (8 * h, 8 * w):
                raise ValueError(f"controlnet_cond must be [B, {self.config.conditioning_channels}, {8 * h}, {8 * w}] for a {h} x {w} latent; got {tuple(cond.shape)}")
            k = self._cond
            if k is not None and k[0] is cond and k[1] == cond._version and k[2] == self._weights_gen:
                e = k[3]
            else:
                e = self.embed_condition(cond)
                self._cond = (cond, cond._version, self._weights_gen, e)
        if e.shape[0] != B:
            if B % e.shape[0]:
                raise ValueError(f"controlnet_cond holds {e.shape[0]} images for a batch of {B}")
            e = e.repeat(B // e.shape[0], 1, 1, 1)      # (classifier-free guidance: the condition is repeated for both halves)
        return e

    # ---- forward ------------------------------------------------------------------------------------------------------
    def residual_layout(self, B: int, h: int, w: int):
        n = self._lib.ia2p_controlnet_num_residuals(self._h)
        offs, ch, hs, ws = (C.c_int64 * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        total = self._lib.ia2p_controlnet_residual_layout(self._h, B, h, w, offs, ch, hs, ws)
        if total == 0:
            self.check(2)
        return total, [(int(offs[k]), int(ch[k]), int(hs[k]), int(ws[k])) for k in range(n)]

    @_ffi.on_device
    def __call__(self, sample, timestep, encoder_hidden_states=None, controlnet_cond=None, conditioning_scale=1.0, added_cond_kwargs=None,
                 guess_mode: bool = False, return_dict: bool = False, **unused):
        """-> (down_block_res_samples, mid_block_res_sample): logical-NCHW tensors with channels-last strides that VIEW this model's residual buffer (no copy; the next
        call overwrites them). `conditioning_scale`: a number, or a [B] tensor -- one scale per batch element. `timestep`: a number or a [B] tensor."""
        if guess_mode:
            raise ValueError("guess_mode=True is not supported")
        if controlnet_cond is None:
            raise ValueError("controlnet_cond is required")
        ctx_in = encoder_hidden_states
        sample, ctx, te, tid, (B, h, w, L) = _inputs(self, sample, encoder_hidden_states, added_cond_kwargs)
        if L <= self.num_tokens:
            raise ValueError(f"a context of {L} rows leaves no text rows in front of the {self.num_tokens} image tokens")
        cond = self._embedded(controlnet_cond, B, h, w)
        ts, sc = per_row(timestep, B, "timestep tensor", self.device), per_row(conditioning_scale, B, "conditioning_scale", self.device)
        key = (B, h, w, L, self.num_tokens, self._lib.ia2p_plan_generation())
        if self._ws_key != key:
            self.workspace(self._lib.ia2p_controlnet_workspace_bytes(self._h, B, h, w, L))
            self._ws_key = key
        ws = self._ws
        total, layout = self.residual_layout(B, h, w)
        if self._res is None or self._res.numel() * 2 != total:
            self._res = torch.empty(total // 2, dtype=torch.float16, device=self.device)
        res = self._res
        kv = None
        if self.cache_context_kv:
            kv = self._context_kv(self.num_tokens, self._lib.ia2p_controlnet_context_kv_bytes, self._lib.ia2p_controlnet_project_context, ctx_in, ctx, B, L, ws)
        self.check(self._lib.ia2p_controlnet_forward(self._h, _ffi.current_stream(), _ffi.ptr(sample), _ffi.ptr(ts), None if kv is not None else _ffi.ptr(ctx),
                                                     _ffi.ptr(kv) if kv is not None else None, L, _ffi.ptr(te), _ffi.ptr(tid), _ffi.ptr(cond), _ffi.ptr(sc),
                                                     _ffi.ptr(res), total, B, h, w, _ffi.ptr(ws), ws.numel()))
        views = [res[o:o + B * hh * ww * c].view(B, hh, ww, c).permute(0, 3, 1, 2) for o, c, hh, ww in layout]
        down, mid = views[:-1], views[-1]
        if return_dict:
            return SimpleNamespace(down_block_res_samples=down, mid_block_res_sample=mid)
        return down, mid


def build_controlnet(config: ControlNetConfig, state_dict=None, device="cuda:0") -> HipControlNetModel:
    m = HipControlNetModel(config, device)
    if state_dict is not None:
        m.load_state_dict(state_dict)
    return m
