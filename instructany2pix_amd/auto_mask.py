"""Automatic edit masks (the rule is in include/ia2p.h, "Automatic edit mask"; kernels: csrc/auto_mask.hip).

Nobody draws a mask for "make the fox blue". The estimator noises the base latents n times at one level of the request's own schedule, asks the UNet for the
noise under the base condition (one inversion evaluation: the '' context) and under the edit's condition (the conditional half of one sampling evaluation: prompt
embeddings + IP tokens), and marks the cells where the two answers differ by more than `ratio / 2` times their mean difference (the DiffEdit construction),
grown by `dilate` cells. The result is a {0, 1} latent mask [1, 1, h, w] on the device that `pipeline.resolve_edit_mask` accepts: everything after it is the
existing edit-mask path.

  AutoMask(num_maps, strength, ratio, dilate, noise, max_rows)   the knobs; `resolve_auto_mask` turns True / a dict / an AutoMask into one
  contrast_map(eps_tgt, eps_src) / contrast_mask(map, ...)        the two launches (`ia2p_eps_contrast_map`, `ia2p_contrast_mask`)
  estimate_noises(...)                                            the host draws of the unseeded requests, in request order
  estimate_group(pipeline, reqs, knobs, noises, max_rows)         ONE group of requests through both evaluations: the stage both serving paths share
  estimate_requests(pipeline, requests, group, max_rows)          a list of `batch.EditRequest`s: draws, then groups -> one AutoMaskEstimate (or None) each
  estimate_edit_mask(pipeline, base_latents, latent_la, ...)      one request on explicit conditioning: a group of one
  apply_auto_masks(pipeline, requests, group)                     `denoise_batch`: requests with `auto_mask` -> copies whose `edit_mask` carries the result
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import _ffi
from . import noise as _noise
from .scheduler import DDIMScheduler, check_kept_steps, fused_update_v, kept_steps

MAX_DILATE = 16          # latent cells (`ia2p_contrast_mask` refuses more)
MAX_MAPS = 64
MAX_ROWS = 16            # rows of one UNet evaluation (B_eff = 2 x 8, the limit of the embedding kernels)


@dataclass(frozen=True)
class AutoMask:
    """The knobs of one request's mask estimate. `noise`: the n noises [num_maps, C, h, w] themselves (wins over the request's seed and the global generator);
    `max_rows`: rows per UNet evaluation (None: num_maps in a serial call, 2 x group in a batched one -- what the guided loop runs at anyway)."""
    num_maps: int = 8
    strength: float = 0.5
    ratio: float = 3.0
    dilate: int = 1
    noise: Optional[torch.Tensor] = None
    max_rows: Optional[int] = None

    def __post_init__(self):
        self.check()

    def check(self, who: str = ""):
        n, d, r = self.num_maps, self.dilate, self.max_rows
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= MAX_MAPS:
            raise ValueError(f"auto_mask: num_maps={n!r} must be an integer in 1 .. {MAX_MAPS}{who}")
        if isinstance(self.strength, bool) or not isinstance(self.strength, (int, float)) or not 0.0 <= float(self.strength) <= 1.0:      # (NaN fails both comparisons)
            raise ValueError(f"auto_mask: The value of strength should in [0.0, 1.0] but is {self.strength!r}{who}")
        if isinstance(self.ratio, bool) or not isinstance(self.ratio, (int, float)) or not (math.isfinite(self.ratio) and self.ratio > 0):
            raise ValueError(f"auto_mask: ratio={self.ratio!r} must be finite and positive{who}")
        if isinstance(d, bool) or not isinstance(d, int) or not 0 <= d <= MAX_DILATE:
            raise ValueError(f"auto_mask: dilate={d!r} must be an integer in 0 .. {MAX_DILATE} latent cells{who}")
        if r is not None and (isinstance(r, bool) or not isinstance(r, int) or not 1 <= r <= MAX_ROWS):
            raise ValueError(f"auto_mask: max_rows={r!r} must be None or an integer in 1 .. {MAX_ROWS}{who}")
        if self.noise is not None and (not torch.is_tensor(self.noise) or self.noise.ndim != 4 or self.noise.shape[0] != n):
            raise ValueError(f"auto_mask: noise must be a tensor [num_maps = {n}, C, h, w]{who}")


def resolve_auto_mask(value, who: str = "") -> Optional[AutoMask]:
    """`auto_mask=` of every entry point -> AutoMask or None (off): None / False -> None, True -> the defaults, a dict -> its keyword arguments, an AutoMask -> itself.
    `who` names the request where several share a call."""
    if value is None or value is False:
        return None
    if value is True:
        return AutoMask()
    if isinstance(value, AutoMask):
        return value
    if isinstance(value, dict):
        unknown = sorted(set(value) - {f.name for f in dataclasses.fields(AutoMask)})
        if unknown:
            raise ValueError(f"auto_mask: unknown keys {unknown}{who}")
        a = AutoMask.__new__(AutoMask)
        for f in dataclasses.fields(AutoMask):
            object.__setattr__(a, f.name, value.get(f.name, f.default))
        a.check(who)
        return a
    raise ValueError(f"auto_mask must be None, True, a dict of AutoMask's fields or an AutoMask, got {type(value).__name__}{who}")


def auto_mask_t_start(num_inference_steps: int, strength: float, who: str = "") -> int:
    """index of the estimate's noise level in the request's own schedule: `t_start` of `scheduler.kept_steps`; a strength that keeps no step is refused in
    `check_kept_steps`'s words. Pure host arithmetic: every entry point calls it before anything runs."""
    if num_inference_steps is None or isinstance(num_inference_steps, bool) or not isinstance(num_inference_steps, int) or num_inference_steps <= 0:
        raise ValueError(f"`num_inference_steps` has to be a positive integer but is {num_inference_steps}{who}")
    t_start, kept = kept_steps(num_inference_steps, float(strength))
    check_kept_steps(kept, strength, who)
    return t_start


def auto_mask_timestep(scheduler_config, num_inference_steps: int, strength: float, who: str = "") -> int:
    """the noise level of the estimate: `timesteps[t_start]` of the request's own DDIM schedule"""
    t_start = auto_mask_t_start(num_inference_steps, strength, who)
    sch = DDIMScheduler.from_config(scheduler_config)
    sch.set_timesteps(num_inference_steps)
    return int(sch.timesteps[t_start])


# ---- the two launches -------------------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def contrast_map(eps_tgt: torch.Tensor, eps_src: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp16 [B, n, C, h, w] x 2 on the device -> fp32 [B, h, w]: the mean absolute difference over (k, c), k outer (`ia2p_eps_contrast_map`)"""
    for t in (eps_tgt, eps_src):
        if t.dtype != torch.float16 or not t.is_cuda or t.ndim != 5:
            raise ValueError("contrast_map takes fp16 device tensors [B, n, C, h, w]")
    if eps_tgt.shape != eps_src.shape:
        raise ValueError(f"eps_tgt {tuple(eps_tgt.shape)} and eps_src {tuple(eps_src.shape)} must have one shape")
    eps_tgt, eps_src = eps_tgt.contiguous(), eps_src.contiguous()
    B, n, Cc, h, w = eps_tgt.shape
    if out is None:
        out = torch.empty(B, h, w, dtype=torch.float32, device=eps_tgt.device)
    elif out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (B, h, w):
        raise ValueError(f"out must be a contiguous fp32 device tensor [{B}, {h}, {w}]")
    with torch.cuda.device(eps_tgt.device):
        _ffi.check(_ffi.lib().ia2p_eps_contrast_map(_ffi.current_stream(), _ffi.ptr(eps_tgt), _ffi.ptr(eps_src), _ffi.ptr(out), B, n, Cc, h * w))
    return out


@torch.no_grad()
def contrast_mask(cmap: torch.Tensor, ratios, dilates) -> tuple:
    """fp32 [B, h, w] on the device -> ({0, 1} latent masks fp16 [B, 1, h, w], stats fp32 [B, 2] = (mean, tau)) (`ia2p_contrast_mask`). `ratios` / `dilates`: one value for
    every request or a list of B; they travel by value."""
    if cmap.dtype != torch.float32 or not cmap.is_cuda or cmap.ndim != 3:
        raise ValueError("contrast_mask takes an fp32 device tensor [B, h, w]")
    cmap = cmap.contiguous()
    B, h, w = cmap.shape
    ratios = [float(ratios)] * B if not isinstance(ratios, (list, tuple)) else [float(r) for r in ratios]
    dilates = [int(dilates)] * B if not isinstance(dilates, (list, tuple)) else [int(d) for d in dilates]
    if len(ratios) != B or len(dilates) != B:
        raise ValueError(f"{len(ratios)} ratios and {len(dilates)} dilations for {B} maps")
    mask = torch.empty(B, 1, h, w, dtype=torch.float16, device=cmap.device)
    stats = torch.empty(B, 2, dtype=torch.float32, device=cmap.device)
    with torch.cuda.device(cmap.device):
        _ffi.check(_ffi.lib().ia2p_contrast_mask(_ffi.current_stream(), _ffi.ptr(cmap), (C.c_float * B)(*ratios), (C.c_int * B)(*dilates), _ffi.ptr(mask),
                                                 _ffi.ptr(stats), B, h, w))
    return mask, stats


# ---- the host stage ---------------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class AutoMaskEstimate:
    mask: torch.Tensor       # {0, 1} latent mask fp16 [1, 1, h, w]
    map: torch.Tensor        # contrast map fp32 [1, h, w]
    stats: torch.Tensor      # fp32 [2] = (mean, tau)
    timestep: int


def estimate_noises(knobs: Sequence[Optional[AutoMask]], latents: Sequence[torch.Tensor], seeds: Sequence[Optional[int]]) -> list:
    """Step 2 of the rule on the host, per request in REQUEST order: a supplied `noise` wins; a request with a seed is left None (its noises are made on the device
    from draw DRAW_AUTO_MASK of its own stream) and draws NOTHING here; every other request with a knob draws ONE `torch.randn(n, C, h, w, dtype=float16)` from
    torch's global CPU generator. A request without a knob (None) draws nothing."""
    out = []
    for i, (a, x, s) in enumerate(zip(knobs, latents, seeds)):
        if a is None:
            out.append(None)
            continue
        shape = (a.num_maps,) + tuple(x.shape[1:])
        if a.noise is not None:
            if tuple(a.noise.shape) != shape:
                raise ValueError(f"auto_mask: noise is {tuple(a.noise.shape)}, expected {shape} (request {i})")
            out.append(a.noise)
        elif s is not None:
            out.append(None)
        else:
            out.append(torch.randn(shape, dtype=torch.float16))
    return out


@torch.no_grad()
def estimate_group(pipeline, reqs: list, knobs: List[AutoMask], noises: list, max_rows: int) -> List[AutoMaskEstimate]:
    """One group of `batch.EditRequest`s (every one with a knob) through steps 2 - 7 of the rule. The requests' rows are laid end to end, request r's n_r rows at its
    own timestep; the two evaluations go through the UNet in chunks of at most `max_rows` rows:
      eps_src: the inversion context ('' embeddings, else the negative ones), its pooled embedding and time ids, NO per-row IP scale -- what `inverse` /
               `invert_batch` hand the UNet, under the scale the processors hold;
      eps_tgt: cat([prompt embeddings, IP tokens of latent_la]), the request's `scale` per row -- the conditional half of `generate` / `sample_batch`.
    `noises[i]` None: the request's n noises are draw DRAW_AUTO_MASK of its own stream, made on the device."""
    from .ddim import conditioning, get_add_time_ids
    unet, ipa, cfg = pipeline.pipe.unet, pipeline.ip_adapter_xl, pipeline.pipe.scheduler.config
    if ipa is None:
        raise NotImplementedError("the mask estimate drives the IP-Adapter path (construct the pipeline with ip_ckpt=)")
    dev = unet.device
    f16 = lambda t: t.to(device=dev, dtype=torch.float16)
    ns = [a.num_maps for a in knobs]
    ts = [auto_mask_timestep(cfg, int(r.num_inference_steps), a.strength) for r, a in zip(reqs, knobs)]
    rep = lambda xs: torch.cat([f16(x).expand(n, *x.shape[1:]) for x, n in zip(xs, ns)], dim=0).contiguous()      # request r's [1, ...] tensor on its n_r rows
    if any(r.base_latents.ndim != 4 or int(r.base_latents.shape[0]) != 1 for r in reqs):
        raise ValueError("auto_mask estimates one mask for ONE base image: base_latents must be [1, C, h, w]")
    x0 = rep([r.base_latents for r in reqs])
    R, (Cc, h, w) = x0.shape[0], x0.shape[1:]
    own = [i for i, z in enumerate(noises) if z is None]
    z = torch.empty_like(x0)
    starts = [sum(ns[:i]) for i in range(len(reqs))]
    for i in own:                    # element k per + e of the draw: noise k, element e -- one row of n_r per elements
        _noise.randn_seeded([reqs[i].seed], _noise.DRAW_AUTO_MASK, (ns[i] * Cc * h * w,), torch.float16, dev, out=z[starts[i]:starts[i] + ns[i]])
    for i, zi in enumerate(noises):
        if zi is not None:
            z[starts[i]:starts[i] + ns[i]].copy_(f16(zi))
    sch = DDIMScheduler.from_config(cfg)
    coef = torch.tensor([(1.0,) + tuple(sch.add_noise_coeffs(t)) for t, n in zip(ts, ns) for _ in range(n)], dtype=torch.float32).to(dev).contiguous()
    x = fused_update_v(x0, z, None, coef, torch.empty_like(x0))                                                    # step 3: add_noise at every request's own level
    t_rows = torch.tensor([float(t) for t, n in zip(ts, ns) for _ in range(n)], dtype=torch.float32)              # (host tables: the UNet uploads the rows of a chunk)
    sc_rows = torch.tensor([float(r.scale) for r, n in zip(reqs, ns) for _ in range(n)], dtype=torch.float32)
    size = (h * pipeline.pipe_inversion.vae_scale_factor, w * pipeline.pipe_inversion.vae_scale_factor)
    inv = lambda r, a, b: getattr(r, a) if getattr(r, a) is not None else getattr(r, b)
    src_ctx = rep([inv(r, "inv_prompt_embeds", "negative_prompt_embeds") for r in reqs])
    src_pool = rep([inv(r, "inv_pooled_prompt_embeds", "negative_pooled_prompt_embeds") for r in reqs])
    ip, _ = ipa.get_image_embeds(clip_image_embeds=torch.stack([r.latent_la.reshape(-1) for r in reqs]), mode="global")
    tgt_ctx = rep([torch.cat([f16(r.prompt_embeds), ip[i:i + 1]], dim=1) for i, r in enumerate(reqs)])             # ip_adapter.py:341
    tgt_pool = rep([r.pooled_prompt_embeds for r in reqs])
    tid = get_add_time_ids(unet, size, (0, 0), size, int(src_pool.shape[-1]))
    eps_src, eps_tgt = torch.empty_like(x), torch.empty_like(x)
    for lo in range(0, R, max_rows):
        hi = min(lo + max_rows, R)
        ctx, added = conditioning(dev, src_ctx[lo:hi], src_pool[lo:hi], tid)
        unet(x[lo:hi], t_rows[lo:hi], encoder_hidden_states=ctx, added_cond_kwargs=added, out=eps_src[lo:hi])
    for lo in range(0, R, max_rows):
        hi = min(lo + max_rows, R)
        ctx, added = conditioning(dev, tgt_ctx[lo:hi], tgt_pool[lo:hi], tid)
        unet(x[lo:hi], t_rows[lo:hi], encoder_hidden_states=ctx, added_cond_kwargs=added, out=eps_tgt[lo:hi], ip_scales=sc_rows[lo:hi])
    maps = torch.empty(len(reqs), h, w, dtype=torch.float32, device=dev)
    for i, (s0, n) in enumerate(zip(starts, ns)):                                                                  # (the requests' n differ: one launch each)
        contrast_map(eps_tgt[s0:s0 + n][None], eps_src[s0:s0 + n][None], out=maps[i:i + 1])
    masks, stats = contrast_mask(maps, [a.ratio for a in knobs], [a.dilate for a in knobs])
    return [AutoMaskEstimate(masks[i:i + 1], maps[i:i + 1], stats[i], ts[i]) for i in range(len(reqs))]


def _check_requests(pipeline, requests, knobs):
    """every refusal of the estimate before any draw or launch, naming the request"""
    for i, (r, a) in enumerate(zip(requests, knobs)):
        if a is None:
            continue
        who = f" (request {i})" if len(requests) > 1 else ""
        auto_mask_timestep(pipeline.pipe.scheduler.config, r.num_inference_steps, a.strength, who)
        if r.base_latents.ndim != 4 or int(r.base_latents.shape[0]) != 1:
            raise ValueError(f"auto_mask estimates one mask for ONE base image: base_latents must be [1, C, h, w], got {tuple(r.base_latents.shape)}{who}")


@torch.no_grad()
def estimate_requests(pipeline, requests: list, group: int = 4, max_rows: Optional[int] = None) -> list:
    """`batch.EditRequest`s -> one AutoMaskEstimate per request with an `auto_mask`, None for the others. Every refusal first, then the host draws of the unseeded
    requests in request order (`estimate_noises`), then the requests with a knob `group` at a time through `estimate_group`. Rows per evaluation: `max_rows`, else
    the smallest `max_rows` the group's knobs name, else 2 x group. Every rank of a process group runs every estimate (the stage is not sharded)."""
    knobs = [resolve_auto_mask(r.auto_mask, f" (request {i})" if len(requests) > 1 else "") for i, r in enumerate(requests)]
    _check_requests(pipeline, requests, knobs)
    noises = estimate_noises(knobs, [r.base_latents for r in requests], [r.seed for r in requests])
    live = [i for i, a in enumerate(knobs) if a is not None]
    out: list = [None] * len(requests)
    for g0 in range(0, len(live), int(group)):
        idx = live[g0:g0 + int(group)]
        named = [knobs[i].max_rows for i in idx if knobs[i].max_rows is not None]
        rows = int(max_rows) if max_rows is not None else (min(named) if named else 2 * int(group))
        est = estimate_group(pipeline, [requests[i] for i in idx], [knobs[i] for i in idx], [noises[i] for i in idx], min(rows, MAX_ROWS))
        for i, e in zip(idx, est):
            out[i] = e
    return out


@torch.no_grad()
def estimate_edit_mask(pipeline, base_latents, latent_la, *, prompt_embeds, pooled_prompt_embeds, negative_prompt_embeds=None, negative_pooled_prompt_embeds=None,
                       inv_prompt_embeds=None, inv_pooled_prompt_embeds=None, num_inference_steps=25, scale=1.0, seed=None, auto_mask=True):
    """One request on explicit conditioning (the embeddings `denoise` takes) -> (latent mask fp16 [1, 1, h, w], contrast map fp32 [1, h, w], stats fp32 [2] =
    (mean, tau)), all on the device: a group of one through `estimate_group`, n rows per evaluation unless the knob names `max_rows`."""
    from .batch import EditRequest
    a = resolve_auto_mask(auto_mask)
    if a is None:
        raise ValueError("estimate_edit_mask needs auto_mask= True, a dict or an AutoMask")
    if inv_prompt_embeds is None and negative_prompt_embeds is None:
        raise ValueError("estimate_edit_mask needs the inversion's embeddings: inv_prompt_embeds / inv_pooled_prompt_embeds, or the negative ones `denoise` falls back to")
    if seed is not None:
        seed = _noise.check_seed(seed)
    req = EditRequest(base_latents=base_latents, latent_la=latent_la, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
                      negative_prompt_embeds=negative_prompt_embeds, negative_pooled_prompt_embeds=negative_pooled_prompt_embeds, inv_prompt_embeds=inv_prompt_embeds,
                      inv_pooled_prompt_embeds=inv_pooled_prompt_embeds, num_inference_steps=num_inference_steps, scale=scale, seed=seed, auto_mask=a)
    e = estimate_requests(pipeline, [req], group=1, max_rows=a.max_rows if a.max_rows is not None else min(a.num_maps, MAX_ROWS))[0]
    return e.mask, e.map, e.stats


def intersect(auto: torch.Tensor, user: Optional[torch.Tensor]) -> torch.Tensor:
    """the latent mask an edit runs under: the estimate, times the user's latent mask where one was given"""
    return auto if user is None else (auto * user.to(device=auto.device, dtype=auto.dtype)).contiguous()


@torch.no_grad()
def apply_auto_masks(pipeline, requests: list, group: int = 4) -> list:
    """`denoise_batch`: the requests with an `auto_mask` replaced by copies whose `edit_mask` is the estimated latent mask (times their own `edit_mask`, resolved to a
    latent mask) and whose `auto_mask` is None; the others as they are"""
    from .pipeline import resolve_edit_mask
    user = [None if r.auto_mask is None or r.edit_mask is None else resolve_edit_mask(pipeline, r.edit_mask, r.base_latents, pixels=False)[1] for r in requests]
    est = estimate_requests(pipeline, requests, group=group)
    return [r if e is None else dataclasses.replace(r, edit_mask=intersect(e.mask, u), auto_mask=None) for r, e, u in zip(requests, est, user)]
