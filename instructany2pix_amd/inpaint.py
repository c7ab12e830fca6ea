"""Subject-consistency inpainting loop: the base UNet re-used with 'local' IP-Adapter tokens and a
per-step latent blend under a mask.

  StableDiffusionXLInpaintPipeline.__call__(image=, mask_image=, strength=, prompt_embeds=..., ...)
      <- the object the reference builds as `self.pipe_inpainting` from the base pipeline's own modules
         (instructany2pix/pipeline.py:132-139) and drives through `IPAdapterXL(pipe_inpainting).generate(image=, mask_image=,
         strength=subject_strength, clip_image_embeds_local=emb[None], mode='local', num_inference_steps=50, scale=0.8)`
         (instructany2pix/gdino/lib.py:89-102, called from pipeline.py:363-368)
  subject_consistency(...)   <- the loop over detected subjects of gdino/lib.py:69-104, on given masks
  subject_consistency_from_boxes(...)   <- the same loop from detector boxes: the masks come from SAM on HIP (sam.py `get_mask`); the boxes from the
                                caller or an injected detector (GroundingDINO is not built here)

The denoising loop follows diffusers 0.26.3 `StableDiffusionXLInpaintPipeline.__call__` for a 4-channel UNet: `get_timesteps`
(strength -> tail of the schedule), start latents = noise (strength 1) or `add_noise(image_latents, noise, t_0)`, the mask resized to
the latent grid (nearest) after binarising at 0.5, and after every scheduler step
    latents = (1 - mask) * add_noise(image_latents, noise, t_{i+1}) + mask * latents        (no re-noising after the last step)
with the shared DDIM scheduler. UNet: `ia2p_unet_forward`; CFG + DDIM step: `ia2p_ddim_step`; blend: `ia2p_mask_blend`.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import noise as _noise
from .ddim import StableDiffusionXLPipelineOutput, _PipelineBase, conditioning, expand_rows, get_add_time_ids
from .scheduler import DDIMScheduler, check_kept_steps, fused_update, kept_steps, mask_blend


def prepare_mask(mask_image, h: int, w: int, device) -> torch.Tensor:
    """`mask_processor.preprocess` (grayscale, binarise at 0.5, no normalisation) + `interpolate(size=(h, w))` (nearest) of
    diffusers' `prepare_mask_latents`: any [H,W] / [1,H,W] / [B,1,H,W] array in [0,1] (or uint8 0..255) -> [B,1,h,w] fp16 in {0,1}."""
    m = torch.as_tensor(mask_image)
    if m.dtype == torch.uint8:
        m = m.float() / 255.0
    m = m.float()
    while m.ndim < 4:
        m = m[None]
    if m.shape[1] != 1:
        raise ValueError(f"mask must have one channel, got shape {tuple(m.shape)}")
    m = (m >= 0.5).float()
    m = torch.nn.functional.interpolate(m, size=(h, w))
    return m.to(device=device, dtype=torch.float16).contiguous()


def prepare_region_masks(region_masks, h: int, w: int, device) -> torch.Tensor:
    """The subject masks of a joint pass on the latent grid: a list of G masks ([H,W] / [1,H,W], one per subject, the same for every row) or a [G,H,W] /
    [B,G,H,W] array -> [B or 1, G, h, w] fp16 in {0,1}, each mask through `prepare_mask`."""
    if isinstance(region_masks, (list, tuple)):
        if not region_masks:
            raise ValueError("region_masks is empty")
        return torch.cat([prepare_mask(torch.as_tensor(m).reshape(1, 1, *torch.as_tensor(m).shape[-2:]), h, w, device) for m in region_masks], 1)
    m = torch.as_tensor(region_masks)
    if m.ndim == 3:
        m = m[None]
    if m.ndim != 4:
        raise ValueError(f"region_masks must be a list of masks, [G,H,W] or [B,G,H,W]; got shape {tuple(m.shape)}")
    B, G = m.shape[:2]
    return prepare_mask(m.reshape(B * G, 1, *m.shape[2:]), h, w, device).reshape(B, G, h, w)


def union_mask(regions: torch.Tensor) -> torch.Tensor:
    """[B, G, h, w] region weights -> the blend mask [B, 1, h, w] of a joint pass: the element-wise maximum of the subject masks"""
    return regions.amax(1, keepdim=True)


def _is_pil(x) -> bool:
    if isinstance(x, list):
        return len(x) > 0 and all(_is_pil(i) for i in x)
    return type(x).__module__.startswith("PIL.")


class StableDiffusionXLInpaintPipeline(_PipelineBase):
    def get_timesteps(self, num_inference_steps: int, strength: float):
        t_start, n_steps = kept_steps(num_inference_steps, strength)
        return self.scheduler.timesteps[t_start * self.scheduler.order:], n_steps

    @torch.no_grad()
    def __call__(self, prompt=None, image=None, mask_image=None, height=None, width=None, strength: float = 0.9999,
                 num_inference_steps: int = 50, guidance_scale: float = 7.5, negative_prompt=None, num_images_per_prompt: int = 1,
                 eta: float = 0.0, generator=None, latents: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                 prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None,
                 output_type="pil", return_dict=True, callback=None, callback_steps=1, cross_attention_kwargs=None,
                 guidance_rescale: float = 0.0, original_size=None, crops_coords_top_left=(0, 0), target_size=None, noise_seed=None, noise_draw=None,
                 region_masks=None, **unused):
        """`region_masks` (a list of G subject masks, [G,H,W] or [B,G,H,W]): a JOINT subject pass -- the last 4 G rows of the prompt embeddings are G groups of
        four image tokens, group g acts where mask g says (`prepare_region_masks`; the UNet's `ip_adapter_masks`), and the blend mask is the element-wise maximum
        of the subject masks unless `mask_image` is given too (then the blend keeps to `mask_image`). Both classifier-free-guidance rows carry the same masks.
        `latents` = clean image latents (scaled) instead of `image`; `noise` = the start / re-noising noise instead of drawing it
        from `generator` (conveniences for tests and latent-space callers, as in img2img.py).
        `noise_seed` (an int, or one per batch element; None: `generator` as ever): the noise is drawn on the device from the request's own stream (noise.py:
        draw id `noise_draw`, default DRAW_INPAINT, the first subject pass). A supplied `noise` wins over the seed, the seed over `generator`."""
        if strength < 0 or strength > 1:
            raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
        if guidance_rescale != 0.0 or eta != 0.0:
            raise NotImplementedError("guidance_rescale / eta are inactive on the reference's path")
        if mask_image is None and region_masks is None:
            raise ValueError("`mask_image` input cannot be undefined.")
        self._check_embeds(prompt, prompt_embeds, pooled_prompt_embeds)
        self._check_output_type(output_type)
        do_cfg = guidance_scale > 1.0
        if prompt_embeds is None:
            prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds = self.encode_prompt(
                prompt=prompt, num_images_per_prompt=num_images_per_prompt, do_classifier_free_guidance=do_cfg, negative_prompt=negative_prompt)
        if do_cfg and (negative_prompt_embeds is None or negative_pooled_prompt_embeds is None):
            raise ValueError("classifier-free guidance needs negative_prompt_embeds and negative_pooled_prompt_embeds")
        dev = self.device
        self.scheduler.set_timesteps(num_inference_steps, device=dev)
        timesteps, n_steps = self.get_timesteps(num_inference_steps, strength)
        check_kept_steps(n_steps, strength)
        if latents is None:
            if image is None:
                raise ValueError("inpainting needs `image` (with vae= or a vae_encode callable) or `latents`")
            latents = self._image_latents(image, height, width)
        image_latents = latents.to(device=dev, dtype=torch.float16).contiguous()
        B, _, h, w = image_latents.shape
        if self.vae is not None and _is_pil(mask_image):                   # PIL mask: mask_processor (resize, grayscale, binarise at 0.5)
            mask_image = self.mask_processor.preprocess(mask_image, height=h * self.vae_scale_factor, width=w * self.vae_scale_factor)
        regions = None
        if region_masks is not None:
            regions = prepare_region_masks(region_masks, h, w, dev)
            if regions.shape[0] not in (1, B):
                raise ValueError(f"region_masks carry {regions.shape[0]} rows for a batch of {B}")
            regions = regions.expand(B, -1, -1, -1)
        mask = prepare_mask(mask_image, h, w, dev) if mask_image is not None else union_mask(regions).contiguous()
        if mask.shape[0] != B:
            mask = mask.expand(B, -1, -1, -1).contiguous()
        noise, = _noise.resolve_noises([noise], [image_latents.shape], [noise_seed], [_noise.DRAW_INPAINT if noise_draw is None else noise_draw], dev, generator)
        noise = noise.to(device=dev, dtype=torch.float16).contiguous()
        if strength == 1.0:
            x = (noise * self.scheduler.init_noise_sigma).contiguous()
        else:
            x = self.scheduler.add_noise(image_latents, noise, timesteps[:1])

        height, width = h * self.vae_scale_factor, w * self.vae_scale_factor
        original_size = original_size or (height, width)
        target_size = target_size or (height, width)
        add_time_ids = get_add_time_ids(self.unet, original_size, crops_coords_top_left, target_size, int(pooled_prompt_embeds.shape[-1]))
        neg = (expand_rows(negative_prompt_embeds, B), expand_rows(negative_pooled_prompt_embeds, B)) if do_cfg else ()
        prompt_embeds, added = conditioning(dev, expand_rows(prompt_embeds, B), expand_rows(pooled_prompt_embeds, B), add_time_ids, *neg)

        if regions is not None:
            cross_attention_kwargs = dict(cross_attention_kwargs or {}, ip_adapter_masks=(torch.cat([regions, regions], 0) if do_cfg else regions).contiguous())
        model_in = torch.cat([x, x], dim=0) if do_cfg else x.clone()
        eps = torch.empty_like(model_in)
        stepped = torch.empty_like(x)
        for i, t in enumerate(timesteps):
            t = int(t)
            self.unet(model_in, t, encoder_hidden_states=prompt_embeds, cross_attention_kwargs=cross_attention_kwargs,
                      added_cond_kwargs=added, return_dict=False, out=eps)
            c_x, c_e = self.scheduler.step_coeffs(t)
            if do_cfg:
                fused_update(model_in[:B], eps[:B], eps[B:], guidance_scale, c_x, c_e, stepped)
            else:
                fused_update(model_in, eps, None, 1.0, c_x, c_e, stepped)
            c0, c1 = self.scheduler.add_noise_coeffs(int(timesteps[i + 1])) if i < len(timesteps) - 1 else (1.0, 0.0)
            mask_blend(stepped, image_latents, noise, mask, c0, c1, model_in[:B], model_in[B:] if do_cfg else None)
            if callback is not None and i % callback_steps == 0:
                callback(i, t, model_in[:B])
        out = model_in[:B].clone()
        image_out = self._output(out, output_type)
        return StableDiffusionXLPipelineOutput(images=image_out) if return_dict else (image_out,)


def subject_consistency(subject_data, latents, ip_adapter_xl_inpaint, subject_strength: float = 0.7, joint: bool = False, **generate_kwargs):
    """The per-subject loop of reference gdino/lib.py:85-103 on given masks: `subject_data` = [(mask, subject embedding)], each pass
    re-paints the masked region guided by the subject's 'local' image tokens (50 steps, IP scale 0.8). With `noise_seed=` among the keywords, pass k
    draws its noise from draw id DRAW_INPAINT + k of that seed (unless `noise=` is supplied, which wins).
    `joint=True`: ONE pass for all subjects -- every subject's tokens in one context, each acting under its own mask, the blend under the union of the masks,
    one noise (draw id DRAW_INPAINT + 0). This is NOT the serial result: serially, pass k + 1 starts from the repaint of pass k and draws its own noise;
    jointly, all subjects are repainted from the same start under one noise."""
    if joint and len(subject_data):
        if generate_kwargs.get("noise_seed") is not None:
            generate_kwargs["noise_draw"] = _noise.inpaint_draw(0)
        embs = torch.stack([emb.reshape(-1) for _, emb in subject_data])
        return ip_adapter_xl_inpaint.generate(latents=latents, mask_image=[m for m, _ in subject_data], pil_image=None, strength=subject_strength,
                                              clip_image_embeds_local=embs, mode="local", joint=True, num_inference_steps=50, scale=0.8, **generate_kwargs)
    subject = latents
    for k, (msk, emb) in enumerate(subject_data):
        if generate_kwargs.get("noise_seed") is not None:
            generate_kwargs["noise_draw"] = _noise.inpaint_draw(k)
        subject = ip_adapter_xl_inpaint.generate(latents=subject, mask_image=msk, pil_image=None, strength=subject_strength,
                                                 clip_image_embeds_local=emb[None] if emb.ndim == 1 else emb, mode="local",
                                                 num_inference_steps=50, scale=0.8, **generate_kwargs)
    return subject


def subject_consistency_from_boxes(subject_data, latents, ip_adapter_xl_inpaint, segmenter, boxes, phrases, vae, subject_strength: float = 0.7, joint: bool = False,
                                   **generate_kwargs):
    """Reference gdino/lib.py:69-103 on given detector output: `subject_data` = [(phrase, subject embedding)], `boxes` cxcywh in [0, 1] [n, 4] with their
    `phrases`. The current result is decoded through `vae` once and set as the segmenter's image (:73); per subject the phrase loses '.' and "'s" (:86), its
    mask is `get_mask(..., d=40, b=20)` (:87) and the inpaint pass of `subject_consistency` follows. Boxes are scaled by the decoded image's longer side
    (the reference's literal 1024 is the side of the images it generates). -> (latents, masks as PIL images)"""
    pairs, masks = subject_masks_from_boxes(subject_data, latents, segmenter, boxes, phrases, vae)
    return subject_consistency(pairs, latents, ip_adapter_xl_inpaint, subject_strength, joint=joint, **generate_kwargs), masks


def subject_masks_from_boxes(subject_data, latents, segmenter, boxes, phrases, vae):
    """The mask half of `subject_consistency_from_boxes` (gdino/lib.py:69-87): every subject's mask from the ONE decode of `latents`, before any pass
    repaints it. -> ([(mask tensor, subject embedding)] for `subject_consistency`, masks as PIL images)"""
    import numpy as np
    from .sam import get_mask
    if segmenter is None:
        raise ValueError("subjects given as (phrase, embedding) need the pipeline built with segmenter=<HipSamPredictor>")
    if vae is None:
        raise ValueError("subjects given as (phrase, embedding) need the pipeline built with vae=<HipAutoencoderKL> (the segmenter sees the decoded image)")
    if boxes is None or phrases is None:
        raise KeyError("subjects given as (phrase, embedding) need boxes and phrases: build the pipeline with detector= or return c['subject_boxes'] = (boxes, phrases)")
    x = vae.decode_from_latents(latents)[:1]                                  # [-1, 1]; the 8-bit image of `postprocess(output_type="pil")`
    a = ((x.float() / 2 + 0.5).clamp(0, 1) * 255.0).round().to(torch.uint8)[0].permute(1, 2, 0).cpu().numpy()
    segmenter.set_image(np.ascontiguousarray(a))
    masks = [get_mask(ph.replace(".", "").replace("'s", ""), boxes, phrases, segmenter, i=0, d=40, b=20, size=max(a.shape[0], a.shape[1])) for ph, _ in subject_data]
    return [(torch.from_numpy(np.array(m)), emb) for m, (_, emb) in zip(masks, subject_data)], masks
